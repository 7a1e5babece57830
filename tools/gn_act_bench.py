"""GroupNorm + SiLU behind the backbone in training (unicorn/models/backbone/network_blocks.py:29-51 after convert_bn_model_to_gn:
act(bn(conv(x))) with bn = GroupNorm(16, C, eps=1e-3), act = SiLU(inplace=True)), forward + backward, at the map sizes of the YOLOX-PAFPN and
of the head in unicorn_track_large at 800 x 1280 with the two frames of one sample: widths 192 / 384 / 768 / 1536 at strides 8 / 16 / 32 and the
head's 256.

Part 1, the operator: ops.group_norm_act (uni_gn_act_train_fwd / _bwd) against the eager lines act_(F.group_norm(x)) on the same GPU in the
same run, the two alternating, fp32 and fp16 autocast (x is the half map a convolution returns there), NCHW and channels-last memory.
Part 2, a stand-in neck (tests/gn_act_ref.py: BaseConv stand-ins with an upsample, a concat and a residual add) with and without
fuse_groupnorm_act.

HIP events around every call, 3 warm-up calls, two alternating windows, median of the timed calls; kernel launches of one call and the sum of
their device times from torch.profiler (a run of its own; copies and fills left out); the bytes autograd holds between forward and backward
(torch.autograd.graph.saved_tensors_hooks, every storage once); peak memory of one call; achieved bytes per second of the operator against
the counted bytes (forward: two reads of x and one write of y; backward: two reads of x, two of grad_y and one write of grad_x), over the call
time and over the device time.

    python tools/gn_act_bench.py [--runs 20] [--out profiles/gn_act.txt]
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gn_act_ref as R  # noqa: E402
from block_tail_bench import device_of, two_windows  # noqa: E402
from dwln_train_bench import peak_of  # noqa: E402
from unicorn_amd import nn as unn, ops  # noqa: E402

CL, NCHW = torch.channels_last, torch.contiguous_format
SHAPES = ((2, 192, 100, 160), (2, 384, 100, 160), (2, 256, 100, 160), (2, 384, 50, 80), (2, 768, 50, 80), (2, 256, 50, 80), (2, 768, 25, 40),
          (2, 1536, 25, 40))
G, EPS = 16, 1e-3


def held_bytes(forward):
    """bytes of the storages autograd saves in one forward"""
    seen = {}

    def pack(t):
        s = t.untyped_storage()
        seen[s.data_ptr()] = s.nbytes()
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = forward()
    del out
    return sum(seen.values())


def operator_part(say, runs):
    slower, slower_dev = [], []
    for shape in SHAPES:
        N, C, H, W = shape
        for layout in (NCHW, CL):
            for autocast in (False, True):
                x, w, b, g = (t.cuda() for t in R.draw("plain", C, shape))
                x = x.to(torch.float16 if autocast else torch.float32).contiguous(memory_format=layout).requires_grad_(True)
                g = g.contiguous(memory_format=layout)
                w.requires_grad_(True), b.requires_grad_(True)

                def clear():
                    x.grad = w.grad = b.grad = None

                def hip_fwd():
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        return ops.group_norm_act(x, G, w, b, EPS, "silu")

                def eager_fwd():
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        return F.silu(F.group_norm(x, G, w, b, EPS), inplace=True)

                def hip():
                    clear()
                    hip_fwd().backward(g)

                def eager():
                    clear()
                    eager_fwd().backward(g)

                th, te = two_windows(hip, eager, runs)
                _, te2 = two_windows(hip, eager, runs)                      # the spread of repeating the eager side
                ph, pe = peak_of(hip), peak_of(eager)
                (lh, dh), (le, de) = device_of(hip), device_of(eager)
                (_, _), (_, de2) = device_of(hip), device_of(eager)
                hh, he = held_bytes(hip_fwd), held_bytes(eager_fwd)
                ex = x.element_size()
                nbytes = ((2 * ex + 4) + (2 * ex + 2 * 4 + ex)) * 1e-12 * N * C * H * W
                lname = "channels-last" if layout is CL else "NCHW"
                key = (shape, lname, "fp16 autocast" if autocast else "fp32")
                flag = "   SLOWER" if te < th else ""
                if max(de, de2) < dh:
                    flag += "   SLOWER ON THE DEVICE"
                    slower_dev.append(key)
                if te < th:
                    slower.append(key)
                say("  %-20s %-13s %-13s HIP %7.4f ms call, %7.4f ms device in %d launches (%.2f / %.2f TB/s), holds %6.1f MB, peak %6.1f MB   eager "
                    "%7.4f ms call (again %7.4f), %7.4f ms device (again %7.4f) in %d launches, holds %6.1f MB, peak %6.1f MB   eager / HIP %.2f x call, "
                    "%.2f x device%s" % (shape, lname, key[2], th, dh, lh, nbytes / (th * 1e-3), nbytes / (dh * 1e-3), hh / 2 ** 20, ph, te, te2, de, de2,
                                         le, he / 2 ** 20, pe, te / th, de / dh, flag))
    say()
    say("operator slower than the eager lines by call time at: %s" % ("; ".join(str(s) for s in slower) or "no measured case"))
    say("operator slower than the eager lines by device time, beyond the two eager measurements, at: %s"
        % ("; ".join(str(s) for s in slower_dev) or "no measured case"))


def neck_part(say, runs):
    torch.manual_seed(3)
    C = 192
    proto = R.MiniNeck(C).cuda().train()
    fine, coarse = torch.randn(2, C, 100, 160, device="cuda"), torch.randn(2, 2 * C, 50, 80, device="cuda")
    t = torch.randn(2, 2 * C, 100, 160, device="cuda")
    say()
    say("stand-in neck (tests/gn_act_ref.py MiniNeck(%d)) on maps (2, %d, 100, 160) and (2, %d, 50, 80): five GroupNorm sites" % (C, C, 2 * C))
    for autocast in (False, True):
        fused, plain = copy.deepcopy(proto), copy.deepcopy(proto)
        assert unn.fuse_groupnorm_act(fused) == 5

        def step(net):
            def fn():
                net.zero_grad(set_to_none=True)
                with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                    out = net(fine, coarse)
                (out * t).sum().backward()
            return fn

        f, p = step(fused), step(plain)
        tf, tp = two_windows(f, p, runs)
        (lf, df), (lp, dp) = device_of(f), device_of(p)
        say("  %-14s fuse_groupnorm_act %8.3f ms call, %8.3f ms device (%s launches, peak %7.1f MB)   unfused %8.3f ms call, %8.3f ms device (%s "
            "launches, peak %7.1f MB)   unfused / fused %.3f x call, %.3f x device%s"
            % ("fp16 autocast" if autocast else "fp32", tf, df, lf, peak_of(f), tp, dp, lp, peak_of(p), tp / tf, dp / df, "   SLOWER" if tp < tf else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("operator", "neck", "both"), default="both")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs a HIP device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("GroupNorm(16, C, eps=1e-3) + SiLU, training (forward + backward) -- tools/gn_act_bench.py on %s" % torch.cuda.get_device_name(0))
    say("HIP = ops.group_norm_act; eager = F.silu(F.group_norm(x, 16, weight, bias, 1e-3), inplace=True).  HIP events, 3 warm-up calls, median of")
    say("%d calls in each of two alternating windows; `again`: the eager side measured a second time.  TB/s: the counted bytes (forward 2 x + y," % args.runs)
    say("backward 2 x + 2 grad_y + grad_x) over call / device time.  holds: the storages autograd keeps between forward and backward.")
    if args.part in ("operator", "both"):
        say()
        operator_part(say, args.runs)
    if args.part in ("neck", "both"):
        neck_part(say, args.runs)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
