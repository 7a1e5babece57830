"""The channels-first LayerNorm between the ConvNeXt stages in training (unicorn/models/backbone/convnext.py:160-184), forward + backward, at
its seven sites in unicorn_track_large at 800 x 1280 with the two frames of one sample: after the stem (NCHW, fp32 and the fp16 that the stem
convolution returns under autocast), before the three downsample convolutions (channels-last memory, what ops.block_tail writes) and on the
three stage outputs (channels-last in a fused model, NCHW in an unfused one).

Part 1, the operator: ops.layernorm_cf (uni_lncf_train_fwd / _bwd) against the eager lines on the same GPU in the same run, the two
alternating.  Part 2, a stand-in stage with the norms included: norm + 2x2 stride-2 convolution + three blocks (tests/block_tail_ref.py
StandInBlock) + output norm, with fuse_backbone, with fuse_convnext and with neither, fp32 and fp16 autocast.

HIP events around every call, 3 warm-up calls, two alternating windows, median of the timed calls; kernel launches of one call and the sum of
their device times from torch.profiler (a run of its own; copies and fills left out); peak memory of one call; achieved bytes per second of the
operator against the algorithmic bytes (forward reads x and writes y, backward reads x and grad_y and writes grad_x), over the call time and
over the device time.  A call of a few tens of microseconds of kernels is bound by the host: the call time then measures Python and the
launch path, the device time what the GPU is busy for, which is what a training step that keeps the queue full pays.

    python tools/lncf_bench.py [--runs 20] [--out profiles/lncf_train.txt]
"""
import argparse
import copy
import os
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lncf_ref as R  # noqa: E402
from block_tail_bench import device_of, two_windows  # noqa: E402
from dwln_train_bench import peak_of, timed  # noqa: E402
from unicorn_amd import nn as unn, ops  # noqa: E402

CL, NCHW = torch.channels_last, torch.contiguous_format
# (site, shape, memory layout, dtype of x)
SITES = (("stem", (2, 192, 200, 320), NCHW, torch.float32), ("stem", (2, 192, 200, 320), NCHW, torch.float16),
         ("downsample 1", (2, 192, 200, 320), CL, torch.float32), ("downsample 2", (2, 384, 100, 160), CL, torch.float32),
         ("downsample 3", (2, 768, 50, 80), CL, torch.float32),
         ("output 1", (2, 384, 100, 160), CL, torch.float32), ("output 2", (2, 768, 50, 80), CL, torch.float32),
         ("output 3", (2, 1536, 25, 40), CL, torch.float32),
         ("output 1", (2, 384, 100, 160), NCHW, torch.float32), ("output 2", (2, 768, 50, 80), NCHW, torch.float32),
         ("output 3", (2, 1536, 25, 40), NCHW, torch.float32))
STAGES = ((2, 384, 100, 160), (2, 768, 50, 80), (2, 1536, 25, 40))


def operator_part(say, runs):
    slower, slower_dev = [], []
    for site, shape, layout, xdt in SITES:
        N, C, H, W = shape
        x, w, b, g = (t.cuda() for t in R.draw("plain", C, shape))
        x = x.to(xdt).contiguous(memory_format=layout).requires_grad_(True)
        g = g.contiguous(memory_format=layout)
        w.requires_grad_(True), b.requires_grad_(True)

        def clear():
            x.grad = w.grad = b.grad = None

        def hip():
            clear()
            ops.layernorm_cf(x, w, b, R.EPS).backward(g)

        def eager():
            clear()
            R.forward(x, w, b, R.EPS).backward(g)

        th, te = two_windows(hip, eager, runs)
        ph, pe = peak_of(hip), peak_of(eager)
        (lh, dh), (le, de) = device_of(hip), device_of(eager)
        ex = x.element_size()
        nbytes = ((ex + 4) + (ex + 4 + ex)) * 1e-12 * N * C * H * W
        lname = "channels-last" if layout is CL else "NCHW"
        flag = "   SLOWER" if te < th else ""
        if de < dh:
            flag += "   SLOWER ON THE DEVICE"
            slower_dev.append((site, shape, lname, str(xdt)))
        if te < th:
            slower.append((site, shape, lname, str(xdt)))
        say("  %-12s %-20s %-13s %-4s HIP %7.4f ms call, %7.4f ms device in %d launches (%.2f / %.2f TB/s), peak %6.1f MB   eager %7.4f ms call, "
            "%7.4f ms device in %d launches, peak %6.1f MB   eager / HIP %.2f x call, %.2f x device%s"
            % (site, shape, lname, "fp16" if xdt == torch.float16 else "fp32", th, dh, lh, nbytes / (th * 1e-3), nbytes / (dh * 1e-3), ph, te, de,
               le, pe, te / th, de / dh, flag))
    say()
    say("operator slower than the eager lines by call time at: %s" % ("; ".join(str(s) for s in slower) or "no measured case"))
    say("operator slower than the eager lines by device time at: %s" % ("; ".join(str(s) for s in slower_dev) or "no measured case"))


def stage_part(say, runs):
    slower = []
    for shape in STAGES:
        N, C, H, W = shape
        torch.manual_seed(C)
        proto = nn.Sequential(R.StandInNorm(C // 2, data_format="channels_first"), nn.Conv2d(C // 2, C, kernel_size=2, stride=2),
                              *(R.StandInBlock(C) for _ in range(3)), R.StandInNorm(C, data_format="channels_first")).cuda().train()
        x = torch.randn(N, C // 2, 2 * H, 2 * W, device="cuda").contiguous(memory_format=CL)       # the output of the stage before
        t = torch.randn(N, C, H, W, device="cuda")
        say()
        say("stage of (%d, %d, %d, %d): norm + 2x2 stride-2 convolution + 3 blocks + output norm" % shape)
        for autocast in (False, True):
            nets = {}
            for name, fuse in (("fuse_backbone", unn.fuse_backbone), ("fuse_convnext", unn.fuse_convnext), ("neither", None)):
                nets[name] = copy.deepcopy(proto)
                if fuse:
                    fuse(nets[name])

            def step(net):
                def fn():
                    net.zero_grad(set_to_none=True)
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        out = net(x)
                    (out * t).sum().backward()
                return fn

            full, cn, none = (step(nets[n]) for n in ("fuse_backbone", "fuse_convnext", "neither"))
            tf, tc = two_windows(full, cn, runs)
            tn = timed(none, runs)[1]
            say("  %-14s fuse_backbone %8.3f ms (%s launches, peak %7.1f MB)   fuse_convnext %8.3f ms (%s launches, peak %7.1f MB)   "
                "neither %8.3f ms (%s launches, peak %7.1f MB)   fuse_convnext / fuse_backbone %.3f x%s"
                % ("fp16 autocast" if autocast else "fp32", tf, device_of(full)[0], peak_of(full), tc, device_of(cn)[0], peak_of(cn), tn,
                   device_of(none)[0], peak_of(none), tc / tf, "   SLOWER" if tc < tf else ""))
            if tc < tf:
                slower.append((shape, "fp16 autocast" if autocast else "fp32"))
            del nets
    say()
    say("stage with fuse_backbone slower than with fuse_convnext at: %s" % ("; ".join(str(s) for s in slower) or "no measured case"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("operator", "stage", "both"), default="both")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the measurement needs a HIP device"
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Channels-first LayerNorm, training (forward + backward) -- tools/lncf_bench.py on %s" % torch.cuda.get_device_name(0))
    say("HIP = ops.layernorm_cf; eager = the reference's four lines (mean, centred square mean, division, weight * x + bias).  HIP events, 3 warm-up")
    say("calls, median of %d calls in each of two alternating windows.  TB/s: the algorithmic bytes (x + y forward, x + grad_y + grad_x backward)" % args.runs)
    say("over call / device time.")
    if args.part in ("operator", "both"):
        say()
        operator_part(say, args.runs)
    if args.part in ("stage", "both"):
        stage_part(say, args.runs)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
