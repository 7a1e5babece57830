"""The point-wise middle of a ConvNeXt block in training (unicorn/models/backbone/convnext.py:46-48: pwconv1 -> GELU -> pwconv2), forward +
backward, at the four stage shapes of unicorn_track_large at 800 x 1280 with the two frames of one sample, fp32 and fp16 autocast.

Part 1, the operator: ops.pw_mlp with keep="hidden" and with keep="input" against the three eager lines on the same GPU in the same run (the
eager lines are what a model without fuse_pw_mlp runs).  Part 2, the stand-in stages of tools/lncf_bench.py (norm + 2x2 stride-2 convolution +
three blocks + output norm) with fuse_backbone against fuse_backbone_mlp in both modes.

HIP events around every call, 3 warm-up calls, two alternating windows, median of the timed calls; the two window medians are printed, their
distance is the run-to-run spread a difference has to exceed.  Kernel launches of one call and the sum of their device times from
torch.profiler (a run of its own; copies and fills left out); peak memory of one call; bytes held between forward and backward
(torch.cuda.memory_allocated after the forward, the inputs and parameters not counted).

    python tools/pw_mlp_bench.py [--runs 20] [--out profiles/pw_mlp.txt]
"""
import argparse
import copy
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lncf_ref as RL  # noqa: E402
import pw_mlp_ref as R  # noqa: E402
from block_tail_bench import device_of  # noqa: E402
from dwln_train_bench import peak_of, timed  # noqa: E402
from unicorn_amd import nn as unn, ops  # noqa: E402

CL = torch.channels_last
SHAPES = ((2, 192, 200, 320), (2, 384, 100, 160), (2, 768, 50, 80), (2, 1536, 25, 40))
STAGES = ((2, 384, 100, 160), (2, 768, 50, 80), (2, 1536, 25, 40))


def windows(fns, runs):
    """[(median of window 1, median of window 2)] of every function, the functions alternating"""
    first = [timed(f, runs)[1] for f in fns]
    second = [timed(f, runs)[1] for f in fns]
    return list(zip(first, second))


def held_of(fwd):
    """MB allocated by a forward and still held when it returns (what waits for the backward, the output included)"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    out = fwd()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    del out
    return held / 1e6


def report(say, label, names, fns, fwds, runs):
    """one line per function; -> {name: (median ms, spread ms)}"""
    res = {}
    for name, (t1, t2), fn, fwd in zip(names, windows(fns, runs), fns, fwds):
        n, dev = device_of(fn)
        med = statistics.median([t1, t2])
        res[name] = (med, abs(t1 - t2))
        say("  %-14s %-7s %8.3f ms call (windows %8.3f / %8.3f), %8.3f ms device in %3d launches, peak %7.1f MB, held for the backward %7.1f MB"
            % (label, name, med, t1, t2, dev, n, peak_of(fn), held_of(fwd)))
    return res


def operator_part(say, runs):
    slower = []
    for shape in SHAPES:
        N, C, H, W = shape
        M, Hd = N * H * W, 4 * C
        t, w1, b1, w2, b2, g = (x.cuda() for x in R.draw("plain", C, ((N, H, W), C, Hd, C)))
        leaves = (t, w1, b1, w2, b2)
        for x in leaves:
            x.requires_grad_(True)
        say()
        say("(%d, %d, %d, %d): M = %d rows, C = %d -> Hd = %d; one (M, Hd) map is %.1f MB in fp32, %.1f MB in fp16"
            % (N, C, H, W, M, C, Hd, 4e-6 * M * Hd, 2e-6 * M * Hd))
        for autocast in (False, True):
            def fwd_of(kind):
                def fwd():
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        if kind == "eager":
                            return F.linear(F.gelu(F.linear(t, w1, b1)), w2, b2)
                        return ops.pw_mlp(t, w1, b1, w2, b2, keep=kind)
                return fwd

            def step_of(fwd):
                def fn():
                    for x in leaves:
                        x.grad = None
                    y = fwd()
                    y.backward(g.to(y.dtype))
                return fn

            names = ("eager", "hidden", "input")
            fwds = [fwd_of(k) for k in names]
            label = "fp16 autocast" if autocast else "fp32"
            res = report(say, label, names, [step_of(f) for f in fwds], fwds, runs)
            te, se = res["eager"]
            for k in ("hidden", "input"):
                tk, sk = res[k]
                flag = ""
                if tk > te:
                    flag = "   SLOWER" + (" (inside the spread of the windows)" if tk - te <= max(se, sk) else " BY MORE THAN THE SPREAD OF THE WINDOWS")
                    slower.append("%s %s %s: %.3f against %.3f ms" % (shape, label, k, tk, te))
                say("  %-14s %-7s / eager = %.3f x call time%s" % (label, k, tk / te, flag))
    say()
    say("operator slower than the eager lines by call time at: %s" % ("; ".join(slower) or "no measured case"))


def stage_part(say, runs):
    slower = []
    for shape in STAGES:
        N, C, H, W = shape
        torch.manual_seed(C)
        proto = nn.Sequential(RL.StandInNorm(C // 2, data_format="channels_first"), nn.Conv2d(C // 2, C, kernel_size=2, stride=2),
                              *(RL.StandInBlock(C) for _ in range(3)), RL.StandInNorm(C, data_format="channels_first")).cuda().train()
        x = torch.randn(N, C // 2, 2 * H, 2 * W, device="cuda").contiguous(memory_format=CL)       # the output of the stage before
        t = torch.randn(N, C, H, W, device="cuda")
        say()
        say("stage of (%d, %d, %d, %d): norm + 2x2 stride-2 convolution + 3 blocks + output norm" % shape)
        for autocast in (False, True):
            nets = {"backbone": copy.deepcopy(proto), "hidden": copy.deepcopy(proto), "input": copy.deepcopy(proto)}
            unn.fuse_backbone(nets["backbone"])
            unn.fuse_backbone_mlp(nets["hidden"], "hidden")
            unn.fuse_backbone_mlp(nets["input"], "input")

            def fwd_of(net):
                def fwd():
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        return net(x)
                return fwd

            def step_of(net, fwd):
                def fn():
                    net.zero_grad(set_to_none=True)
                    (fwd() * t).sum().backward()
                return fn

            names = ("backbone", "hidden", "input")
            fwds = [fwd_of(nets[n]) for n in names]
            label = "fp16 autocast" if autocast else "fp32"
            res = report(say, label, names, [step_of(nets[n], f) for n, f in zip(names, fwds)], fwds, runs)
            tb, sb = res["backbone"]
            for k in ("hidden", "input"):
                tk, sk = res[k]
                flag = ""
                if tk > tb:
                    flag = "   SLOWER" + (" (inside the spread of the windows)" if tk - tb <= max(sb, sk) else " BY MORE THAN THE SPREAD OF THE WINDOWS")
                    slower.append("%s %s %s: %.3f against %.3f ms" % (shape, label, k, tk, tb))
                say("  %-14s fuse_backbone_mlp(%s) / fuse_backbone = %.3f x call time%s" % (label, k, tk / tb, flag))
            del nets
    say()
    say("stage with fuse_backbone_mlp slower than with fuse_backbone at: %s" % ("; ".join(slower) or "no measured case"))


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

    say("pwconv1 -> GELU -> pwconv2, training (forward + backward) -- tools/pw_mlp_bench.py on %s" % torch.cuda.get_device_name(0))
    say("eager = F.linear(F.gelu(F.linear(t, w1, b1)), w2, b2); hidden / input = ops.pw_mlp(keep=...).  HIP events, 3 warm-up calls, median of %d"
        % args.runs)
    say("calls in each of two alternating windows; the GEMMs are the vendor library's in all three.")
    if args.part in ("operator", "both"):
        operator_part(say, args.runs)
    if args.part in ("stage", "both"):
        stage_part(say, args.runs)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
