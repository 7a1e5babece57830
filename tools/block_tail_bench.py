"""The close of a ConvNeXt block in training (unicorn/models/backbone/convnext.py:49-53: layer scale, permute, input + drop_path), forward +
backward, at the four stage shapes of unicorn_track_large at 800 x 1280 with the two frames of one sample.

Part 1, the operator: ops.block_tail (uni_block_tail_fwd / _bwd) against the eager lines on the same GPU in the same run, the two alternating,
for residual / grad_out in channels-last and in NCHW-contiguous memory, without drop path, with drop_prob 0.7 and both samples kept (the factor
is 1 / 0.3 for both: the most work) and with one of the two dropped, in fp32 and with an fp16 y (what pwconv2 hands over under autocast).
Part 2, a stand-in stage: a 2x2 stride-2 convolution and three blocks (tests/block_tail_ref.py StandInBlock, DropPath(0.7), seeded per call so
that every configuration drops the same samples) with fuse_convnext, with fuse_dwconv_ln alone and with neither, fp32 and fp16 autocast.

HIP events around every call, 3 warm-up calls, two alternating windows, median of the timed calls; kernel launches of one call and the sum of
their device times from torch.profiler (a run of its own; copies left out: the copy autograd makes when it stores grad_out in residual.grad is
the same on both sides); peak memory of one call; achieved bytes per second of the operator against the algorithmic bytes (forward reads y
and the residual and writes out; backward reads grad_out and y and writes grad_y: three maps each way), over the call time and over the
device time.  A call of a few tens of microseconds of kernels is bound by the host: the call time then measures Python and the launch path,
the device time what the GPU is busy for, which is what a training step that keeps the queue full pays.

    python tools/block_tail_bench.py [--runs 20] [--out profiles/block_tail.txt]
"""
import argparse
import copy
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import block_tail_ref as R  # noqa: E402
from dwln_train_bench import peak_of, timed  # noqa: E402
from unicorn_amd import nn as unn, ops  # noqa: E402

SHAPES = ((2, 192, 200, 320), (2, 384, 100, 160), (2, 768, 50, 80), (2, 1536, 25, 40))
CL = torch.channels_last
DROPS = (("no drop path", None), ("p=0.7, both kept", (1 / 0.3, 1 / 0.3)), ("p=0.7, one dropped", (1 / 0.3, 0.0)))


def device_of(fn):
    """(kernel launches, the sum of their device times in ms) of one call (torch.profiler, device activity; copies and fills left out)"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
          and "memset" not in e.name.lower()]
    return len(ev), sum(e.time_range.elapsed_us() for e in ev) * 1e-3


def two_windows(a, b, runs):
    """medians of a and b over two alternating windows each"""
    ta, tb = timed(a, runs)[1], timed(b, runs)[1]
    ta2, tb2 = timed(a, runs)[1], timed(b, runs)[1]
    return statistics.median([ta, ta2]), statistics.median([tb, tb2])


def operator_part(say, runs):
    slower, slower_dev = [], []
    for shape in SHAPES:
        N, C, H, W = shape
        say()
        say("(%d, %d, %d, %d): %.1f MB per fp32 map" % (N, C, H, W, 4e-6 * N * C * H * W))
        for half in (False, True):
            for layout, lname in ((CL, "channels-last"), (torch.contiguous_format, "NCHW")):
                for dname, scale in DROPS:
                    y, res, gamma, sc, g = (None if t is None else t.cuda() for t in R.draw("plain", C, shape, scale=scale))
                    y = (y.half() if half else y).requires_grad_(True)
                    res = res.contiguous(memory_format=layout).requires_grad_(True)
                    g = g.contiguous(memory_format=layout)
                    gamma.requires_grad_(True)

                    def clear():
                        y.grad = res.grad = gamma.grad = None

                    def hip():
                        clear()
                        ops.block_tail(y, res, gamma, sc).backward(g)

                    def eager():
                        clear()
                        R.forward(y, res, gamma, sc).backward(g)

                    th, te = two_windows(hip, eager, runs)
                    ph, pe = peak_of(hip), peak_of(eager)
                    (lh, dh), (le, de) = device_of(hip), device_of(eager)
                    ey = 2 if half else 4
                    nbytes = (3 * ey + 3 * 4) * 1e-12 * N * C * H * W
                    flag = "   SLOWER" if te < th else ""
                    if de < dh:
                        flag += "   SLOWER ON THE DEVICE"
                        slower_dev.append((shape, half, lname, dname))
                    say("  %-4s %-13s %-18s HIP %7.4f ms call, %7.4f ms device in %d launches (%.2f / %.2f TB/s), peak %6.1f MB   eager %7.4f ms call, "
                        "%7.4f ms device in %d launches, peak %6.1f MB   eager / HIP %.2f x call, %.2f x device%s"
                        % ("fp16" if half else "fp32", lname, dname, th, dh, lh, nbytes / (th * 1e-3), nbytes / (dh * 1e-3), ph, te, de, le, pe,
                           te / th, de / dh, flag))
                    if te < th:
                        slower.append((shape, half, lname, dname))
    say()
    say("operator slower than the eager lines by call time at: %s" % ("; ".join(str(s) for s in slower) or "no measured case"))
    say("operator slower than the eager lines by device time at: %s" % ("; ".join(str(s) for s in slower_dev) or "no measured case"))
    return slower


def stage_part(say, runs):
    slower = []
    for shape in SHAPES:
        N, C, H, W = shape
        torch.manual_seed(C)
        proto = nn.Sequential(nn.Conv2d(C // 2, C, kernel_size=2, stride=2), *(R.StandInBlock(C, drop_path=0.7) for _ in range(3))).cuda().train()
        x = torch.randn(N, C // 2, 2 * H, 2 * W, device="cuda")
        t = torch.randn(N, C, H, W, device="cuda")
        say()
        say("stage of (%d, %d, %d, %d): 2x2 stride-2 convolution + 3 blocks, DropPath(0.7)" % shape)
        for autocast in (False, True):
            nets = {}
            for name, fuse in (("fuse_convnext", unn.fuse_convnext), ("fuse_dwconv_ln alone", unn.fuse_dwconv_ln), ("neither", None)):
                nets[name] = copy.deepcopy(proto)
                if fuse:
                    fuse(nets[name])

            def step(net):
                def fn():
                    net.zero_grad(set_to_none=True)
                    torch.manual_seed(1)
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        out = net(x)
                    (out * t).sum().backward()
                return fn

            both, dw, none = (step(nets[n]) for n in ("fuse_convnext", "fuse_dwconv_ln alone", "neither"))
            tb, td = two_windows(both, dw, runs)
            tn = timed(none, runs)[1]
            say("  %-14s fuse_convnext %8.3f ms (%s launches, peak %7.1f MB)   fuse_dwconv_ln alone %8.3f ms (%s launches, peak %7.1f MB)   "
                "neither %8.3f ms (%s launches, peak %7.1f MB)   dwconv_ln alone / both %.3f x%s"
                % ("fp16 autocast" if autocast else "fp32", tb, device_of(both)[0], peak_of(both), td, device_of(dw)[0], peak_of(dw), tn,
                   device_of(none)[0], peak_of(none), td / tb, "   SLOWER" if td < tb else ""))
            if td < tb:
                slower.append((shape, "fp16 autocast" if autocast else "fp32"))
            del nets
    say()
    say("stage with both fusions slower than with fuse_dwconv_ln alone at: %s" % ("; ".join(str(s) for s in slower) or "no measured case"))
    return slower


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

    say("ConvNeXt block tail, training (forward + backward) -- tools/block_tail_bench.py on %s" % torch.cuda.get_device_name(0))
    say("HIP = ops.block_tail; eager = gamma * y, permute, residual + x * mask (the reference's lines with timm's per-sample factor).  HIP events,")
    say("3 warm-up calls, median of %d calls in each of two alternating windows.  TB/s: the algorithmic bytes (three maps each way) over call / device time." % args.runs)
    if args.part in ("operator", "both"):
        operator_part(say, args.runs)
    if args.part in ("stage", "both"):
        stage_part(say, args.runs)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
