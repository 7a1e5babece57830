"""The opening of a ConvNeXt block in training (unicorn/models/backbone/convnext.py:43-45: depthwise 7x7, permute, LayerNorm over C), forward +
backward with all five gradients, at the four stage shapes of unicorn_track_large at 800 x 1280 with the two frames of one sample:
ops.dwconv7_ln (uni_dwln_train_fwd / _bwd) against the reference's three eager lines in fp32 on an NCHW-contiguous input, on the same GPU in
the same run, the two alternating shape by shape; as context only, the same eager lines under fp16 autocast (how the reference trains).
HIP events around every call, 3 warm-up calls, min / median of the timed calls; kernel launches of one call counted by torch.profiler; peak
memory of one call; achieved bytes per second of the operator against the algorithmic bytes (forward reads x and writes y; backward reads x
and grad_y, writes and re-reads du, writes dx: 8 maps of N C H W elements).

    python tools/dwln_train_bench.py [--runs 20] [--out profiles/dwln_train.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dwln_train_ref as R  # noqa: E402
from unicorn_amd import ops  # noqa: E402

SHAPES = ((2, 192, 200, 320), (2, 384, 100, 160), (2, 768, 50, 80), (2, 1536, 25, 40))


def timed(fn, runs, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), statistics.median(ts)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def launches_of(fn):
    """kernel launches of one call (torch.profiler, device activity), or None where the profiler reports none"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
            and "memset" not in e.name.lower())
    return n or None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("Depthwise 7x7 + LayerNorm, training (forward + backward, five gradients), fp32 -- tools/dwln_train_bench.py on %s" % torch.cuda.get_device_name(0))
    say("HIP = ops.dwconv7_ln on a channels-last x; eager = F.conv2d(groups=C) + permute + F.layer_norm on an NCHW-contiguous x (the reference's")
    say("lines); eager fp16 = the same under torch.autocast (context only).  HIP events, 3 warm-up calls, min / median of %d calls, alternating." % args.runs)
    slower = []
    for shape in SHAPES:
        N, C, H, W = shape
        ins = [t.cuda() for t in R.draw("plain", C, shape)]
        gy = ins[5]
        x_cl = ins[0].contiguous(memory_format=torch.channels_last).requires_grad_(True)
        x_nchw = ins[0].contiguous().requires_grad_(True)
        params = [t.requires_grad_(True) for t in ins[1:5]]

        def clear(x):
            x.grad = None
            for p in params:
                p.grad = None

        def hip():
            clear(x_cl)
            ops.dwconv7_ln(x_cl, *params).backward(gy)

        def eager():
            clear(x_nchw)
            R.forward(x_nchw, *params).backward(gy)

        def eager_fp16():
            clear(x_nchw)
            with torch.autocast("cuda", torch.float16):
                y = R.forward(x_nchw, *params)
            y.backward(gy)

        def hip_fwd():
            with torch.no_grad():
                ops.DwConv7LNFunction.apply(x_cl, *params, R.EPS)

        say()
        say("x (%d, %d, %d, %d): %.1f MB per map" % (N, C, H, W, 4e-6 * N * C * H * W))
        th, te = timed(hip, args.runs), timed(eager, args.runs)
        th2, te2 = timed(hip, args.runs), timed(eager, args.runs)                  # alternate: the second window of each
        th, te = (min(th[0], th2[0]), statistics.median([th[1], th2[1]])), (min(te[0], te2[0]), statistics.median([te[1], te2[1]]))
        t16 = timed(eager_fp16, args.runs)
        tf = timed(hip_fwd, args.runs)
        ph, pe, p16 = peak_of(hip), peak_of(eager), peak_of(eager_fp16)
        lh, le, l16 = launches_of(hip), launches_of(eager), launches_of(eager_fp16)
        gbs = 8 * 4e-9 * N * C * H * W / (th[1] * 1e-3)
        say("  HIP dwconv7_ln + backward          min %8.4f ms   median %8.4f ms   launches %s   peak %8.1f MB   %.2f TB/s of 8 maps" % (th + (lh, ph, gbs / 1e3)))
        say("    of which the forward alone       min %8.4f ms   median %8.4f ms" % tf)
        say("  eager fp32 three lines + backward  min %8.4f ms   median %8.4f ms   launches %s   peak %8.1f MB" % (te + (le, pe)))
        say("  eager fp16 autocast (context)      min %8.4f ms   median %8.4f ms   launches %s   peak %8.1f MB" % (t16 + (l16, p16)))
        say("  eager fp32 / HIP (median)          %.2f x; peak memory eager - HIP %.1f MB (one map = %.1f MB)" % (te[1] / th[1], pe - ph, 4e-6 * N * C * H * W))
        if te[1] < th[1]:
            slower.append(shape)
            say("  NOTE: the HIP operator is SLOWER than the eager fp32 lines at this shape")
        hip()
        got = [x_cl.grad.clone()] + [p.grad.clone() for p in params]
        eager()
        ref = [x_nchw.grad] + [p.grad for p in params]
        say("  max |HIP - eager| / max |eager|    " + ", ".join("%s %.2g" % (n, R.rel_err(a, b)) for n, a, b in zip(R.RESULTS[1:], got, ref)))
    say()
    say("slower than eager fp32 at: %s" % (", ".join(str(s) for s in slower) or "no shape"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
