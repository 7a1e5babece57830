"""The head-output assembly of the training step (unicorn/models/unicorn_head_mask.py:339-366, get_output_and_grid :476-500, the level cats
:396-401 / :554-558) at the headline geometry 800 x 1280 (levels 100 x 160, 50 x 80, 25 x 40 with strides 8 / 16 / 32: 21000 anchors):
ops.head_assemble (uni_head_assemble_fwd, and uni_head_assemble_bwd in the backward) against the eager lines on the same GPU in the same run
-- tests/head_assemble_ref.py assemble, the per-level host-built tensors (torch.zeros(1, n).fill_(stride).type_as, torch.full, the grid)
included.  With fp16 maps ("as under autocast") the eager lines decode in fp16 and then widen outputs, origin_preds and dynamic_params with
.float(), because the loss operators take fp32; the operator reads the fp16 maps and writes fp32.

The timed quantity is forward + backward (the gradients of outputs, origin_preds and dynamic_params are handed to autograd.backward as
ready tensors, so that nothing but the assembly runs).  Per case, after warm-up, windows of --calls calls alternate between the two paths
(eager, HIP, eager, HIP, ...); reported is the median over the windows of
  call time    host clock around a window that ends in a device synchronise, per call
  device time  sum of the kernel durations of one call from torch.profiler (a run of its own, not the timed one), and the number of kernels
               launched in it; "not measured" where the profiler gives no device events
plus the host synchronisations of one call (torch.cuda.set_sync_debug_mode("warn")) and the peak memory of one call.

    python tools/head_assemble_bench.py [--windows 7] [--calls 20] [--out profiles/head_assemble.txt]
"""
import argparse
import os
import statistics
import sys
import time
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import head_assemble_ref as R  # noqa: E402
from unicorn_amd import ops  # noqa: E402

LEVELS = ((100, 160), (50, 80), (25, 40))
STRIDES = (8, 16, 32)
P = 169
CASES = [(B, C, ctrl, dt) for dt in (torch.float32, torch.float16) for ctrl in (True, False) for B in (2, 8) for C in (1, 8)]


def window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def alternating(fns, windows, calls, warm=3):
    for fn in fns:
        for _ in range(warm):
            fn()
    ts = [[] for _ in fns]
    for _ in range(windows):
        for k, fn in enumerate(fns):
            ts[k].append(window(fn, calls))
    return [statistics.median(t) for t in ts]


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def syncs_of(fn):
    """host synchronisations of one call, as torch reports them"""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("called a synchronizing" in str(w.message) for w in seen)


def device_of(fn):
    """(kernels launched, copies, sum of their durations in ms) of one call from torch.profiler, or None where it records no device event"""
    from torch.profiler import ProfilerActivity, profile
    try:
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
    except Exception as e:                                           # a measurement that cannot be taken is reported as such, never guessed
        return None, "%s: %s" % (type(e).__name__, e)
    if not ev:
        return None, "the profiler recorded no device event"
    copies = [e for e in ev if e.name.lower().startswith(("memcpy", "memset"))]       # what is no kernel: host-to-device copies among them
    dur = lambda e: getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0)      # noqa: E731
    return (len(ev) - len(copies), len(copies), sum(dur(e) for e in ev) / 1e3), ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    A = sum(h * w for h, w in LEVELS)
    say("Head-output assembly, %s, strides %s (%d anchors), P = %d -- tools/head_assemble_bench.py on %s"
        % (" ".join("%dx%d" % l for l in LEVELS), "/".join(map(str, STRIDES)), A, P, torch.cuda.get_device_name(0)))
    say("timed: forward + backward (gradients of outputs, origin_preds, dynamic_params given); 3 warm-up calls, then %d alternating windows of"
        % args.windows)
    say("%d calls per path; call time = host clock around a window ending in a synchronise, per call, median over the windows; device time and"
        % args.calls)
    say("launches from torch.profiler in a run of its own.  HIP = ops.head_assemble; eager = tests/head_assemble_ref.py assemble (the")
    say("reference's lines, host-built per-level tensors included; fp16 maps: fp16 decode, then .float() of the three results)")
    slower = []
    for B, C, with_ctrl, dt in CASES:
        g = torch.Generator().manual_seed(1)
        mk = lambda nc: [torch.randn(B, nc, h, w, generator=g).to("cuda", dt).requires_grad_(True) for h, w in LEVELS]      # noqa: E731
        reg, obj, cls = mk(4), mk(1), mk(C)
        ctrl = mk(P) if with_ctrl else None
        leaves = reg + obj + cls + (ctrl or [])
        grads = [torch.randn(B, A, 5 + C, device="cuda"), torch.randn(B, A, 4, device="cuda")] + ([torch.randn(B, A, P, device="cuda")] if with_ctrl else [])

        def finish(res):
            outs = [res[0], res[1]] + ([res[5]] if with_ctrl else [])
            torch.autograd.backward(outs, grads)

        def hip():
            for t in leaves:
                t.grad = None
            finish(ops.head_assemble(reg, obj, cls, STRIDES, ctrl))

        def eager():
            for t in leaves:
                t.grad = None
            res = R.assemble(reg, obj, cls, STRIDES, ctrl)
            if dt != torch.float32:
                res = tuple(t.float() if i in (0, 1, 5) and t is not None else t for i, t in enumerate(res))
            finish(res)
        name = "B = %d, C = %d, %s controller maps, %s maps" % (B, C, "with" if with_ctrl else "no", str(dt).replace("torch.", ""))
        say()
        say(name)
        te, th = alternating((eager, hip), args.windows, args.calls)
        for label, fn, t in (("HIP head_assemble + backward", hip, th), ("eager lines + backward", eager, te)):
            dev, why = device_of(fn)
            devs = "device %8.4f ms in %3d kernels + %d copies" % (dev[2], dev[0], dev[1]) if dev else "device not measured (%s)" % why
            say("  %-30s call %8.4f ms   %s   host syncs %d   peak %7.1f MB" % (label, t, devs, syncs_of(fn), peak_of(fn)))
        say("  eager / HIP (call time, median)  %.2f x" % (te / th))
        if te < th:
            say("  NOTE: the HIP operator is SLOWER than the eager lines in this case")
            slower.append(name)
        hip()
        gh = [t.grad.clone() for t in leaves]
        with torch.no_grad():
            rh, re_ = ops.head_assemble(reg, obj, cls, STRIDES, ctrl), R.assemble(reg, obj, cls, STRIDES, ctrl)
        eager()
        say("  max |HIP - eager| / max |eager|  outputs %.3g, gradients %.3g"
            % (R.rel_err(rh[0], re_[0]), max(R.rel_err(a, t.grad) for a, t in zip(gh, leaves))))
    say()
    say("cases in which the operator is slower by call time: %s" % ("; ".join(slower) if slower else "none"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
