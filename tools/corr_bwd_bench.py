"""Label propagation of the training losses (unicorn/models/unicorn.py:321-326), forward-with-lse and backward, fp32, at the headline
geometry R = Q = 16000 (800 x 1280 at stride 8), D = 128, K = 1, B = 1 and B = 4: the HIP operator (uni_corr_softmax_pv_lse /
uni_corr_softmax_pv_bwd, precision 0) against the same three lines in PyTorch eager on the same GPU in the same run, and against the
derived floor of the MFMA products.  HIP events around every call, warm-up first, median of the timed runs; peak memory of forward +
backward for both.

    python tools/corr_bwd_bench.py [--runs 20] [--out profiles/corr_backward.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unicorn_amd import ops  # noqa: E402

R = Q = 16000
D = 128
K = 1
F32_MFMA_PEAK = 155e12            # v_mfma_f32_32x32x2_f32, dense peak of the chip (flop / s)


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
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def three_lines(e0, e1, lb):
    return lb @ torch.softmax(e0.transpose(1, 2) @ e1, dim=1)          # e0 (B, C, HW_0), e1 (B, C, HW_1), lb (B, K, HW_0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("label propagation forward (with lse) + backward, fp32 precision 0, R = Q = %d, D = %d, K = %d -- tools/corr_bwd_bench.py on %s"
        % (R, D, K, torch.cuda.get_device_name(0)))
    say("times: HIP events around every call, 3 warm-up calls, min / median of %d timed calls" % args.runs)
    for B in args.batches:
        g = torch.Generator().manual_seed(B)
        e0 = (0.3 * torch.randn(B, D, R, generator=g)).cuda()
        e1 = (0.3 * torch.randn(B, D, Q, generator=g)).cuda()
        lb = torch.rand(B, K, R, generator=g).cuda()
        go = torch.randn(B, K, Q, generator=g).cuda()
        er, ec = e0.transpose(1, 2).contiguous(), e1.transpose(1, 2).contiguous()
        say()
        say("B = %d" % B)
        out, lse = ops.corr_softmax_pv_lse(er, ec, lb)
        fwd = timed(lambda: ops.corr_softmax_pv_lse(er, ec, lb), args.runs)
        bwd = timed(lambda: ops.corr_softmax_pv_backward(er, ec, lb, out, lse, go), args.runs)
        bwd_e = timed(lambda: ops.corr_softmax_pv_backward(er, ec, lb, out, lse, go, need=(True, True, False)), args.runs)
        bwd_c = timed(lambda: ops.corr_softmax_pv_backward(er, ec, lb, out, lse, go, need=(False, True, False)), args.runs)

        def hip_fb():
            a, b, c = (t.detach().requires_grad_(True) for t in (e0, e1, lb))
            ops.propagate_labels(a, b, c).backward(go)
        hip_peak = peak_of(hip_fb)
        say("  HIP forward with lse                 min %9.4f ms   median %9.4f ms" % fwd)
        say("  HIP backward (all three gradients)   min %9.4f ms   median %9.4f ms" % bwd)
        say("  HIP backward (both embeddings)       min %9.4f ms   median %9.4f ms" % bwd_e)
        say("  HIP backward (embed_1 only, 1 pass)  min %9.4f ms   median %9.4f ms" % bwd_c)
        say("  HIP forward + backward peak memory   %9.1f MB (propagate_labels from (B, C, HW) maps, row-major copies included)" % hip_peak)
        flop3, flop4 = 3 * 2.0 * R * Q * D * B, 4 * 2.0 * R * Q * D * B
        say("  floor, 3 products at %.0f TF           %9.4f ms   (3 x 2 R Q D = %.3g flop)" % (F32_MFMA_PEAK / 1e12, flop3 / F32_MFMA_PEAK * 1e3, flop3))
        say("  floor, 4 products (two passes)       %9.4f ms   -> HIP backward (median) = %.2f x this floor; no atomics are used"
            % (flop4 / F32_MFMA_PEAK * 1e3, bwd[1] / (flop4 / F32_MFMA_PEAK * 1e3)))
        # the same three lines in eager PyTorch on this GPU (2 GB of matrices per frame for autograd, as much again in the backward)
        try:
            def eager_fwd():
                with torch.no_grad():
                    three_lines(e0, e1, lb)

            def eager_fb():
                a, b, c = (t.detach().requires_grad_(True) for t in (e0, e1, lb))
                three_lines(a, b, c).backward(go)
            ef = timed(eager_fwd, args.runs)
            efb = timed(eager_fb, args.runs)
            a, b, c = (t.detach().requires_grad_(True) for t in (e0, e1, lb))
            o = three_lines(a, b, c)
            eb = timed(lambda: torch.autograd.grad(o, (a, b, c), go, retain_graph=True), args.runs)
            errs = [float((x - y).abs().max() / y.abs().max()) for x, y in
                    zip(ops.corr_softmax_pv_backward(er, ec, lb, out, lse, go)[:2], [t.transpose(1, 2) for t in torch.autograd.grad(o, (a, b), go)])]
            del o, a, b, c
            eager_peak = peak_of(eager_fb)
            say("  eager forward (no_grad)              min %9.4f ms   median %9.4f ms" % ef)
            say("  eager backward                       min %9.4f ms   median %9.4f ms" % eb)
            say("  eager forward + backward             min %9.4f ms   median %9.4f ms" % efb)
            say("  eager forward + backward peak memory %9.1f MB" % eager_peak)
            say("  eager / HIP (median)                 forward %.2f x, backward %.2f x, forward + backward %.2f x; memory %.0f x"
                % (ef[1] / fwd[1], eb[1] / bwd[1], efb[1] / (fwd[1] + bwd[1]), eager_peak / hip_peak))
            say("  max |HIP - eager| / max |eager|      grad_embed_0 %.3g, grad_embed_1 %.3g" % tuple(errs))
        except torch.cuda.OutOfMemoryError as e:
            say("  eager PyTorch could not run this batch on this (shared) card: out of memory (%s)" % str(e).split(".")[0])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
