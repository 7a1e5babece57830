"""The MOT instance-contrastive loss of the training loop (unicorn/models/unicorn.py:407-466), fp32, forward + backward at the headline
geometry 100 x 160 x 128 (an 800 x 1280 input at stride 8) with max_labels = 100 target rows: the fused HIP operator (ops.mot_corr_loss:
uni_mot_corr_loss_fwd / _bwd) against the same lines in PyTorch eager on the same GPU in the same run -- the two restatements of
tests/mot_corr_ref.py: the reference-shaped loop (a Python loop over the id pairs, one grid_sample per instance; the reference compares
device tensors in that loop and so reads back once per pair, the restatement reads the ids once, which flatters it) and the vectorised
form.  HIP events around every call, warm-up first, min / median of the timed runs; peak memory of one call; the largest deviation of the
losses and gradients from the vectorised form.

    python tools/mot_corr_bench.py [--runs 20] [--out profiles/mot_corr_loss.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mot_corr_ref as R  # noqa: E402
from unicorn_amd import ops  # noqa: E402

C, H, W, M = 128, 100, 160, 100
CASES = ((1, 10), (1, 100), (8, 100))          # samples, instances per frame (up to)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("MOT instance-contrastive loss, fp32, forward + backward, maps %d x %d x %d, %d target rows -- tools/mot_corr_bench.py on %s"
        % (H, W, C, M, torch.cuda.get_device_name(0)))
    say("times: HIP events around every call (loss.mean().backward() included), 3 warm-up calls, min / median of %d timed calls" % args.runs)
    say("eager: tests/mot_corr_ref.py, loss_loop (the reference's shape; ids read once instead of once per pair) and loss_vectorised")
    for B, n in CASES:
        e0, e1, t, _ = R.draw("large", 7 * n + B, (B, C, H, W, n))
        targets = torch.zeros(B, 2, M, 6)
        targets[:, :, :n] = t
        e0, e1, targets = e0.cuda(), e1.cuda(), targets.cuda()
        counts = (targets[..., 5] != 0).sum(-1).tolist()
        say()
        say("B = %d samples, instances per frame %s" % (B, counts if B == 1 else "%d .. %d" % (min(map(min, counts)), max(map(max, counts)))))

        def both(fn):
            a, b = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
            loss = fn(a, b, targets)
            loss.mean().backward()
            return loss.detach(), a.grad, b.grad

        def forward(fn):
            with torch.no_grad():
                return fn(e0, e1, targets)
        hip = timed(lambda: both(ops.mot_corr_loss), args.runs)
        hip_f = timed(lambda: forward(ops.mot_corr_loss), args.runs)
        say("  HIP mot_corr_loss forward + backward     min %9.4f ms   median %9.4f ms" % hip)
        say("  HIP mot_corr_loss forward only           min %9.4f ms   median %9.4f ms" % hip_f)
        hip_peak = peak_of(lambda: both(ops.mot_corr_loss))
        say("  HIP peak memory, forward + backward      %9.1f MB (two map clones and two gradient maps: %.1f MB)" % (hip_peak, 4 * e0.numel() * 4 / 1e6))
        vec, loop = timed(lambda: both(R.loss_vectorised), args.runs), timed(lambda: both(R.loss_loop), args.runs)
        vec_peak = peak_of(lambda: both(R.loss_vectorised))
        say("  eager, vectorised form                   min %9.4f ms   median %9.4f ms" % vec)
        say("  eager, per-instance loop (the reference) min %9.4f ms   median %9.4f ms" % loop)
        say("  eager peak memory (vectorised form)      %9.1f MB" % vec_peak)
        say("  eager / HIP (median)                     vectorised %.2f x, loop %.2f x; memory %.2f x" % (vec[1] / hip[1], loop[1] / hip[1], vec_peak / max(hip_peak, 1e-9)))
        if min(vec[1], loop[1]) < hip[1]:
            say("  NOTE: the HIP operator is SLOWER than eager PyTorch in this case")
        got, ref = both(ops.mot_corr_loss), both(R.loss_vectorised)
        say("  max |HIP - vectorised| / max |vectorised|  loss %.2e  grad_embed_0 %.2e  grad_embed_1 %.2e"
            % tuple(float((g - r).abs().max() / r.abs().max()) for g, r in zip(got, ref)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
