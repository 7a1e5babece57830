"""SimOTA label assignment of the training loop (unicorn/models/unicorn_head_mask.py:571-645 with :754-983), fp32, at the headline geometry
800 x 1280 (21000 anchors): the fused HIP operator (ops.simota_assign_batch / simota_assign: uni_simota_assign) against the same lines in
PyTorch eager on the same GPU in the same run -- the restatement of tests/simota_ref.py, once with the reference's per-box topk loop and
its host read-backs (what the reference runs) and once with the loop replaced by a sort.  HIP events around every call, warm-up first,
min / median of the timed runs; peak memory of one call; the number of anchors whose foreground decision differs.

    python tools/simota_bench.py [--runs 20] [--out profiles/simota_assign.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import simota_ref as R  # noqa: E402
from unicorn_amd import ops  # noqa: E402

H, W = 800, 1280
CASES = ((1, 1, 1), (1, 100, 1), (1, 50, 80), (8, 100, 1))          # images, boxes per image, classes


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

    xs, ys, st = R.anchors(H, W, "cuda")
    A = xs.shape[0]
    say("SimOTA label assignment, fp32, %d x %d (%d anchors) -- tools/simota_bench.py on %s" % (H, W, A, torch.cuda.get_device_name(0)))
    say("times: HIP events around every call, 3 warm-up calls, min / median of %d timed calls; every timed call ends with the read of num_fg"
        % args.runs)
    say("eager: tests/simota_ref.py assign() per image in a Python loop over the batch, as get_losses does (top-10 IoUs by topk, no diagnostics)")
    for B, G, C in CASES:
        imgs = [[t.cuda() for t in R.draw(H, W, G, C, 10 * G + b, "mot")] for b in range(B)]
        outputs = torch.stack([torch.cat(i[:3], 1) for i in imgs]).contiguous()
        labels = torch.stack([torch.cat([i[4][:, None], i[3]], 1) for i in imgs]).contiguous()
        say()
        say("B = %d images, G = %d boxes each, C = %d classes" % (B, G, C))

        def hip_batch():
            return ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)

        def hip_batch_read():
            return hip_batch()[3].tolist()

        def hip_per_image():
            return [ops.simota_assign(*i, xs, ys, st, (H, W), C) for i in imgs]

        def eager(loop):
            return [R.assign(*i, xs, ys, st, (H, W), C, loop=loop) for i in imgs]
        hb, hp = timed(hip_batch_read, args.runs), timed(hip_per_image, args.runs)
        say("  HIP simota_assign_batch + num_fg read     min %9.4f ms   median %9.4f ms" % hb)
        say("  HIP simota_assign per image (%d calls)     min %9.4f ms   median %9.4f ms" % ((B,) + hp))
        hip_peak = peak_of(hip_batch)
        say("  HIP peak memory of the batched call      %9.1f MB (workspace %.1f MB; one (G, A, C) fp32 tensor per image would be %.1f MB)"
            % (hip_peak, _ws(B, A, G, C) / 1e6, G * A * C * 4 / 1e6))
        try:
            el, es = timed(lambda: eager(True), args.runs), timed(lambda: eager(False), args.runs)
            eager_peak = peak_of(lambda: eager(True))
            say("  eager, per-box topk loop (the reference) min %9.4f ms   median %9.4f ms" % el)
            say("  eager, loop replaced by one sort         min %9.4f ms   median %9.4f ms" % es)
            say("  eager peak memory (one image at a time)  %9.1f MB" % eager_peak)
            say("  eager / HIP (median)                     loop %.2f x, sort %.2f x (batched call); loop %.2f x (per-image calls); memory %.1f x"
                % (el[1] / hb[1], es[1] / hb[1], el[1] / hp[1], eager_peak / max(hip_peak, 1e-9)))
            if min(el[1], es[1]) < hb[1]:
                say("  NOTE: the HIP operator is SLOWER than eager PyTorch in this case")
            fg = hip_batch()[0]
            ref = eager(False)
            diff = sum(int((fg[b] != ref[b]["fg_mask"]).sum()) for b in range(B))
            say("  fg decisions that differ from eager      %d of %d anchors (matched anchors: %d)" % (diff, B * A, int(fg.sum())))
        except torch.cuda.OutOfMemoryError as e:
            say("  eager PyTorch could not run this size on this (shared) card: out of memory (%s)" % str(e).split(".")[0])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def _ws(B, A, G, C):
    from unicorn_amd import _lib
    return _lib.lib().uni_simota_workspace_bytes(B, A, G, C)


if __name__ == "__main__":
    main()
