"""The detection losses of the training step (unicorn/models/unicorn_head_mask.py:571-745 without the CondInst lines), fp32, at the headline
geometry 800 x 1280 (21000 anchors): ops.head_det_loss (uni_simota_assign + uni_head_loss_fwd, and uni_head_loss_bwd in the backward)
against the eager lines on the same GPU in the same run -- ops.simota_assign_batch feeding tests/head_loss_ref.py det_losses, boolean
indexing included.  The timed quantity is forward + backward of assignment + losses.  HIP events around every call, warm-up first, min /
median of the timed runs; peak memory of one call; the number of host synchronisations of one call, counted with
torch.cuda.set_sync_debug_mode("warn").

    python tools/head_loss_bench.py [--runs 20] [--out profiles/head_loss.txt]
"""
import argparse
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import head_loss_ref as R  # noqa: E402
import simota_ref as S  # noqa: E402
from unicorn_amd import ops  # noqa: E402

H, W = 800, 1280
CASES = ((1, 100, 1), (8, 100, 1), (1, 100, 80), (8, 100, 80))          # images, boxes per image, classes


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
    return sum("called a synchronizing" in str(w.message) for w in seen)      # not the one-time notice that the mode is a prototype


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    xs, ys, st = S.anchors(H, W, "cuda")
    A = xs.shape[0]
    say("Detection-head losses, fp32, %d x %d (%d anchors) -- tools/head_loss_bench.py on %s" % (H, W, A, torch.cuda.get_device_name(0)))
    say("timed: forward + backward of SimOTA assignment + the four losses (gradients of outputs and origin_preds); HIP events around every")
    say("call, 3 warm-up calls, min / median of %d timed calls.  HIP = ops.head_det_loss; eager = ops.simota_assign_batch feeding" % args.runs)
    say("tests/head_loss_ref.py det_losses (the reference's lines vectorised over the batch, boolean indexing included)")
    for B, G, C in CASES:
        imgs = [[t.cuda() for t in S.draw(H, W, G, C, 10 * G + b, "mot")] for b in range(B)]
        outputs = torch.stack([torch.cat(i[:3], 1) for i in imgs]).contiguous().requires_grad_(True)
        labels = torch.stack([torch.cat([i[4][:, None], i[3]], 1) for i in imgs]).contiguous()
        origin = torch.randn(B, A, 4, device="cuda").requires_grad_(True)
        say()
        say("B = %d images, G = %d boxes each, C = %d classes" % (B, G, C))

        given = ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)

        def hip(assignment=None):
            outputs.grad = origin.grad = None
            losses, _ = ops.head_det_loss(outputs, origin, labels, xs, ys, st, (H, W), C, assignment=assignment)
            losses["total_loss"].backward()
            return losses

        def eager(assignment=None):
            outputs.grad = origin.grad = None
            fg, matched, iou, _ = assignment or ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)
            losses = R.det_losses(outputs, origin, labels, fg, matched, iou, xs, ys, st)
            losses["total_loss"].backward()
            return losses
        th, te = timed(hip, args.runs), timed(eager, args.runs)
        ph, pe = peak_of(hip), peak_of(eager)
        sh, se = syncs_of(hip), syncs_of(eager)
        say("  HIP head_det_loss + backward              min %9.4f ms   median %9.4f ms   peak %8.1f MB   host syncs %d" % (th + (ph, sh)))
        say("  eager assignment + det_losses + backward  min %9.4f ms   median %9.4f ms   peak %8.1f MB   host syncs %d" % (te + (pe, se)))
        say("  eager / HIP (median)                      %.2f x; memory %.2f x" % (te[1] / th[1], pe / max(ph, 1e-9)))
        if te[1] < th[1]:
            say("  NOTE: the HIP operator is SLOWER than the eager lines in this case")
        # the same with the assignment handed in: the losses alone (the assignment's workspace dominates the peaks above)
        th, te = timed(lambda: hip(given), args.runs), timed(lambda: eager(given), args.runs)
        ph, pe = peak_of(lambda: hip(given)), peak_of(lambda: eager(given))
        sh, se = syncs_of(lambda: hip(given)), syncs_of(lambda: eager(given))
        say("  losses alone (assignment given): HIP      min %9.4f ms   median %9.4f ms   peak %8.1f MB   host syncs %d" % (th + (ph, sh)))
        say("  losses alone (assignment given): eager    min %9.4f ms   median %9.4f ms   peak %8.1f MB   host syncs %d" % (te + (pe, se)))
        say("  eager / HIP (median)                      %.2f x; memory %.2f x" % (te[1] / th[1], pe / max(ph, 1e-9)))
        if te[1] < th[1]:
            say("  NOTE: the HIP operator is SLOWER than the eager lines in this case")
        lh = hip()
        gh = (outputs.grad.clone(), origin.grad.clone())
        le = eager()
        say("  max |HIP - eager| / max |eager|           losses %.3g, grad_outputs %.3g, grad_origin %.3g"
            % (max(R.rel_err(lh[k], le[k]) for k in R.QUANTITIES[:4]), R.rel_err(gh[0], outputs.grad), R.rel_err(gh[1], origin.grad)))
    say()
    say("not measured here: the reference's own per-image Python loop (:571-673; its 3 B further read-backs come on top of the eager lines")
    say("above, which are already vectorised over the batch), fp64.")
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
