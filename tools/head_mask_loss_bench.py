"""CondInst mask loss of get_losses (unicorn/models/unicorn_head_mask.py:675-694, :731-732) for a batch, forward + backward, fp32, at
800 x 1280 (H8 x W8 = 100 x 160, A = 21000 anchors), up_rate 4: the batched operator (ops.head_mask_loss: uni_head_mask_loss_fwd / _bwd)
against the path it replaces -- the per-image loop of those lines with ops.condinst_dice_loss on rows compacted by boolean index, each
image's `torch.sum(fg_mask) > 0` included -- on the same GPU in the same run.  Every configuration is run with the default capacity
B * min(A, 10 M) and with capacity = the instance count, so that the cost of empty slots is measured.  HIP events around every call,
warm-up first, min / median of the timed runs; host synchronisations counted with torch's sync debug mode; peak memory of forward +
backward for both.

    python tools/head_mask_loss_bench.py [--runs 20] [--out profiles/head_mask_loss.txt]
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
from unicorn_amd import ops  # noqa: E402
import simota_ref as S  # noqa: E402

H8, W8, R = 100, 160, 4
# (name, B, boxes per image M, anchors per box): SimOTA gives a box up to 10 anchors
CONFIGS = (("B 1, ~10 instances (SOT / VOS: one box)", 1, 1, 10), ("B 1, 128 instances (16 boxes x 8)", 1, 16, 8),
           ("B 8, 100 instances each (100 boxes x 1)", 8, 100, 1))


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
    return min(ts), statistics.median(ts), max(ts)


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def syncs_of(fn):
    """host synchronisations torch reports for one call (sync debug mode "warn": one warning each)"""
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return sum("synchroniz" in str(x.message).lower() for x in w)


def problem(B, M, per_box, seed):
    g = torch.Generator().manual_seed(seed)
    xs, ys, st = S.anchors(8 * H8, 8 * W8, "cuda")
    A = xs.shape[0]
    mf, um = torch.randn(B, 8, H8, W8, generator=g).cuda(), torch.randn(B, 9 * R * R, H8, W8, generator=g).cuda()
    dp = (0.35 * torch.randn(B, A, 169, generator=g)).cuda()
    lvl = torch.randint(0, 5, (B, A), generator=g).to(torch.int32).cuda()
    masks = torch.zeros(B, M, R * H8, R * W8)
    fg, matched = torch.zeros(B, A, dtype=torch.bool), torch.full((B, A), -1, dtype=torch.int64)
    for b in range(B):
        rows = torch.randperm(A, generator=g)[:M * per_box]
        fg[b, rows] = True
        matched[b, rows] = torch.arange(M).repeat_interleave(per_box)
        for m in range(M):
            y0, x0 = int(torch.randint(0, R * H8 // 2, (1,), generator=g)), int(torch.randint(0, R * W8 // 2, (1,), generator=g))
            masks[b, m, y0:y0 + 8 + int(torch.randint(0, R * H8 // 2, (1,), generator=g)),
                  x0:x0 + 8 + int(torch.randint(0, R * W8 // 2, (1,), generator=g))] = 1
    fg, matched = fg.cuda(), matched.cuda()
    return mf, um, dp, lvl, masks.cuda(), (fg, matched, torch.zeros(B, A, device="cuda"), fg.sum(dim=1)), xs, ys, st


def loop_loss(mf, um, dp, lvl, masks, assignment, xs, ys, st):
    """the parent path: :675-694 and :731-732 per image with the fused per-image operator on compacted rows"""
    fg, matched = assignment[0], assignment[1]
    loss_masks, num_valid = [], 0
    for b in range(mf.shape[0]):
        m = fg[b]
        if torch.sum(m) > 0:
            loc = torch.stack([st[m] * (xs[m] + 0.5), st[m] * (ys[m] + 0.5)], dim=1)
            gt = masks[b][matched[b, m]].unsqueeze(1)
            loss_masks.append(ops.condinst_dice_loss(mf[b:b + 1], um[b:b + 1], dp[b, m], loc, lvl[b, m], gt, R).mean())
            num_valid += 1
        else:
            loss_masks.append(torch.sum(mf[b:b + 1]) * 0.0 + torch.sum(dp[b]) * 0.0)
    return torch.sum(torch.stack(loss_masks)) / max(num_valid, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--configs", type=int, nargs="+", default=list(range(len(CONFIGS))))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("CondInst mask loss of a batch, forward + backward, fp32, %d x %d feature map (800 x 1280), up_rate %d -- tools/head_mask_loss_bench.py on %s"
        % (H8, W8, R, torch.cuda.get_device_name(0)))
    say("times: HIP events around every call, 3 warm-up calls, min / median / max of %d timed calls; both operands in this run on this GPU" % args.runs)
    say("operator launches: 5 forward + 22 backward of its own whatever the data (plus torch's layout copies); the loop's grow with B and N")
    for k in args.configs:
        name, B, M, per_box = CONFIGS[k]
        mf, um, dp, lvl, masks, asg, xs, ys, st = problem(B, M, per_box, 7 + k)
        n = int(asg[0].sum())
        A = dp.shape[1]
        say()
        say("%s: %d instances, M = %d" % (name, n, M))

        def leaves():
            return [t.detach().requires_grad_(True) for t in (mf, um, dp)]

        def op_fb(cap):
            a, b, c = leaves()
            loss, _ = ops.head_mask_loss(a, b, c, lvl, masks, asg, xs, ys, st, R, capacity=cap)
            loss.backward()
            return loss.detach(), a.grad, b.grad, c.grad

        def loop_fb():
            a, b, c = leaves()
            loss = loop_loss(a, b, c, lvl, masks, asg, xs, ys, st)
            loss.backward()
            return loss.detach(), a.grad, b.grad, (torch.zeros_like(c) if c.grad is None else c.grad)
        ref = loop_fb()
        for label, cap in (("default capacity %d" % (B * min(A, 10 * M)), None), ("capacity = count %d" % n, n)):
            t = timed(lambda: op_fb(cap), args.runs)
            ws = ops.L.lib().uni_head_mask_loss_workspace_bytes(B, A, H8, W8, R, cap or B * min(A, 10 * M))
            say("  operator, %-24s min %9.4f ms   median %9.4f ms   max %9.4f ms   host syncs %d   peak memory %8.1f MB (workspace %.1f MB)"
                % (label, t[0], t[1], t[2], syncs_of(lambda: op_fb(cap)), peak_of(lambda: op_fb(cap)), ws / 1e6))
            got = op_fb(cap)
            errs = [float((x - y).abs().max() / y.abs().max().clamp(min=1e-30)) for x, y in zip(got, ref)]
            say("    max |operator - loop| / max |loop|   loss %.3g, grad_mask_feats %.3g, grad_up_masks %.3g, grad_dynamic_params %.3g" % tuple(errs))
        t = timed(loop_fb, args.runs)
        say("  per-image loop (parent path)        min %9.4f ms   median %9.4f ms   max %9.4f ms   host syncs %d   peak memory %8.1f MB"
            % (t[0], t[1], t[2], syncs_of(loop_fb), peak_of(loop_fb)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
