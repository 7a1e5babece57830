"""CondInst mask loss of the training loop (unicorn/models/condinst/dynamic_mask_head.py:247-278), forward and backward, fp32, at the headline
geometry 800 x 1280 (H8 x W8 = 100 x 160), up_rate 4, N = 16 / 64 / 128 foreground anchors: the fused HIP operator
(ops.condinst_dice_loss: uni_condinst_loss_fwd / _bwd) against the same lines in PyTorch eager on the same GPU in the same run, and
against the derived HBM floor.  HIP events around every call, warm-up first, min / median of the timed runs; peak memory of forward +
backward for both.

    python tools/condinst_loss_bench.py [--runs 20] [--out profiles/condinst_loss.txt]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unicorn_amd import ops  # noqa: E402

H8, W8, R = 100, 160, 4
HBM_BW = 6.3e12                   # achievable HBM bandwidth of the chip (float4 copy), bytes / s
SOI = (64.0, 128.0, 256.0, 512.0, 1024.0)


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


def eager_loss(mask_feats, up_masks, params, inst_loc, inst_lvl, gt, r):
    """What a PyTorch-ROCm user runs without the fused operator, with the operators the reference's training loop uses
    (dynamic_mask_head.py:138-170, :172-225, :247-278): the three dynamic layers as grouped 1x1 convolutions with one group per instance,
    an F.unfold of the logits, the broadcast product against the shared tap softmax, full-resolution logits, sigmoid and the dice sums."""
    n, (H, W), dev = params.shape[0], mask_feats.shape[2:], params.device
    cx = torch.arange(W, device=dev, dtype=torch.float32) * 8 + 4
    cy = torch.arange(H, device=dev, dtype=torch.float32) * 8 + 4
    size = torch.tensor(SOI, device=dev)[inst_lvl.long()]
    dx = ((inst_loc[:, 0, None, None] - cx[None, None, :]) / size[:, None, None]).expand(n, H, W)
    dy = ((inst_loc[:, 1, None, None] - cy[None, :, None]) / size[:, None, None]).expand(n, H, W)
    act = torch.cat([dx[:, None], dy[:, None], mask_feats.expand(n, 8, H, W)], dim=1).reshape(1, 10 * n, H, W)
    layers = ((params[:, :80], params[:, 152:160], 8), (params[:, 80:144], params[:, 160:168], 8), (params[:, 144:152], params[:, 168:169], 1))
    for k, (wgt, bias, cout) in enumerate(layers):
        act = F.conv2d(act, wgt.reshape(n * cout, -1, 1, 1), bias.reshape(n * cout), groups=n)
        act = F.relu(act) if k < 2 else act
    taps = F.unfold(act.reshape(n, 1, H, W), 3, padding=1).reshape(n, 9, 1, 1, H, W)
    weights = up_masks.reshape(1, 9, r, r, H, W).softmax(dim=1)
    fine = (weights * taps).sum(dim=1)                                       # (n, r, r, H, W): the (n, 9, r, r, H, W) product is formed first
    score = torch.sigmoid(fine.permute(0, 3, 1, 4, 2).reshape(n, r * H * r * W))
    target = gt.reshape(n, -1)
    return 1 - 2 * (score * target).sum(1) / (score.pow(2).sum(1) + target.pow(2).sum(1) + 1e-5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--instances", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("CondInst dice loss forward + backward, fp32, %d x %d feature map (800 x 1280), up_rate %d -- tools/condinst_loss_bench.py on %s"
        % (H8, W8, R, torch.cuda.get_device_name(0)))
    say("times: HIP events around every call, 3 warm-up calls, min / median of %d timed calls" % args.runs)
    for n in args.instances:
        g = torch.Generator().manual_seed(n)
        mf = torch.randn(1, 8, H8, W8, generator=g).cuda()
        um = torch.randn(1, 9 * R * R, H8, W8, generator=g).cuda()
        p = (0.35 * torch.randn(n, 169, generator=g)).cuda()
        loc = torch.stack([torch.randint(0, 8 * W8, (n,), generator=g), torch.randint(0, 8 * H8, (n,), generator=g)], dim=1).float().cuda()
        lvl = torch.randint(0, 5, (n,), generator=g).to(torch.int32).cuda()
        gt = torch.zeros(n, 1, R * H8, R * W8)
        for i in range(n):
            y0, x0 = int(torch.randint(0, R * H8 // 2, (1,), generator=g)), int(torch.randint(0, R * W8 // 2, (1,), generator=g))
            gt[i, 0, y0:y0 + 8 + int(torch.randint(0, R * H8 // 2, (1,), generator=g)), x0:x0 + 8 + int(torch.randint(0, R * W8 // 2, (1,), generator=g))] = 1
        gt = gt.cuda()
        go = torch.randn(n, generator=g).cuda()
        say()
        say("N = %d" % n)

        def leaves():
            return [t.detach().requires_grad_(True) for t in (mf, um, p)]

        def hip_fwd():
            with torch.no_grad():
                ops.condinst_dice_loss(mf, um, p, loc, lvl, gt, R)

        def hip_fb():
            a, b, c = leaves()
            ops.condinst_dice_loss(a, b, c, loc, lvl, gt, R).backward(go)
        a, b, c = leaves()
        out = ops.condinst_dice_loss(a, b, c, loc, lvl, gt, R)
        fwd = timed(hip_fwd, args.runs)
        bwd = timed(lambda: torch.autograd.grad(out, (a, b, c), go, retain_graph=True), args.runs)
        fb = timed(hip_fb, args.runs)
        hip_grads = torch.autograd.grad(out, (a, b, c), go)
        hip_loss = out.detach()
        del out, a, b, c
        hip_peak = peak_of(hip_fb)
        say("  HIP forward                          min %9.4f ms   median %9.4f ms" % fwd)
        say("  HIP backward (all three gradients)   min %9.4f ms   median %9.4f ms" % bwd)
        say("  HIP forward + backward               min %9.4f ms   median %9.4f ms" % fb)
        say("  HIP forward + backward peak memory   %9.1f MB (from NCHW maps, layout copies and gradients included)" % hip_peak)
        hw = H8 * W8
        gt_b, um_b, lg_b = n * hw * R * R * 4, hw * 9 * R * R * 4, n * hw * 4
        # forward: gt once, up_masks once per chunk of 8 instances is served by the caches after the first -> once, logits written + read
        f_fwd = (gt_b + um_b + 2 * lg_b) / HBM_BW * 1e3
        # backward: gt once, up_masks read + its gradient written, logits written + read, dL written + read twice
        f_bwd = (gt_b + 2 * um_b + 2 * lg_b + 3 * lg_b) / HBM_BW * 1e3
        say("  HBM floor at %.1f TB/s                forward %.4f ms (gt %.1f MB + up_masks %.1f MB + logits 2 x %.1f MB), backward %.4f ms"
            % (HBM_BW / 1e12, f_fwd, gt_b / 1e6, um_b / 1e6, lg_b / 1e6, f_bwd))
        say("  HIP (median) / floor                 forward %.1f x, backward %.1f x" % (fwd[1] / f_fwd, bwd[1] / f_bwd))
        try:
            def eager_fwd():
                with torch.no_grad():
                    eager_loss(mf, um, p, loc, lvl, gt, R)

            def eager_fb():
                a, b, c = leaves()
                eager_loss(a, b, c, loc, lvl, gt, R).backward(go)
            ef = timed(eager_fwd, args.runs)
            efb = timed(eager_fb, args.runs)
            a, b, c = leaves()
            o = eager_loss(a, b, c, loc, lvl, gt, R)
            eg = torch.autograd.grad(o, (a, b, c), go)
            errs = [float((x - y).abs().max() / y.abs().max()) for x, y in zip((hip_loss,) + tuple(hip_grads), (o.detach(),) + tuple(eg))]
            del o, a, b, c, eg
            eager_peak = peak_of(eager_fb)
            say("  eager forward (no_grad)              min %9.4f ms   median %9.4f ms" % ef)
            say("  eager forward + backward             min %9.4f ms   median %9.4f ms" % efb)
            say("  eager forward + backward peak memory %9.1f MB" % eager_peak)
            say("  eager / HIP (median)                 forward %.2f x, forward + backward %.2f x; memory %.1f x"
                % (ef[1] / fwd[1], efb[1] / fb[1], eager_peak / hip_peak))
            say("  max |HIP - eager| / max |eager|      loss %.3g, grad_mask_feats %.3g, grad_up_masks %.3g, grad_params %.3g" % tuple(errs))
        except torch.cuda.OutOfMemoryError as e:
            say("  eager PyTorch could not run this size on this (shared) card: out of memory (%s)" % str(e).split(".")[0])
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
