"""The label-propagation parts of the SOT / VOS training losses (unicorn/models/unicorn.py:315-390), fp32, forward + backward at the headline
geometry 100 x 160 x 128 (an 800 x 1280 input at stride 8): ops.sot_prop_loss / ops.vos_prop_loss against what a user could do before they
existed, on the same GPU in the same run -- the reference's eager lines for the label maps (get_label_map with its .tolist() per sample,
F.interpolate of the full-resolution map), the pyramids (two F.interpolate) and the Dice, its Python match loop over device ids, and
ops.propagate_labels for the product, once per instance in the VOS branch as the reference does.  Both sides differentiate the same
scalar: corr_loss plus a fixed linear form of the three priors (the head's share of the gradient).  HIP events around every call, warm-up
first, min / median of the timed runs; peak memory of one call; kernel launches of one call counted by torch.profiler.

    python tools/prop_loss_bench.py [--runs 20] [--out profiles/prop_loss.txt]
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
import prop_loss_ref as R  # noqa: E402
from unicorn_amd import ops  # noqa: E402

C, H8, W8 = 128, 100, 160
H, W = 8 * H8, 8 * W8
CASES = (("sot", 1, 1), ("sot", 8, 1), ("vos", 2, 3), ("vos", 2, 8))          # branch, samples, matched instances per sample


def get_label_map(boxes, bs):
    """the reference's lines (:521-540), the device being the boxes' own"""
    x_c, y_c, w, h = boxes.unbind(-1)
    xyxy = torch.round(torch.stack([x_c - 0.5 * w, y_c - 0.5 * h, x_c + 0.5 * w, y_c + 0.5 * h], dim=-1)).int()
    labels = torch.zeros((bs, 1, H, W), dtype=torch.float32, device=boxes.device)
    for b in range(bs):
        x1, y1, x2, y2 = xyxy[b].tolist()
        labels[b, 0, max(0, y1):y2, max(0, x1):x2] = 1.0
    return labels


def down8(x):
    return F.interpolate(x, scale_factor=1 / 8, mode="bilinear", align_corners=False).flatten(-2)


def tail(pred, gt1):
    ms = (pred, F.interpolate(pred, scale_factor=1 / 2, mode="bilinear", align_corners=False),
          F.interpolate(pred, scale_factor=1 / 4, mode="bilinear", align_corners=False))
    return R.dice(pred.reshape(-1), gt1.reshape(-1)), ms


def eager_sot(e0, e1, t, w):
    bs = e0.shape[0]
    gt0 = down8(get_label_map(t[:, 0, 0, 1:5], bs))
    pred = ops.propagate_labels(e0, e1, gt0).view(bs, 1, H8, W8)
    loss, ms = tail(pred, down8(get_label_map(t[:, 1, 0, 1:5], bs)))
    return loss + sum((a * p).sum() for a, p in zip(w, ms))


def eager_vos(e0, e1, t, w):
    total, n = 0, 0
    for b in range(e0.shape[0]):
        id_r, id_c = t[b, 0, :, 5], t[b, 1, :, 5]
        s = 0
        for i, r in enumerate(id_r):
            j_hit = None
            if r != 0:                                                    # a device comparison per test, as in the reference
                for j, c in enumerate(id_c):
                    if (c != 0) and (c == r):
                        j_hit = j
                        break
            if j_hit is None:
                continue
            gt0 = down8(get_label_map(t[b:b + 1, 0, i, 1:5], 1))
            gt1 = down8(get_label_map(t[b:b + 1, 1, j_hit, 1:5], 1))
            pred = ops.propagate_labels(e0[b:b + 1], e1[b:b + 1], gt0).view(1, 1, H8, W8)
            loss, ms = tail(pred, gt1)
            total = total + loss + sum((a[b:b + 1, s:s + 1] * p).sum() for a, p in zip(w, ms))
            n, s = n + 1, s + 1
    return total / max(n, 1)


def hip_sot(e0, e1, t, w):
    loss, ms = ops.sot_prop_loss(e0, e1, t, (H, W))
    return loss + sum((a * p).sum() for a, p in zip(w, ms))


def hip_vos(e0, e1, t, w):
    loss, ms, _, num = ops.vos_prop_loss(e0, e1, t, (H, W))
    return (loss.sum() + sum((a * p).sum() for a, p in zip(w, ms))) / num.sum().clamp(min=1)


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

    say("SOT / VOS label-propagation losses, fp32, forward + backward, maps %d x %d x %d -- tools/prop_loss_bench.py on %s"
        % (H8, W8, C, torch.cuda.get_device_name(0)))
    say("times: HIP events around every call (backward() included), 3 warm-up calls, min / median of %d timed calls" % args.runs)
    say("eager: the reference's label-map, pyramid, Dice and match-loop lines around ops.propagate_labels (once per instance for VOS)")
    for kind, B, K in CASES:
        g = torch.Generator().manual_seed(31 * B + K)
        e0, e1 = (0.25 * torch.randn(B, C, H8, W8, generator=g)).cuda(), (0.25 * torch.randn(B, C, H8, W8, generator=g)).cuda()
        M = max(K, 2)
        t = torch.zeros(B, 2, M, 6)
        t[..., 1:5] = R._box_rows(g, B * 2 * M, H, W).view(B, 2, M, 4)
        t[:, 0, :K, 5] = torch.arange(1, K + 1).float()
        t[:, 1, :K, 5] = torch.arange(K, 0, -1).float()
        t = t.cuda()
        Kc = 1 if kind == "sot" else M
        w = [torch.randn(B, Kc, H8 // s, W8 // s, generator=g).cuda() for s in (1, 2, 4)]
        hip_fn, eager_fn = (hip_sot, eager_sot) if kind == "sot" else (hip_vos, eager_vos)
        say()
        say("%s, B = %d samples%s" % (kind.upper(), B, "" if kind == "sot" else ", %d matched instances per sample" % K))

        def both(fn):
            a, b = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
            total = fn(a, b, t, w)
            total.backward()
            return total.detach(), a.grad, b.grad
        hip, eag = timed(lambda: both(hip_fn), args.runs), timed(lambda: both(eager_fn), args.runs)
        hip_peak, eag_peak = peak_of(lambda: both(hip_fn)), peak_of(lambda: both(eager_fn))
        hip_n, eag_n = launches_of(lambda: both(hip_fn)), launches_of(lambda: both(eager_fn))
        say("  HIP operator    min %9.4f ms   median %9.4f ms   peak %8.1f MB   kernel launches %s" % (hip + (hip_peak, hip_n or "not measured")))
        say("  eager lines     min %9.4f ms   median %9.4f ms   peak %8.1f MB   kernel launches %s" % (eag + (eag_peak, eag_n or "not measured")))
        say("  eager / HIP (median) %.2f x; memory %.2f x" % (eag[1] / hip[1], eag_peak / max(hip_peak, 1e-9)))
        if eag[1] < hip[1]:
            say("  NOTE: the HIP operator is SLOWER than the eager lines in this case")
        got, ref = both(hip_fn), both(eager_fn)
        say("  max |HIP - eager| / max |eager|  total %.2e  grad_embed_0 %.2e  grad_embed_1 %.2e"
            % tuple(float((a - r).abs().max() / r.abs().max()) for a, r in zip(got, ref)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
