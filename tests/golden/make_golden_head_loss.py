"""Golden vectors for the fused detection-head loss (uni_head_loss_fwd / _bwd, ops.HeadLossFunction / head_det_loss), produced by EXECUTING
the reference's own UnicornHeadMask.get_losses (unicorn/models/unicorn_head_mask.py:521-745) on the CPU, once in fp64 and once in fp32,
with its backward.  The head is made with __new__: get_losses reads only mode, num_classes, num_classes_sot, use_l1 and the three loss
modules.  masks = up_masks = None and zero mask_feats / dynamic_params make loss_condinst an exact 0.  The assignment the reference reached
is recorded by wrapping get_assignments.  No reference text is stored.

Inputs: the outputs / labels of the simota_*.npz fixtures (only read), origin_preds drawn from a recorded seed, grad_out = four unequal
weights.  Every file holds the five results and both gradients of the fp64 run, the same of the fp32 run, and per quantity
<name>_fp32_ref_err = max |fp32 - fp64| / max |fp64| (0 where the quantity is exactly zero in both).

Asserted per case (origin_preds is redrawn with the next seed on a failure of the L1 rule; anything else fails; nothing is filtered):
the fp32 and the fp64 run reach the same fg_mask / matched_gt_inds; no foreground anchor has a predicted edge within 1e-6 px of the
ground-truth edge it is compared with, an L1 residual below 1e-6, or br - tl within 1e-6 of zero.

    python tests/golden/make_golden_head_loss.py        -> tests/golden/head_loss_<case>.npz
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import head_loss_ref as R  # noqa: E402
import simota_ref as S  # noqa: E402

KINK = 1e-6


def reference_losses(mode, C, use_l1, outputs, origin, labels, xs, ys, st, img_size, grad_out, dtype):
    """the reference's get_losses + backward on the CPU in `dtype` -> the seven quantities and the assignment it reached"""
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.losses import IOUloss
    from unicorn.models.unicorn_head_mask import UnicornHeadMask
    head = UnicornHeadMask.__new__(UnicornHeadMask)
    nn.Module.__init__(head)
    head.mode, head.num_classes, head.num_classes_sot, head.use_l1 = mode, C, C, use_l1
    head.iou_loss = IOUloss(reduction="none")
    head.bcewithlog_loss = nn.BCEWithLogitsLoss(reduction="none")
    head.l1_loss = nn.L1Loss(reduction="none")
    B, A = outputs.shape[:2]
    seen = {}
    inner = head.get_assignments

    def recording(batch_idx, *rest, **kw):
        got = inner(batch_idx, *rest, **kw)
        seen[batch_idx] = tuple(t.clone() if isinstance(t, torch.Tensor) else t for t in got)
        return got
    head.get_assignments = recording
    o = outputs.to(dtype).clone().requires_grad_(True)
    g = origin.to(dtype).clone().requires_grad_(True)
    imgs = torch.zeros(B, 3, img_size[0], img_size[1], dtype=dtype)
    res = head.get_losses(imgs, [xs.to(dtype)[None]], [ys.to(dtype)[None]], [st.to(dtype)[None]], labels.to(dtype), o, [g], dtype,
                          torch.zeros(B, 8, 1, 1, dtype=dtype), torch.zeros(B, A, 1, dtype=dtype), None, None, None)
    _, l_iou, l_obj, l_cls, l_l1, l_mask, ratio = res
    assert float(l_mask) == 0.0
    four = (l_iou, l_obj, l_cls, l_l1)
    sum(w * t for w, t in zip(grad_out, four) if isinstance(t, torch.Tensor)).backward()
    fg = torch.zeros(B, A, dtype=torch.bool)
    matched = torch.full((B, A), -1, dtype=torch.int64)
    iou = torch.zeros(B, A, dtype=dtype)
    num_fg = torch.zeros(B, dtype=torch.int64)
    for b, (_, m, ious, inds, n) in seen.items():
        fg[b], num_fg[b] = m, int(n)
        matched[b][m], iou[b][m] = inds, ious.to(dtype)
    out = {k: torch.as_tensor(float(t.detach() if isinstance(t, torch.Tensor) else t), dtype=dtype) for k, t in zip(R.QUANTITIES[:4], four)}
    out["num_fg"] = torch.as_tensor(float(ratio), dtype=dtype)
    out["grad_outputs"] = o.grad
    out["grad_origin"] = g.grad if use_l1 else None
    return out, (fg, matched, iou, num_fg)


def kinks(outputs, origin, labels, fg, matched, xs, ys, st):
    """the smallest distance of a foreground anchor from a kink, in fp64: (edge tie, |br - tl|, L1 residual)"""
    if not bool(fg.any()):
        return float("inf"), float("inf"), float("inf")
    o, lab = outputs.double(), labels.double()
    rows = R.matched_rows(lab, fg, matched)
    pred, tgt = o[:, :, :4].reshape(-1, 4)[fg.reshape(-1)], rows[:, 1:5]
    pe = torch.cat([pred[:, :2] - pred[:, 2:] / 2, pred[:, :2] + pred[:, 2:] / 2], 1)
    ge = torch.cat([tgt[:, :2] - tgt[:, 2:] / 2, tgt[:, :2] + tgt[:, 2:] / 2], 1)
    _, tl, br = R.iou_of(pred, tgt)
    B, A = fg.shape
    e = [t.double().reshape(1, A).expand(B, A)[fg] for t in (st, xs, ys)]
    res = origin.double().reshape(-1, 4)[fg.reshape(-1)] - R.l1_target(tgt, *e)
    return float((pe - ge).abs().min()), float((br - tl).abs().min()), float(res.abs().min())


def one_case(tag, seed):
    src, use_l1, _ = R.CASES[tag]
    mode = S.CASES[src][4]
    outputs, labels, (H, W, C) = R.problem(tag)
    xs, ys, st = S.anchors(H, W)
    B, A = outputs.shape[:2]
    grad_out = torch.tensor(R.GRAD_OUT, dtype=torch.float64)
    first = seed
    while True:
        assert seed < first + 20, "no draw of origin_preds passes for %s" % tag
        origin = torch.randn(B, A, 4, generator=torch.Generator().manual_seed(seed)).float()
        r64, a64 = reference_losses(mode, C, use_l1, outputs, origin, labels, xs, ys, st, (H, W), grad_out, torch.float64)
        r32, a32 = reference_losses(mode, C, use_l1, outputs, origin, labels, xs, ys, st, (H, W), grad_out.float(), torch.float32)
        assert torch.equal(a64[0], a32[0]) and torch.equal(a64[1], a32[1]) and torch.equal(a64[3], a32[3]), "fp32 and fp64 assign differently"
        edge, span, resid = kinks(outputs, origin, labels, a64[0], a64[1], xs, ys, st)
        assert edge > KINK and span > KINK, (tag, edge, span)
        if resid > KINK or not use_l1:
            break
        print("%s seed %d: L1 residual %.3g -- redrawing origin_preds" % (tag, seed, resid))
        seed += 1
    res = {"outputs": outputs.numpy(), "labels": labels.numpy(), "grad_out": grad_out.numpy(),
           "shape": np.array([H, W, C], dtype=np.int64), "seed": np.int64(seed), "use_l1": np.bool_(use_l1),
           "fg_mask": a64[0].numpy(), "matched_gt_inds": a64[1].numpy(), "matched_ious": a64[2].numpy(), "matched_ious_fp32": a32[2].numpy(),
           "num_fg_per_image": a64[3].numpy(), "kink_edge": np.float64(edge), "kink_span": np.float64(span), "kink_l1": np.float64(resid)}
    if use_l1:
        res["origin_preds"] = origin.numpy()
    for k in R.QUANTITIES:
        if r64[k] is None:
            continue
        res[k], res[k + "_fp32"] = r64[k].numpy(), r32[k].numpy()
        res[k + "_fp32_ref_err"] = np.float64(0.0 if torch.equal(r32[k].double(), r64[k]) else R.rel_err(r32[k], r64[k]))
    disjoint = int((a64[2][a64[0]] == 0).sum())
    res["prop_disjoint"] = np.int64(disjoint)
    print("%-10s seed %d  B %d A %d C %d  num_fg %s  disjoint matched %d  kinks edge %.3g span %.3g l1 %.3g\n           %s" % (
        tag, seed, B, A, C, a64[3].tolist(), disjoint, edge, span, resid,
        "  ".join("%s %.6g (%.2g)" % (k, float(np.abs(res[k]).max()), float(res[k + "_fp32_ref_err"])) for k in R.QUANTITIES if k in res)))
    return res


def main():
    want_disjoint = {"cls4": 9, "small": 11, "edge": 5}
    for k, tag in enumerate(R.CASES):
        res = one_case(tag, 1000 + 100 * k)
        if tag in want_disjoint:
            assert int(res["prop_disjoint"]) == want_disjoint[tag], (tag, int(res["prop_disjoint"]))
        if tag == "empty":
            assert not res["fg_mask"].any() and float(res["num_fg"]) == 1.0
        path = os.path.join(HERE, "head_loss_%s.npz" % tag)
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
