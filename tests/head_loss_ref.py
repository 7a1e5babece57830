"""Pure-torch restatement of the detection losses of get_losses (unicorn/models/unicorn_head_mask.py:646-745 with IOUloss of
unicorn/models/losses.py:15-36 and get_l1_target :747-752), vectorised over the batch, in the dtype and on the device of its inputs: the
eager lines that ops.head_det_loss replaces, boolean indexing included (every such index reads a count back to the host).  It takes the
assignment as tensors.  tests/test_head_loss_cpu.py pins it to the fixtures the reference's own get_losses produced; the GPU tests and
tools/head_loss_bench.py use it where no fixture exists.  A plain module imported like tests/planted.py; it holds no fixture and changes
no pytest setting."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import simota_ref as S

GOLD = S.GOLD
# tag -> (simota fixture the outputs / labels come from, use_l1, labels zeroed)
CASES = {"sot": ("sot", True, False), "cls4": ("cls4", True, False), "small": ("small", True, False), "edge": ("edge", True, False),
         "tiny": ("tiny", True, False), "batch": ("batch", True, False), "batch_nol1": ("batch", False, False), "empty": ("batch", True, True)}
QUANTITIES = ("iou_loss", "conf_loss", "cls_loss", "l1_loss", "num_fg", "grad_outputs", "grad_origin")
GRAD_OUT = (0.7, 1.3, 0.45, 1.9)       # the weights of the four losses in the recorded backward: unequal, so that a swap shows


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "head_loss_%s.npz" % tag)))


def problem(tag):
    """outputs (B, A, 5 + C) and labels (B, M, 5) fp32 of a case, from the simota fixture it is built on, and (H, W, C)"""
    src, _, zero = CASES[tag]
    H, W, Gs, C, _ = S.CASES[src]
    c = S.load_case(src)
    if len(Gs) == 1:
        outputs = torch.from_numpy(np.concatenate([c["bbox"], c["obj"], c["cls"]], 1))[None]
        labels = torch.from_numpy(np.concatenate([c["gt_classes"][:, None], c["gt_bboxes"]], 1))[None]
    else:
        outputs, labels = torch.from_numpy(c["outputs"]), torch.from_numpy(c["labels"])
    if zero:
        labels = torch.zeros_like(labels)
    return outputs.contiguous(), labels.contiguous(), (H, W, C)


def iou_of(pred, target):
    """losses.py:15-36 up to the IoU: (n, 4), (n, 4) boxes as cx, cy, w, h -> iou (n,), tl (n, 2), br (n, 2)"""
    tl = torch.max(pred[:, :2] - pred[:, 2:] / 2, target[:, :2] - target[:, 2:] / 2)
    br = torch.min(pred[:, :2] + pred[:, 2:] / 2, target[:, :2] + target[:, 2:] / 2)
    area_p, area_g = torch.prod(pred[:, 2:], 1), torch.prod(target[:, 2:], 1)
    en = (tl < br).to(pred.dtype).prod(dim=1)
    area_i = torch.prod(br - tl, 1) * en
    return area_i / (area_p + area_g - area_i + 1e-16), tl, br


def l1_target(gt, stride, xs, ys):
    return torch.stack([gt[:, 0] / stride - xs, gt[:, 1] / stride - ys, torch.log(gt[:, 2] / stride + 1e-8), torch.log(gt[:, 3] / stride + 1e-8)], 1)


def matched_rows(labels, fg, matched):
    """the label row (class, cx, cy, w, h) of every foreground anchor, in (image, anchor) order; indices clamped as the operator does"""
    B, A = fg.shape
    M = labels.shape[1]
    img = torch.arange(B, device=fg.device)[:, None].expand(B, A)[fg]
    return labels[img, matched[fg].long().clamp(min=0, max=max(M - 1, 0))] if M else labels.new_zeros((0, 5))


def det_losses(outputs, origin_preds, labels, fg, matched, iou, xs, ys, st, reg_weight=5.0):
    """outputs (B, A, 5 + C), origin_preds (B, A, 4) or None, labels (B, M, 5), fg (B, A) bool, matched (B, A) integer, iou (B, A), xs / ys /
    st (A,) -> dict of 0-d tensors: iou_loss (times reg_weight), conf_loss, cls_loss, l1_loss, num_fg (the ratio), total_loss"""
    B, A, C = outputs.shape[0], outputs.shape[1], outputs.shape[2] - 5
    dt = outputs.dtype
    flat = fg.reshape(-1)
    rows = matched_rows(labels, fg, matched)
    n = fg.sum().clamp(min=1).to(dt)
    cls_target = F.one_hot(rows[:, 0].long().clamp(min=0, max=C - 1), C).to(dt) * iou[fg].to(dt)[:, None]
    v = iou_of(outputs[:, :, :4].reshape(-1, 4)[flat], rows[:, 1:5])[0]
    loss_iou = (1 - v ** 2).sum() / n
    loss_obj = F.binary_cross_entropy_with_logits(outputs[:, :, 4].reshape(-1, 1), flat[:, None].to(dt), reduction="none").sum() / n
    loss_cls = F.binary_cross_entropy_with_logits(outputs[:, :, 5:].reshape(-1, C)[flat], cls_target, reduction="none").sum() / n
    if origin_preds is not None:
        e = [t.reshape(1, A).expand(B, A)[fg] for t in (st, xs, ys)]
        loss_l1 = (origin_preds.reshape(-1, 4)[flat] - l1_target(rows[:, 1:5], *e)).abs().sum() / n
    else:
        loss_l1 = outputs.new_zeros(())
    num_gt = (labels.sum(dim=2) > 0).sum()
    out = {"iou_loss": reg_weight * loss_iou, "conf_loss": loss_obj, "cls_loss": loss_cls, "l1_loss": loss_l1,
           "num_fg": n / num_gt.clamp(min=1).to(dt)}                # the reference divides its clamped count
    out["total_loss"] = out["iou_loss"] + out["conf_loss"] + out["cls_loss"] + out["l1_loss"]
    return out


def weighted(losses, grad_out):
    """the scalar whose gradient the fixtures record: sum_k grad_out[k] x (iou, conf, cls, l1 loss)"""
    return sum(w * losses[k] for w, k in zip(grad_out, QUANTITIES[:4]))


def run(outputs, origin_preds, labels, fg, matched, iou, xs, ys, st, grad_out, dtype, device="cpu", reg_weight=5.0):
    """the restatement with its backward -> dict of the seven QUANTITIES (grad_origin None without origin_preds), detached"""
    o = outputs.to(device=device, dtype=dtype).clone().requires_grad_(True)
    g = None if origin_preds is None else origin_preds.to(device=device, dtype=dtype).clone().requires_grad_(True)
    f = [t.to(device=device, dtype=dtype) for t in (labels, iou, xs, ys, st)]
    res = det_losses(o, g, f[0], fg.to(device), matched.to(device), f[1], f[2], f[3], f[4], reg_weight)
    weighted(res, [float(w) for w in grad_out]).backward()
    out = {k: res[k].detach() for k in QUANTITIES[:5]}
    out["grad_outputs"], out["grad_origin"] = o.grad, None if g is None else g.grad
    return out


def bound32(ref_err):
    """the fp32 bound of the project (tests/test_mot_corr_gpu.py): 4 x the reference's own fp32-vs-fp64 deviation, floored at one fp32 ulp"""
    return 4.0 * max(float(ref_err), 2.0 ** -23)


def rel_err(got, want):
    """max |got - want| / max |want| in double (0 / 0 = 0: a quantity that is exactly zero must come back exactly zero)"""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d, s = float((got - want).abs().max()) if want.numel() else 0.0, float(want.abs().max()) if want.numel() else 0.0
    return (0.0 if d == 0.0 else float("inf")) if s == 0.0 else d / s
