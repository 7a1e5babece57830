"""Pure-torch restatement of the CondInst lines of get_losses (unicorn/models/unicorn_head_mask.py:568-569, :675-694, :731-732), per image,
built on the per-instance restatement tests/condinst_loss_ref.py, differentiable, in the dtype and on the device of its inputs: the eager
loop that ops.head_mask_loss replaces, with its boolean indices and its gather of one ground-truth map per foreground anchor.  It takes the
assignment as tensors.  tests/test_head_mask_loss_cpu.py pins it to the fixtures the reference's own get_losses produced; the GPU tests and
tools/head_mask_loss_bench.py use it where no fixture exists.  A plain module imported like tests/planted.py; it holds no fixture and changes
no pytest setting."""
import os

import numpy as np
import torch

import condinst_loss_ref as CR
import simota_ref as S

GOLD = CR.GOLD
# tag -> (head_loss fixture the assignment comes from, up_rate)
CASES = {"sot": ("sot", 4), "batch": ("batch", 4), "edge": ("edge", 4), "small_r2": ("small", 2), "tiny_r8": ("tiny", 8), "empty": ("empty", 4)}
INPUTS = ("mask_feats", "up_masks", "dynamic_params", "fpn_levels", "masks", "grad_out")
QUANTITIES = ("loss_condinst", "per_image", "g_mask_feats", "g_up_masks", "g_dynamic_params")
GRAD_OUT = 1.7          # the weight of loss_condinst in the recorded backward: not 1, so that a dropped factor shows


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "head_mask_loss_%s.npz" % tag)))


def load_assignment(tag):
    """(H, W), fg (B, A) bool, matched (B, A) int64, the anchors and M of the head_loss fixture a case is built on (read only)"""
    c = np.load(os.path.join(GOLD, "head_loss_%s.npz" % CASES[tag][0]))
    H, W, _ = (int(v) for v in c["shape"])
    return (H, W), torch.from_numpy(c["fg_mask"]), torch.from_numpy(c["matched_gt_inds"]), S.anchors(H, W), c["labels"].shape[1]


def instances(b, dynamic_params, fpn_levels, masks, fg, matched, xs, ys, st):
    """:679-684 for image b: the compacted rows of the foreground anchors -> params (N, 169), locations (N, 2), levels (N,), gt (N, rH, rW)"""
    m = fg[b]
    M = masks.shape[1]
    loc = torch.stack([st[m] * (xs[m] + 0.5), st[m] * (ys[m] + 0.5)], dim=1)
    return dynamic_params[b, m], loc, fpn_levels[b, m], masks[b][matched[b, m].long().clamp(min=0, max=M - 1)]


def mask_loss(mask_feats, up_masks, dynamic_params, fpn_levels, masks, fg, matched, xs, ys, st, r):
    """mask_feats (B, 8, H8, W8), up_masks (B, 9 r r, H8, W8), dynamic_params (B, A, 169), fpn_levels (B, A), masks (B, M, r H8, r W8),
    fg (B, A) bool, matched (B, A) integer, xs / ys / st (A,) -> loss_condinst (0-d), loss_masks (B,)"""
    B = mask_feats.shape[0]
    loss_masks, num_valid = [], 0
    for b in range(B):
        if int(fg[b].sum()) > 0:
            p, loc, lvl, gt = instances(b, dynamic_params, fpn_levels, masks, fg, matched, xs, ys, st)
            loss_masks.append(CR.dice_loss(mask_feats[b:b + 1], up_masks[b:b + 1], p, loc, lvl, gt, r).mean())
            num_valid += 1
        else:
            loss_masks.append(torch.sum(mask_feats[b:b + 1]) * 0.0 + torch.sum(dynamic_params[b]) * 0.0)
    loss_masks = torch.stack(loss_masks) if B else dynamic_params.new_zeros((0,))
    return torch.sum(loss_masks) / max(num_valid, 1), loss_masks


def loss_and_grads(mask_feats, up_masks, dynamic_params, fpn_levels, masks, fg, matched, xs, ys, st, r, grad_out, chunk=None):
    """the restatement with its backward -> dict of the five QUANTITIES (dense gradients), detached.  chunk: the instances of an image go
    through condinst_loss_ref.loss_and_grads in chunks of that many (instances are independent; each carries the weight
    grad_out / (N_b num_valid) of the mean and the final division), so that no (N, r H8, r W8) graph is held at the headline geometry"""
    if chunk is None:
        mf, um, dp = (t.detach().clone().requires_grad_(True) for t in (mask_feats, up_masks, dynamic_params))
        loss, per = mask_loss(mf, um, dp, fpn_levels, masks, fg, matched, xs, ys, st, r)
        (loss * grad_out).backward()
        g = [torch.zeros_like(t) if t.grad is None else t.grad for t in (mf, um, dp)]      # the dummy loss of :691 does not touch up_masks
        return {"loss_condinst": loss.detach(), "per_image": per.detach(), "g_mask_feats": g[0], "g_up_masks": g[1], "g_dynamic_params": g[2]}
    B = mask_feats.shape[0]
    counts = fg.sum(dim=1)
    num_valid = max(int((counts > 0).sum()), 1)
    g_mf, g_um, g_dp = torch.zeros_like(mask_feats), torch.zeros_like(up_masks), torch.zeros_like(dynamic_params)
    per = dynamic_params.new_zeros((B,))
    for b in range(B):
        n = int(counts[b])
        if n == 0:
            continue
        p, loc, lvl, gt = instances(b, dynamic_params, fpn_levels, masks, fg, matched, xs, ys, st)
        w = torch.full((n,), float(grad_out) / (n * num_valid), device=p.device, dtype=p.dtype)
        res = CR.loss_and_grads(mask_feats[b:b + 1], up_masks[b:b + 1], p, loc, lvl, gt, r, w, chunk=chunk)
        per[b] = res["loss"].mean()
        g_mf[b:b + 1], g_um[b:b + 1] = res["g_mask_feats"], res["g_up_masks"]
        g_dp[b, fg[b]] = res["g_params"]
    return {"loss_condinst": per.sum() / num_valid, "per_image": per, "g_mask_feats": g_mf, "g_up_masks": g_um, "g_dynamic_params": g_dp}


def fixture_tensors(c, tag, dtype=torch.float64, device="cpu"):
    """the operator's arguments of a fixture: mask_feats, up_masks, dynamic_params, fpn_levels, masks, fg, matched, xs, ys, st, r"""
    _, fg, matched, anchors, _ = load_assignment(tag)
    f = [torch.from_numpy(c[k]).to(device=device, dtype=dtype) for k in ("mask_feats", "up_masks", "dynamic_params", "masks")]
    xs, ys, st = (t.to(device=device, dtype=dtype) for t in anchors)
    return (f[0], f[1], f[2], torch.from_numpy(c["fpn_levels"]).to(device), f[3], fg.to(device), matched.to(device), xs, ys, st, CASES[tag][1])


def expected(c, tag):
    """the recorded fp64 results with g_dynamic_params scattered back to its dense (B, A, 169) form (the file holds the foreground rows)"""
    _, fg, _, _, _ = load_assignment(tag)
    want = {k: torch.from_numpy(np.asarray(c[k])) for k in QUANTITIES[:4]}
    dense = torch.zeros(fg.shape + (169,), dtype=torch.float64)
    dense[fg] = torch.from_numpy(c["g_dynamic_params_fg"])
    want["g_dynamic_params"] = dense
    return want


def bound32(ref_err):
    """the fp32 bound of the project (tests/head_loss_ref.py): 4 x the reference's own fp32-vs-fp64 deviation, floored at one fp32 ulp"""
    return 4.0 * max(float(ref_err), 2.0 ** -23)


def rel_err(got, want):
    """max |got - want| / max |want| in double (0 / 0 = 0: a quantity that is exactly zero must come back exactly zero)"""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d, s = float((got - want).abs().max()) if want.numel() else 0.0, float(want.abs().max()) if want.numel() else 0.0
    return (0.0 if d == 0.0 else float("inf")) if s == 0.0 else d / s
