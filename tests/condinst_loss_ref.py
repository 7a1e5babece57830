"""Pure-torch restatement of the CondInst mask loss (unicorn/models/condinst/dynamic_mask_head.py:138-170, :172-225, :247-278 with
dice_coefficient :50-58), differentiable, in the dtype of its inputs.  tests/test_condinst_loss_cpu.py pins it to the fixtures the reference's
own functions produced; the GPU tests use it where no fixture exists (the headline geometry).  A plain module imported like tests/planted.py;
it holds no fixture and changes no pytest setting."""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
# tag -> (H8, W8, up_rate, N)
CASES = {"flat": (12, 20, 4, 5), "ragged": (7, 13, 4, 3), "r2": (10, 14, 2, 4), "r8": (6, 10, 8, 3), "edge": (9, 11, 4, 6)}
INPUTS = ("mask_feats", "up_masks", "params", "inst_loc", "gt", "grad_loss")
OUTPUTS = ("loss", "g_mask_feats", "g_up_masks", "g_params")
SOI = (64.0, 128.0, 256.0, 512.0, 1024.0)


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "condinst_loss_%s.npz" % tag)))


def pre_activations(mask_feats, params, inst_loc, inst_lvl):
    """mask_feats (1,8,H,W), params (N,169), inst_loc (N,2), inst_lvl (N,) -> logits (N,H,W), pre-activations of the two hidden layers (N,8,HW)"""
    _, _, H, W = mask_feats.shape
    n, dt = params.shape[0], params.dtype
    xs = torch.arange(W, device=params.device, dtype=dt) * 8 + 4
    ys = torch.arange(H, device=params.device, dtype=dt) * 8 + 4
    soi = torch.tensor(SOI, device=params.device, dtype=dt)[inst_lvl.long()]
    rel_x = ((inst_loc[:, 0, None, None] - xs[None, None, :]) / soi[:, None, None]).expand(n, H, W)
    rel_y = ((inst_loc[:, 1, None, None] - ys[None, :, None]) / soi[:, None, None]).expand(n, H, W)
    x = torch.cat([rel_x.reshape(n, 1, H * W), rel_y.reshape(n, 1, H * W), mask_feats.reshape(1, 8, H * W).expand(n, 8, H * W)], dim=1)
    w0, w1, w2 = params[:, :80].reshape(n, 8, 10), params[:, 80:144].reshape(n, 8, 8), params[:, 144:152].reshape(n, 1, 8)
    b0, b1, b2 = params[:, 152:160], params[:, 160:168], params[:, 168:169]
    p0 = torch.bmm(w0, x) + b0[:, :, None]
    p1 = torch.bmm(w1, torch.relu(p0)) + b1[:, :, None]
    logits = torch.bmm(w2, torch.relu(p1)) + b2[:, :, None]
    return logits.reshape(n, H, W), p0, p1


def dice_loss(mask_feats, up_masks, params, inst_loc, inst_lvl, gt, r):
    """-> (N,) per-instance losses; gt (N, rH, rW) or (N, 1, rH, rW)"""
    _, _, H, W = mask_feats.shape
    n = params.shape[0]
    logits, _, _ = pre_activations(mask_feats, params, inst_loc, inst_lvl)
    w = torch.softmax(up_masks.reshape(9, r, r, H, W), dim=0)
    lp = F.pad(logits, (1, 1, 1, 1))
    u = 0
    for t in range(9):                                   # F.unfold(pred, [3, 3], padding=1): tap t = 3 ky + kx reads (y + ky - 1, x + kx - 1)
        u = u + w[t][None] * lp[:, None, None, t // 3:t // 3 + H, t % 3:t % 3 + W]
    s = torch.sigmoid(u.permute(0, 3, 1, 4, 2).reshape(n, -1))          # (N, r, r, H, W) -> (N, H, r, W, r)
    g = gt.reshape(n, -1)
    inter = (s * g).sum(dim=1)
    union = (s ** 2.0).sum(dim=1) + (g ** 2.0).sum(dim=1) + 1e-5
    return 1. - (2 * inter / union)


def loss_and_grads(mask_feats, up_masks, params, inst_loc, inst_lvl, gt, r, grad_loss, chunk=None):
    """the restatement under autograd, optionally in instance chunks (instances are independent; the shared maps' gradients add up)"""
    mf, um = mask_feats.detach().clone().requires_grad_(True), up_masks.detach().clone().requires_grad_(True)
    n = params.shape[0]
    chunk = chunk or max(n, 1)
    losses, gps = [], []
    for i0 in range(0, n, chunk):
        p = params[i0:i0 + chunk].detach().clone().requires_grad_(True)
        ls = dice_loss(mf, um, p, inst_loc[i0:i0 + chunk], inst_lvl[i0:i0 + chunk], gt[i0:i0 + chunk], r)
        ls.backward(grad_loss[i0:i0 + chunk])
        losses.append(ls.detach())
        gps.append(p.grad)
    return {"loss": torch.cat(losses), "g_mask_feats": mf.grad, "g_up_masks": um.grad, "g_params": torch.cat(gps)}
