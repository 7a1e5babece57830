"""Golden vectors for the fused CondInst mask loss (uni_condinst_loss_fwd / _bwd, ops.condinst_dice_loss), produced by EXECUTING the
reference's own functions on the CPU in fp64 under autograd: parse_dynamic_params, DynamicMaskHead.mask_heads_forward,
DynamicMaskHead.upsample_preds, dice_coefficient (unicorn/models/condinst/dynamic_mask_head.py) and compute_locations (condinst/comm.py).
The relative-coordinate lines :194-202 of mask_heads_forward_with_coords are restated here, because that method hard-codes
device="cuda" at :186.  Per tensor, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same lines run in fp32 on the CPU: the
yardstick of the fp32 GPU test (no figure comes from the kernel).  Inputs are fp32-representable.  No reference text is stored.

No fixture input sits on a ReLU kink: every pre-activation of the two hidden layers has |value| > 1e-6 (asserted; a draw that fails is
redrawn with the next seed, never filtered), so fp32 and fp64 take the same branches.

    python tests/golden/make_golden_condinst_loss.py        -> tests/golden/condinst_loss_<case>.npz
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import condinst_loss_ref as R  # noqa: E402

KINK = 1e-6


def reference_head(up_rate):
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.condinst import dynamic_mask_head as dmh
    from unicorn.models.condinst.comm import compute_locations
    head = dmh.DynamicMaskHead.__new__(dmh.DynamicMaskHead)          # the constructor wants a detectron-style cfg; the methods used need these only
    nn.Module.__init__(head)
    head.up_rate, head.channels, head.in_channels = up_rate, 8, 8
    head.weight_nums, head.bias_nums = [80, 64, 8], [8, 8, 1]
    head.register_buffer("sizes_of_interest", torch.tensor([64, 128, 256, 512, 1024]))
    return head, dmh, compute_locations


def evaluate(mask_feats, up_masks, params, inst_loc, inst_lvl, gt, grad_loss, up_rate):
    """the reference's functions under autograd in the dtype of the inputs -> loss, gradients, hidden pre-activations"""
    head, dmh, compute_locations = reference_head(up_rate)
    mf, um, p = (t.clone().requires_grad_(True) for t in (mask_feats, up_masks, params))
    n, (_, _, H, W) = p.shape[0], mf.shape
    centres = compute_locations(H, W, stride=8, device="cpu").to(inst_loc.dtype)          # (HW, 2) pixel centres, x first
    # the relative coordinates and the stacked head input of :194-206, in this project's words (:186 pins the method to device="cuda"):
    # offset of the instance from every pixel centre over the size of interest of its level, then the eight shared feature channels
    size = head.sizes_of_interest.to(mf.dtype)[inst_lvl.long()]
    offsets = ((inst_loc[:, None, :] - centres[None, :, :]).transpose(1, 2) / size[:, None, None]).to(mf.dtype)      # (n, 2, HW)
    feats = mf.reshape(1, head.in_channels, H * W).expand(n, -1, -1)
    mask_head_inputs = torch.cat([offsets, feats], dim=1).reshape(1, n * (2 + head.in_channels), H, W)
    weights, biases = dmh.parse_dynamic_params(p, head.channels, head.weight_nums, head.bias_nums)
    mask_logits = head.mask_heads_forward(mask_head_inputs, weights, biases, n).reshape(-1, 1, H, W)
    mask_logits = head.upsample_preds(mask_logits, um)
    loss = dmh.dice_coefficient(mask_logits.sigmoid(), gt)
    loss.backward(grad_loss)
    return {"loss": loss.detach(), "g_mask_feats": mf.grad, "g_up_masks": um.grad, "g_params": p.grad}


def draw(tag, seed):
    H, W, r, n = R.CASES[tag]
    g = torch.Generator().manual_seed(seed)
    mask_feats = torch.randn(1, 8, H, W, generator=g)
    up_masks = torch.randn(1, 9 * r * r, H, W, generator=g)
    params = 0.5 * torch.randn(n, 169, generator=g)
    inst_loc = torch.stack([torch.randint(0, 32 * W, (n,), generator=g), torch.randint(0, 32 * H, (n,), generator=g)], dim=1).float() / 4
    inst_lvl = torch.randint(0, 5, (n,), generator=g).to(torch.int32)
    gt = torch.zeros(n, 1, r * H, r * W)
    for i in range(n):                                               # one random box per instance
        y0, x0 = int(torch.randint(0, r * H // 2, (1,), generator=g)), int(torch.randint(0, r * W // 2, (1,), generator=g))
        y1, x1 = y0 + 1 + int(torch.randint(0, r * H // 2, (1,), generator=g)), x0 + 1 + int(torch.randint(0, r * W // 2, (1,), generator=g))
        gt[i, 0, y0:y1, x0:x1] = 1
    if tag == "edge":
        corners = torch.tensor([[0., 0.], [8 * W - 1., 0.], [0., 8 * H - 1.], [8 * W - 1., 8 * H - 1.]])
        inst_loc[:4] = corners                                       # instances located at the image corners
        inst_lvl = torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32)      # levels 0..2
        gt[4] = 0                                                    # an all-zero ground truth
        params[5] *= 40                                              # the sigmoid saturates
        params[3, 152:160] -= 3                                      # ReLUs mostly dead
        params[3, 160:168] -= 1
    grad_loss = torch.randn(n, generator=g)
    return mask_feats, up_masks, params, inst_loc, inst_lvl, gt, grad_loss, r


def main():
    for k, tag in enumerate(R.CASES):
        seed = 100 * k
        while True:
            mask_feats, up_masks, params, inst_loc, inst_lvl, gt, grad_loss, r = draw(tag, seed)
            _, p0, p1 = R.pre_activations(mask_feats.double(), params.double(), inst_loc.double(), inst_lvl)
            kink = min(float(p0.abs().min()), float(p1.abs().min()))
            if kink > KINK:
                break
            print("%-6s seed %d: a pre-activation at %.3g of a ReLU kink, redrawing" % (tag, seed, kink))
            seed += 1
        assert kink > KINK
        ins = {"mask_feats": mask_feats, "up_masks": up_masks, "params": params, "inst_loc": inst_loc, "gt": gt, "grad_loss": grad_loss}
        ref = evaluate(*[t.double() for t in (mask_feats, up_masks, params, inst_loc)], inst_lvl, gt.double(), grad_loss.double(), r)
        f32 = evaluate(mask_feats, up_masks, params, inst_loc, inst_lvl, gt, grad_loss, r)
        res = {"shape": np.array(R.CASES[tag], dtype=np.int64), "seed": np.int64(seed), "min_abs_pre_activation": np.float64(kink),
               "inst_lvl": inst_lvl.numpy()}
        for n_, t in ins.items():
            assert t.dtype == torch.float32
            res[n_] = t.numpy()
        for n_, t in ref.items():
            assert t.dtype == torch.float64
            res[n_] = t.numpy()
            err = float((f32[n_].double() - t).abs().max() / t.abs().max())
            res[n_ + "_fp32_ref_err"] = np.float64(err)
            print("%-6s %-13s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n_, float(t.abs().max()), err))
        dead = float((p0 <= 0).double().mean(dim=(1, 2)).max())
        print("%-6s seed %d, min |pre-activation| %.3g, largest dead share of layer 0 %.2f" % (tag, seed, kink, dead))
        path = os.path.join(HERE, "condinst_loss_%s.npz" % tag)
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
