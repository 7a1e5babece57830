"""Golden vectors for the batched CondInst mask loss (uni_head_mask_loss_fwd / _bwd, ops.head_mask_loss), produced by EXECUTING the
reference's own UnicornHeadMask.get_losses (unicorn/models/unicorn_head_mask.py:521-745) on the CPU with masks / up_masks / dynamic_params /
fpn_levels given, once in fp64 and once in fp32, with the backward of its loss_condinst.  The first of the two routes was taken: the loop
lines :676-694 and :731-732 themselves run, with a DynamicMaskHead made with __new__ (as tests/golden/make_golden_condinst_loss.py makes
it) as the head's mask_head; the device="cuda" factory calls at unicorn_head_mask.py:568 and dynamic_mask_head.py:186 are redirected by
oracle/ref_bootstrap.py.  The `.float()` of the relative coordinates (dynamic_mask_head.py:195-197) is exact here: locations and pixel
centres are integers and the sizes of interest powers of two.  The per-image losses are recorded by wrapping the mask head's call; the
recorded loss_condinst is :731-732 on them, because :568 accumulates into a float32 buffer in the fp64 run too (see reference_run).
No reference text is stored.

Inputs: outputs / labels / origin_preds and the assignment of tests/golden/head_loss_<source>.npz (only read; the reference is asserted to
reach the recorded fg_mask / matched_gt_inds again in both precisions); mask_feats, up_masks, dynamic_params (scale 0.5) and fpn_levels
drawn from a recorded seed; masks = one random box per label row; grad_out = one non-unit scalar.  Inputs are fp32-representable and
stored as float32; g_dynamic_params is stored for the foreground rows only (g_dynamic_params_fg, in (image, anchor) order) after asserting
that every other row is an exact zero.  Per quantity <name>_fp32_ref_err = max |fp32 - fp64| / max |fp64| (0 where both are exactly zero).

No fixture input sits on a ReLU kink: every hidden pre-activation of a foreground instance has |value| > 1e-6 (asserted; a draw that fails
is redrawn with the next seed, never filtered).

    python tests/golden/make_golden_head_mask_loss.py        -> tests/golden/head_mask_loss_<case>.npz
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import condinst_loss_ref as CR  # noqa: E402
import head_loss_ref as HR  # noqa: E402
import head_mask_loss_ref as R  # noqa: E402
import simota_ref as S  # noqa: E402

KINK = 1e-6


def reference_run(src, ins, r, dtype):
    """the reference's get_losses + backward of loss_condinst on the CPU in `dtype` -> the five quantities and the assignment it reached"""
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.condinst import dynamic_mask_head as dmh
    from unicorn.models.losses import IOUloss
    from unicorn.models.unicorn_head_mask import UnicornHeadMask
    c = HR.load_case(src)
    H, W, C = (int(v) for v in c["shape"])
    mode = S.CASES[HR.CASES[src][0]][4]
    head = UnicornHeadMask.__new__(UnicornHeadMask)
    nn.Module.__init__(head)
    head.mode, head.num_classes, head.num_classes_sot, head.use_l1 = mode, C, C, True
    head.iou_loss = IOUloss(reduction="none")
    head.bcewithlog_loss = nn.BCEWithLogitsLoss(reduction="none")
    head.l1_loss = nn.L1Loss(reduction="none")
    mh = dmh.DynamicMaskHead.__new__(dmh.DynamicMaskHead)            # the constructor wants a detectron-style cfg
    nn.Module.__init__(mh)
    mh.up_rate, mh.channels, mh.in_channels = r, 8, 8
    mh.weight_nums, mh.bias_nums = [80, 64, 8], [8, 8, 1]
    mh.disable_rel_coords, mh.use_raft, mh.boxinst_enabled = False, True, False
    mh.register_buffer("sizes_of_interest", torch.tensor([64, 128, 256, 512, 1024]))
    mh.register_buffer("_iter", torch.zeros([1]))
    per_call = []

    class Recording(nn.Module):
        def forward(self, *a, **k):
            out = mh(*a, **k)
            per_call.append(out["loss_mask"].detach().clone())
            return out
    head.mask_head = Recording()
    seen = {}
    inner = head.get_assignments

    def recording(batch_idx, *rest, **kw):
        got = inner(batch_idx, *rest, **kw)
        seen[batch_idx] = (got[1].clone(), got[3].clone())
        return got
    head.get_assignments = recording
    outputs, labels, origin = (torch.from_numpy(c[k]).to(dtype) for k in ("outputs", "labels", "origin_preds"))
    B, A = outputs.shape[:2]
    xs, ys, st = S.anchors(H, W)
    mf, um, dp = (ins[k].to(dtype).clone().requires_grad_(True) for k in ("mask_feats", "up_masks", "dynamic_params"))
    imgs = torch.zeros(B, 3, H, W, dtype=dtype)
    res = head.get_losses(imgs, [xs.to(dtype)[None]], [ys.to(dtype)[None]], [st.to(dtype)[None]], labels, outputs, [origin], dtype, mf, dp,
                          ins["fpn_levels"].long(), ins["masks"].to(dtype), um)
    loss_condinst = res[5]
    (loss_condinst * float(ins["grad_out"])).backward()
    fg = torch.zeros(B, A, dtype=torch.bool)
    matched = torch.full((B, A), -1, dtype=torch.int64)
    for b, (m, inds) in seen.items():
        fg[b] = m
        matched[b][m] = inds
    per = torch.zeros(B, dtype=dtype)
    per[fg.any(dim=1)] = torch.stack(per_call) if per_call else per[:0]       # the mask head is called for the images with foreground, in order
    # :568 makes loss_masks a float32 buffer whatever the dtype of the run, so the value get_losses returns is rounded to fp32 (the gradient
    # is not: grad_out and 1 / num_valid are exact in fp32).  The recorded value is :731-732 on the mask head's own per-image losses in
    # `dtype`; the returned one is asserted to be its fp32 rounding.
    value = per.sum() / max(len(per_call), 1)
    assert loss_condinst.dtype == torch.float32 and abs(float(loss_condinst) - float(value)) <= 2.0 ** -22 * max(abs(float(value)), 1e-30)
    zero = lambda t, like: torch.zeros_like(like) if t is None else t          # noqa: E731  (no foreground at all: some leaves are untouched)
    return {"loss_condinst": value.reshape(()), "per_image": per, "g_mask_feats": zero(mf.grad, mf),
            "g_up_masks": zero(um.grad, um), "g_dynamic_params": zero(dp.grad, dp)}, (fg, matched)


def draw(tag, seed):
    src, r = R.CASES[tag]
    (H, W), fg, matched, _, M = R.load_assignment(tag)
    B, A = fg.shape
    H8, W8 = H // 8, W // 8
    g = torch.Generator().manual_seed(seed)
    ins = {"mask_feats": torch.randn(B, 8, H8, W8, generator=g), "up_masks": torch.randn(B, 9 * r * r, H8, W8, generator=g),
           "dynamic_params": 0.5 * torch.randn(B, A, 169, generator=g), "fpn_levels": torch.randint(0, 5, (B, A), generator=g).to(torch.int32)}
    masks = torch.zeros(B, M, r * H8, r * W8)
    for b in range(B):
        for m in range(M):                                          # one random box per label row
            y0, x0 = int(torch.randint(0, r * H8 // 2, (1,), generator=g)), int(torch.randint(0, r * W8 // 2, (1,), generator=g))
            y1, x1 = y0 + 1 + int(torch.randint(0, r * H8 // 2, (1,), generator=g)), x0 + 1 + int(torch.randint(0, r * W8 // 2, (1,), generator=g))
            masks[b, m, y0:y1, x0:x1] = 1
    ins["masks"], ins["grad_out"] = masks, torch.tensor(R.GRAD_OUT, dtype=torch.float32)
    return ins, fg, matched


def kink_distance(tag, ins, fg, matched):
    _, _, _, (xs, ys, st), _ = R.load_assignment(tag)
    d = [t.double() for t in (ins["mask_feats"], ins["dynamic_params"], ins["masks"], xs, ys, st)]
    worst = float("inf")
    for b in range(fg.shape[0]):
        if bool(fg[b].any()):
            p, loc, lvl, _ = R.instances(b, d[1], ins["fpn_levels"], d[2], fg, matched, d[3], d[4], d[5])
            _, p0, p1 = CR.pre_activations(d[0][b:b + 1], p, loc, lvl)
            worst = min(worst, float(p0.abs().min()), float(p1.abs().min()))
    return worst


def main():
    for k, tag in enumerate(R.CASES):
        src, r = R.CASES[tag]
        seed = 1000 + 100 * k
        while True:
            ins, fg, matched = draw(tag, seed)
            kink = kink_distance(tag, ins, fg, matched)
            if kink > KINK:
                break
            print("%-8s seed %d: a pre-activation at %.3g of a ReLU kink, redrawing" % (tag, seed, kink))
            seed += 1
        assert kink > KINK
        r64, a64 = reference_run(src, ins, r, torch.float64)
        r32, a32 = reference_run(src, ins, r, torch.float32)
        for a in (a64, a32):
            assert torch.equal(a[0], fg) and torch.equal(a[1][fg], matched[fg]), "the reference does not reach the recorded assignment"
        res = {"shape": np.array([fg.shape[0], fg.shape[1], ins["mask_feats"].shape[2], ins["mask_feats"].shape[3], r, ins["masks"].shape[1]],
                                 dtype=np.int64), "seed": np.int64(seed), "min_abs_pre_activation": np.float64(kink),
               "fpn_levels": ins["fpn_levels"].numpy()}
        for n_ in ("mask_feats", "up_masks", "dynamic_params", "masks", "grad_out"):
            assert ins[n_].dtype == torch.float32
            res[n_] = ins[n_].numpy()
        for n_ in R.QUANTITIES:
            t, f = r64[n_], r32[n_]
            assert t.dtype == torch.float64
            err = 0.0 if torch.equal(f.double(), t) else R.rel_err(f, t)
            if n_ == "g_dynamic_params":
                assert not t[~fg].any() and not f[~fg].any(), "a background row with a gradient"
                res["g_dynamic_params_fg"] = t[fg].numpy()
            else:
                res[n_] = t.numpy()
            res[n_ + "_fp32_ref_err"] = np.float64(err)
            print("%-8s %-17s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n_, float(t.abs().max()) if t.numel() else 0.0, err))
        path = os.path.join(HERE, "head_mask_loss_%s.npz" % tag)
        np.savez_compressed(path, **res)
        print("%-8s seed %d, fg %s, min |pre-activation| %.3g -> %s %d bytes" % (tag, seed, fg.sum(dim=1).tolist(), kink, path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
