"""Golden vectors for the SOT / VOS label-propagation losses (uni_prop_labels, uni_prop_dice_pyramid_fwd / _bwd, ops.sot_prop_loss /
vos_prop_loss), produced by EXECUTING the reference's own Unicorn.compute_loss_sot / compute_loss_vos (unicorn/models/unicorn.py:315-390)
on the CPU.  The object is made with __new__ (the methods need `self` for a few flags and the head); Tensor.cuda is a no-op inside this
script; the module's get_label_map is wrapped so that its fp32 map takes the dtype of the embeddings (the maps can then be fp64; a label is
a multiple of 1/4 and exact in both) and its boxes are recorded; the module's F is a namespace whose interpolate records every call.  The
head is a stub that records pred_lbs1_ms and returns total_loss = sum_l <w_l, prior_l> with the fixed random w_l of the draw, so the priors
have a defined upstream gradient; its first argument carries the sample index.  Everything stored comes from those records: gt0 / gt1 are
the reference's own F.interpolate results, the match table is read off the boxes / masks the reference handed over, corr_loss is the
value the reference put into each loss dict, the gradients are those of the total_loss it returned.

Per float tensor, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same call with fp32 maps: the yardstick of the fp32 GPU test
(no figure comes from the kernel).  Inputs are stored as fp32 (uint8 masks as uint8), results as fp64.  No reference text is stored.

The fixture rules of tests/prop_loss_ref.py (no box corner within 1e-3 of a half-integer, fp32 masks in multiples of 1/256, every
fp32_ref_err inside (REF_ERR_MIN, REF_ERR_MAX), the property each case is there for, the file size) are asserted; a draw that fails one
is redrawn with the next seed, never filtered.

    python tests/golden/make_golden_prop_loss.py        -> tests/golden/prop_loss_<case>.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import prop_loss_ref as R  # noqa: E402


def reference(dtype, head):
    """-> (the reference object, the module, the record lists: boxes handed to get_label_map, (input, output) of every F.interpolate)"""
    import ref_bootstrap
    ref_bootstrap.boot()
    import torch.nn.functional as F
    from unicorn.models import unicorn as mod
    torch.Tensor.cuda = lambda self, *a, **k: self
    if not hasattr(mod, "_get_label_map_of_the_reference"):
        mod._get_label_map_of_the_reference = mod.get_label_map
    boxes, interp = [], []

    def get_label_map_in_map_dtype(b, *a, **k):
        boxes.append(b.detach().clone())
        return mod._get_label_map_of_the_reference(b, *a, **k).to(dtype)

    def interpolate_recorded(x, **kw):
        y = F.interpolate(x, **kw)
        interp.append((x.detach(), y.detach()))
        return y
    mod.get_label_map = get_label_map_in_map_dtype
    mod.F = types.SimpleNamespace(interpolate=interpolate_recorded)
    net = mod.Unicorn.__new__(mod.Unicorn)
    net.__dict__["head"] = head
    return net, boxes, interp


def evaluate(tag, ins, dtype):
    """the reference in `dtype` -> the result dict (tensors of `dtype`, int32 match table)"""
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    Kc, H, W, Q = R.case_kc(tag), 8 * H8, 8 * W8, H8 * W8
    e0, e1 = ins["embed_0"].to(dtype).clone().requires_grad_(True), ins["embed_1"].to(dtype).clone().requires_grad_(True)
    targets = ins["targets"]
    w = [ins[k].to(dtype) for k in ("w8", "w16", "w32")]
    images = torch.zeros(1).expand(B, 2, 3, H, W)
    fpn = (torch.arange(B).view(B, 1),)
    calls, slot_of = [], [0] * B

    def head(fpn_feats, priors, labels, imgs, masks=None, mode=None):
        assert mode == "sot" and len(priors) == 3
        if kind == "sot":
            sel = [x for x in w]
            b, s = None, None
        else:
            b = int(fpn_feats[0][0, 0])
            s = slot_of[b]
            slot_of[b] += 1
            sel = [x[b:b + 1, s:s + 1] for x in w]
        d = {"total_loss": sum((a * p).sum() for a, p in zip(sel, priors))}
        calls.append((b, s, priors, labels.detach().clone(), d))
        return d
    net, boxes, interp = reference(dtype, head)
    res = {"matched": torch.full((B, Kc, 2), -1, dtype=torch.int32), "num_matched": torch.zeros(B, dtype=torch.int32)}
    if kind == "sot":
        out = net.compute_loss_sot(e0, e1, fpn, targets, images)
        assert len(calls) == 1 and len(interp) == 4 and len(boxes) == 2
        pri = calls[0][2]
        res.update(corr_loss=out["corr_loss"].detach(), p8=pri[0].detach(), p16=pri[1].detach(), p32=pri[2].detach(),
                   gt0=interp[0][1].flatten(-2), gt1=interp[3][1].flatten(-2))
        assert torch.equal(boxes[0], targets[:, 0, 0, 1:5]) and torch.equal(boxes[1], targets[:, 1, 0, 1:5])
        res["matched"][:] = 0
        res["num_matched"][:] = 1
    else:
        net.__dict__.update(mhs=max_inst is not None, mhs_wo_head=True, mhs_max_inst=max_inst, init_with_mask=bool(r))
        masks = None
        if r:
            net.__dict__["scale_factor"] = 1 / r
            masks = ins["masks"].to(dtype)
        else:
            masks = torch.zeros(B, 2, M, 1, 1)                      # the reference slices it for the head whatever the mode
        out = net.compute_loss_vos(e0, e1, fpn, targets, images, masks)
        n = len(calls)
        assert n > 0 and len(interp) == 4 * n and len(boxes) == (0 if r else 2 * n)
        for k in ("corr_loss",):
            res[k] = torch.zeros(B, Kc, dtype=dtype)
        res.update(p8=torch.zeros(B, Kc, H8, W8, dtype=dtype), p16=torch.zeros(B, Kc, H8 // 2, W8 // 2, dtype=dtype),
                   p32=torch.zeros(B, Kc, H8 // 4, W8 // 4, dtype=dtype), gt0=torch.zeros(B, Kc, Q, dtype=dtype), gt1=torch.zeros(B, Kc, Q, dtype=dtype))
        for c, (b, s, pri, labels, d) in enumerate(calls):
            g0, g1, q16, q32 = interp[4 * c:4 * c + 4]
            assert torch.equal(q16[0], pri[0].detach()) and torch.equal(q32[1], pri[2].detach())
            if r:                                                   # which masks did the reference hand to F.interpolate?
                i = [k for k in range(M) if torch.equal(masks[b, 0, k], g0[0][0, 0])]
                j = [k for k in range(M) if torch.equal(masks[b, 1, k], g1[0][0, 0])]
            else:                                                   # which boxes did it hand to get_label_map?
                i = [k for k in range(M) if torch.equal(targets[b, 0, k, 1:5], boxes[2 * c][0])]
                j = [k for k in range(M) if torch.equal(targets[b, 1, k, 1:5], boxes[2 * c + 1][0])]
            assert len(i) == 1 and len(j) == 1, "rows of a frame must differ so that the reference's choice can be read off"
            assert torch.equal(labels[0, 0, 1:5], targets[b, 1, j[0], 1:5])
            res["matched"][b, s, 0], res["matched"][b, s, 1] = i[0], j[0]
            res["num_matched"][b] = s + 1
            res["corr_loss"][b, s] = d["corr_loss"].detach()
            res["p8"][b, s], res["p16"][b, s], res["p32"][b, s] = pri[0].detach()[0, 0], pri[1].detach()[0, 0], pri[2].detach()[0, 0]
            res["gt0"][b, s], res["gt1"][b, s] = g0[1].reshape(-1), g1[1].reshape(-1)
    out["total_loss"].backward()
    res["g_embed_0"], res["g_embed_1"] = e0.grad, e1.grad
    return res


def main():
    only = sys.argv[1:]
    for k, tag in enumerate(R.CASES):
        if only and tag not in only:
            continue
        seed = 100 * k
        while True:
            assert seed < 100 * k + 50, "%s: 50 draws failed; the case definition is at fault, not the seed" % tag
            ins = R.draw(tag, seed)
            bad = R.rule_violations(ins["targets"])
            if bad or not R.has_property(tag, ins):
                print("%-12s seed %d: %s, redrawing" % (tag, seed, "rule broken at %r" % (bad[:2],) if bad else "lacks its property"))
                seed += 1
                continue
            ref, f32 = evaluate(tag, ins, torch.float64), evaluate(tag, ins, torch.float32)
            res = {"seed": np.int64(seed)}
            for n_, t in ins.items():
                assert t.dtype in (torch.float32, torch.uint8)
                res[n_] = t.numpy()
            for n_ in R.EXACT_RESULTS:                               # labels and the match table: the same in both precisions, exactly
                assert torch.equal(ref[n_].double(), f32[n_].double()), n_
                res[n_] = ref[n_].numpy()
            accident = []
            for n_ in R.FLOAT_RESULTS:
                t = ref[n_]
                assert t.dtype == torch.float64 and bool(torch.isfinite(t).all()) and bool(torch.isfinite(f32[n_]).all())
                res[n_] = t.numpy()
                scale = float(t.abs().max())
                err = float((f32[n_].double() - t).abs().max() / scale)
                res[n_ + "_fp32_ref_err"] = np.float64(err)
                print("%-12s %-10s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n_, scale, err))
                if not R.REF_ERR_MIN < err < R.REF_ERR_MAX:
                    accident.append(n_)
            if accident:
                print("%-12s seed %d: fp32_ref_err of %s is no error of an fp32 evaluation (prop_loss_ref.REF_ERR_MIN), redrawing" % (tag, seed, accident))
                seed += 1
                continue
            path = os.path.join(HERE, "prop_loss_%s.npz" % tag)
            np.savez_compressed(path, **res)
            size = os.path.getsize(path)
            print("%-12s seed %d  %s %d bytes" % (tag, seed, path, size))
            assert size <= R.FIXTURE_SIZE_LIMIT, (tag, size)
            break


if __name__ == "__main__":
    main()
