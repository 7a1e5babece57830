"""Golden vectors for the fused MOT instance-contrastive loss (uni_mot_corr_loss_fwd / _bwd, ops.mot_corr_loss), produced by EXECUTING the
reference's own Unicorn.compute_loss_mot_corr (unicorn/models/unicorn.py:407-466) on the CPU.  The method needs `self` only for
`bidirect` / `grid_sample`, so the object is made with __new__; Tensor.cuda is a no-op inside this script, and the module's
F.grid_sample is wrapped to cast the grid (fp32, from targets.float()) to the dtype of the map, so that the maps can be fp64.  The
method stores each loss into an fp32 tensor; the two cross_entropy values are therefore recorded by a wrapper and the fp64 loss is formed
from them here.  It is called per sample (bs = 1) in fp64 for the gradients, with the sample's upstream gradient.
Per tensor, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same call with fp32 maps: the yardstick of the fp32 GPU test (no
figure comes from the kernel).  Inputs are stored as fp32, results as fp64.  No reference text is stored.

The fixture rule of tests/mot_corr_ref.py (no sampled coordinate within 1e-3 px of an integer unless a clamp makes it exactly 0 or size-1;
no c / s within 1e-3 of a half-integer unless exactly one) and the property each case is there for are asserted; a draw that fails
either is redrawn with the next seed, never filtered.  So is a draw whose fp32_ref_err of some tensor lies outside
(mot_corr_ref.REF_ERR_MIN, REF_ERR_MAX): below 2^-25 the deviation is an accident of rounding -- a (1,) loss is a single rounding -- and
not the error of an fp32 evaluation, so it cannot serve as a yardstick.

    python tests/golden/make_golden_mot_corr.py        -> tests/golden/mot_corr_<case>.npz
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import mot_corr_ref as R  # noqa: E402


def reference(bidirect, grid_sample):
    """-> (the reference object, the list the cross_entropy values of a call are appended to)"""
    import ref_bootstrap
    ref_bootstrap.boot()
    import torch.nn.functional as F
    from unicorn.models import unicorn as mod
    torch.Tensor.cuda = lambda self, *a, **k: self
    seen = []

    def grid_sample_in_input_dtype(inp, grid, **kw):
        return F.grid_sample(inp, grid.to(inp.dtype), **kw)

    def cross_entropy_recorded(*a, **kw):
        v = F.cross_entropy(*a, **kw)
        seen.append(v.detach().clone())
        return v
    mod.F = types.SimpleNamespace(grid_sample=grid_sample_in_input_dtype, cross_entropy=cross_entropy_recorded)
    net = mod.Unicorn.__new__(mod.Unicorn)
    net.__dict__["bidirect"], net.__dict__["grid_sample"] = bidirect, grid_sample
    return net, seen


def evaluate(e0, e1, targets, grad_loss, bidirect, grid_sample):
    """the reference per sample in the dtype of e0 -> loss (B,), g_embed_0, g_embed_1"""
    net, seen = reference(bidirect, grid_sample)
    B, _, H, W = e0.shape
    a, b_ = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
    loss = []
    for b in range(B):
        del seen[:]
        out = net.compute_loss_mot_corr(a[b:b + 1], b_[b:b + 1], targets[b:b + 1], 1, R.S, H, W)
        assert len(seen) == (2 if bidirect else 1) and out.dtype == torch.float32
        loss.append(0.5 * (seen[0] + seen[1]) if bidirect else seen[0])
        out.backward(grad_loss[b].to(out.dtype))
    return {"loss": torch.stack(loss), "g_embed_0": a.grad, "g_embed_1": b_.grad}


def main():
    for k, tag in enumerate(R.CASES):
        B, C, H, W, M, bidirect, grid_sample, kind = R.CASES[tag]
        seed = 100 * k if kind == tag else int(R.load_case(kind)["seed"])       # `unidir`: the inputs of `plain`, as they were stored
        while True:
            assert kind == tag or seed == int(R.load_case(kind)["seed"]), "%s needs another draw of %s: redraw that case first" % (tag, kind)
            e0, e1, targets, grad_loss = R.draw(kind, seed)
            bad = R.rule_violations(targets, H, W, grid_sample)
            if bad or not R.has_property(tag, targets, H, W):
                print("%-8s seed %d: %s, redrawing" % (tag, seed, "rule broken at %r" % (bad[:2],) if bad else "lacks its property"))
                seed += 1
                continue
            ref = evaluate(e0.double(), e1.double(), targets, grad_loss, bidirect, grid_sample)
            f32 = evaluate(e0, e1, targets, grad_loss, bidirect, grid_sample)
            res = {"shape": np.array([B, C, H, W, M], dtype=np.int64), "seed": np.int64(seed), "bidirect": np.int64(bidirect),
                   "grid_sample": np.int64(grid_sample)}
            for n_, t in (("embed_0", e0), ("embed_1", e1), ("targets", targets), ("grad_loss", grad_loss)):
                assert t.dtype == torch.float32
                res[n_] = t.numpy()
            accident = []
            for n_, t in ref.items():
                assert t.dtype == torch.float64
                res[n_] = t.numpy()
                fin = torch.isfinite(t)
                assert torch.equal(fin, torch.isfinite(f32[n_])), "fp32 and fp64 disagree on NaN positions"
                scale = float(t[fin].abs().max())
                err = float((f32[n_].double() - t)[fin].abs().max() / scale)
                res[n_ + "_fp32_ref_err"] = np.float64(err)
                print("%-8s %-10s max|ref| %.4g  fp32_ref_err %.3g  non-finite %d" % (tag, n_, scale, err, int((~fin).sum())))
                if not R.REF_ERR_MIN < err < R.REF_ERR_MAX:
                    accident.append(n_)
            if accident:
                print("%-8s seed %d: fp32_ref_err of %s is no error of an fp32 evaluation (mot_corr_ref.REF_ERR_MIN), redrawing" % (tag, seed, accident))
                seed += 1
                continue
            path = os.path.join(HERE, "mot_corr_%s.npz" % tag)
            np.savez_compressed(path, **res)
            print("%-8s seed %d  %s %d bytes" % (tag, seed, path, os.path.getsize(path)))
            break


if __name__ == "__main__":
    main()
