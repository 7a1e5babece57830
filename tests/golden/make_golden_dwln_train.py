"""Golden vectors for the differentiable depthwise 7x7 + LayerNorm operator (uni_dwln_train_fwd / _bwd, ops.dwconv7_ln), produced by EXECUTING
the reference's own ConvNeXt Block (unicorn/models/backbone/convnext.py:19-54) on the CPU: a Block of the case's width gets the drawn
parameters, and the lines of its forward that the operator replaces are run on its own modules,

    blk.norm(blk.dwconv(x).permute(0, 2, 3, 1))                      # convnext.py:43-45

under autograd with a drawn upstream gradient, in fp64 for the results and in fp32 for the yardstick.  Per result,
<name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same modules in fp32: the bound of the fp32 GPU test is 4 x that (no figure comes
from the kernel).  Inputs are stored as fp32 (they lie on a binary grid, tests/dwln_train_ref.py), results as fp64.  No reference text is
stored.

    python tests/golden/make_golden_dwln_train.py        -> tests/golden/dwln_train_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import dwln_train_ref as R  # noqa: E402

MAX_BYTES = 360 * 1024


def reference_block(C, weight, bias, ln_weight, ln_bias, dtype):
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.backbone.convnext import Block
    blk = Block(dim=C).to(dtype)
    assert blk.norm.eps == R.EPS and tuple(blk.dwconv.weight.shape) == (C, 1, 7, 7)
    with torch.no_grad():
        for p, v in ((blk.dwconv.weight, weight), (blk.dwconv.bias, bias), (blk.norm.weight, ln_weight), (blk.norm.bias, ln_bias)):
            p.copy_(v.to(dtype))
    return blk


def evaluate(x, weight, bias, ln_weight, ln_bias, grad_y, dtype):
    blk = reference_block(x.shape[1], weight, bias, ln_weight, ln_bias, dtype)
    xi = x.detach().to(dtype).clone().requires_grad_(True)
    y = blk.norm(blk.dwconv(xi).permute(0, 2, 3, 1))
    y.backward(grad_y.to(dtype))
    return {"y": y.detach(), "gx": xi.grad, "gw": blk.dwconv.weight.grad, "gb": blk.dwconv.bias.grad, "ggamma": blk.norm.weight.grad,
            "gbeta": blk.norm.bias.grad}


def main():
    for k, tag in enumerate(R.CASES):
        B, C, H, W = R.CASES[tag]
        seed = 100 * k
        ins = R.draw(tag, seed)
        for t in ins:
            assert t.dtype == torch.float32
        ref = evaluate(*ins, torch.float64)
        f32 = evaluate(*ins, torch.float32)
        res = {"shape": np.array([B, C, H, W], dtype=np.int64), "seed": np.int64(seed), "eps": np.float64(R.EPS)}
        res.update({n: t.numpy() for n, t in zip(R.INPUTS, ins)})
        for n in R.RESULTS:
            assert ref[n].dtype == torch.float64 and f32[n].dtype == torch.float32 and torch.isfinite(ref[n]).all()
            res[n] = ref[n].numpy()
            res[n + "_fp32_ref_err"] = np.float64(R.rel_err(f32[n], ref[n]))
            print("%-7s %-7s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(ref[n].abs().max()), res[n + "_fp32_ref_err"]))
        path = os.path.join(HERE, "dwln_train_%s.npz" % tag)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        print("%-7s seed %d  %s %d bytes" % (tag, seed, path, size))
        # the size of the largest loss fixture, unless the non-zero fp64 results alone are larger than that (c1536: 360 KiB of them)
        floor = sum(8 * int(np.count_nonzero(res[n])) for n in R.RESULTS)
        assert size <= max(MAX_BYTES, floor + 192 * 1024), "fixture of %d bytes (its fp64 results: %d)" % (size, floor)


if __name__ == "__main__":
    main()
