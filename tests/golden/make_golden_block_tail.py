"""Golden vectors for the differentiable ConvNeXt block tail (uni_block_tail_fwd / _bwd, ops.block_tail), produced by EXECUTING the reference's
own ConvNeXt Block (unicorn/models/backbone/convnext.py:19-54) on the CPU: a Block of the case's width, built with drop_path=0, gets the drawn
gamma (layer_scale_init_value=0 for the case without gamma: the Block then has gamma = None), and the lines of its forward that the operator
replaces are run on the block's own gamma and drop_path,

    if blk.gamma is not None: x = blk.gamma * x                      # convnext.py:49-50
    x = x.permute(0, 3, 1, 2)                                        # :51
    x = input + drop(blk.drop_path(x))                               # :53

under autograd with a drawn upstream gradient, in fp64 for the results and in fp32 for the yardstick.  timm is not installed where the
fixtures are written and the DropPath that oracle/ref_bootstrap.py provides is an identity stub, so blk.drop_path is nn.Identity and the
per-sample factor is applied here as timm's drop_path applies it: x * random_tensor with random_tensor of shape (N, 1, 1, 1) holding
bernoulli(keep) / keep, i.e. the case's scale (0 or 1 / keep).  Per result, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same
lines in fp32: the bound of the fp32 GPU test is 4 x that (no figure comes from the kernel).  It must be > 0 wherever the result is
computed; it IS 0 where the result is a copy of grad_out (g_residual always, g_y without gamma and scale), and the operator is held to the
exact bits there.  Inputs are stored as fp32, results as fp64.  No reference text is stored.

    python tests/golden/make_golden_block_tail.py        -> tests/golden/block_tail_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import block_tail_ref as R  # noqa: E402

MAX_BYTES = 360 * 1024


def reference_block(C, gamma, dtype):
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.backbone.convnext import Block
    blk = Block(dim=C, drop_path=0.0, layer_scale_init_value=1.0 if gamma is not None else 0.0).to(dtype)
    assert isinstance(blk.drop_path, torch.nn.Identity) and (blk.gamma is None) == (gamma is None)
    if gamma is not None:
        assert tuple(blk.gamma.shape) == (C,)
        with torch.no_grad():
            blk.gamma.copy_(gamma.to(dtype))
    return blk


def evaluate(y, residual, gamma, scale, grad_out, dtype):
    blk = reference_block(residual.shape[1], gamma, dtype)
    yl, inp = (t.detach().to(dtype).clone().requires_grad_(True) for t in (y, residual))
    x = yl
    if blk.gamma is not None:
        x = blk.gamma * x
    x = x.permute(0, 3, 1, 2)
    x = blk.drop_path(x)
    if scale is not None:
        x = x * scale.to(dtype).view(-1, 1, 1, 1)
    out = inp + x
    out.backward(grad_out.to(dtype))
    res = {"out": out.detach(), "g_residual": inp.grad, "g_y": yl.grad}
    if blk.gamma is not None:
        res["g_gamma"] = blk.gamma.grad
    return res


def main():
    for k, tag in enumerate(R.CASES):
        N, C, H, W = R.CASES[tag]
        seed = 100 * k + 7
        ins = R.draw(tag, seed)
        ref = evaluate(*ins, torch.float64)
        f32 = evaluate(*ins, torch.float32)
        res = {"shape": np.array([N, C, H, W], dtype=np.int64), "seed": np.int64(seed)}
        for n, t in zip(R.INPUTS, ins):
            if t is not None:
                assert t.dtype == torch.float32
                res[n] = t.numpy()
        for n in R.RESULTS:
            if n not in ref:
                assert n == "g_gamma" and ins[2] is None
                continue
            assert ref[n].dtype == torch.float64 and f32[n].dtype == torch.float32 and torch.isfinite(ref[n]).all()
            res[n] = ref[n].numpy()
            err = res[n + "_fp32_ref_err"] = np.float64(R.rel_err(f32[n], ref[n]))
            copy = n == "g_residual" or (n == "g_y" and ins[2] is None and ins[3] is None)
            assert (err == 0) if copy else (err > 0), (tag, n, err)
            print("%-8s %-10s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(ref[n].abs().max()), err))
        path = os.path.join(HERE, "block_tail_%s.npz" % tag)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        print("%-8s seed %d  %s %d bytes" % (tag, seed, path, size))
        assert size <= MAX_BYTES, "fixture of %d bytes" % size


if __name__ == "__main__":
    main()
