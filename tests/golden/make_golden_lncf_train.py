"""Golden vectors for the differentiable channels-first LayerNorm (uni_lncf_train_fwd / _bwd, ops.layernorm_cf), produced by EXECUTING the
reference's own LayerNorm(C, eps=1e-6, data_format="channels_first") (unicorn/models/backbone/convnext.py:160-184) on the CPU: a module of the
case's width gets the drawn weight and bias and is run under autograd with a drawn upstream gradient, in fp64 for the results and in fp32 for
the yardstick.  Per result, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same module in fp32: the bound of the fp32 GPU test is
4 x that (no figure comes from the kernel) and it must be > 0.  Inputs are stored as fp32, results as fp64.  No reference text is stored.

    python tests/golden/make_golden_lncf_train.py        -> tests/golden/lncf_train_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import lncf_ref as R  # noqa: E402

MAX_BYTES = 360 * 1024


def reference_norm(C, weight, bias, dtype):
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.backbone.convnext import LayerNorm
    m = LayerNorm(C, eps=R.EPS, data_format="channels_first").to(dtype)
    assert tuple(m.weight.shape) == tuple(m.bias.shape) == (C,) and m.eps == R.EPS
    with torch.no_grad():
        m.weight.copy_(weight.to(dtype)), m.bias.copy_(bias.to(dtype))
    return m


def evaluate(x, weight, bias, grad_out, dtype):
    m = reference_norm(x.shape[1], weight, bias, dtype)
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    y = m(xl)
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_x": xl.grad, "g_weight": m.weight.grad, "g_bias": m.bias.grad}


def main():
    for k, tag in enumerate(R.CASES):
        N, C, H, W = R.CASES[tag]
        seed = 100 * k + 11
        ins = R.draw(tag, seed)
        ref = evaluate(*ins, torch.float64)
        f32 = evaluate(*ins, torch.float32)
        res = {"shape": np.array([N, C, H, W], dtype=np.int64), "seed": np.int64(seed)}
        for n, t in zip(R.INPUTS, ins):
            assert t.dtype == torch.float32
            res[n] = t.numpy()
        for n in R.RESULTS:
            assert ref[n].dtype == torch.float64 and f32[n].dtype == torch.float32 and torch.isfinite(ref[n]).all()
            res[n] = ref[n].numpy()
            err = res[n + "_fp32_ref_err"] = np.float64(R.rel_err(f32[n], ref[n]))
            assert 0 < err < 1e-3, (tag, n, err)
            print("%-8s %-10s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(ref[n].abs().max()), err))
        path = os.path.join(HERE, "lncf_train_%s.npz" % tag)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        print("%-8s seed %d  %s %d bytes" % (tag, seed, path, size))
        assert size <= MAX_BYTES, "fixture of %d bytes" % size


if __name__ == "__main__":
    main()
