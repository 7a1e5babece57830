"""Golden vectors for the differentiable GroupNorm + activation (uni_gn_act_train_fwd / _bwd, ops.group_norm_act), produced by EXECUTING the
reference's own modules on the CPU:
  silu   a reference BaseConv (unicorn/models/backbone/network_blocks.py:29-51) with bn.eps = 1e-3, put through the reference's
         convert_bn_model_to_gn(..., num_groups=G) (unicorn/exp/unicorn_track.py:450-470); its `bn` and `act` are run
  relu   conv_with_kaiming_uniform("BN", activation=True) (unicorn/models/condinst/conv_with_kaiming_uniform.py:37-47) converted the same
         way; the modules [1:] (GroupNorm, ReLU) are run
  none   nn.GroupNorm(G, C, eps) as unicorn/models/unicorn.py:38 builds it (there G = 32 and the default eps: the case `g32`)
The modules get the drawn weight and bias and run under autograd with a drawn upstream gradient, in fp64 for the results and in fp32 for the
yardstick.  Per result, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same modules in fp32: the bound of the fp32 GPU test is 4 x
that (no figure comes from the kernel) and it must be > 0.  For the ReLU cases the first seed with min |z| >= 1e-5 in fp64 is taken, so that
the fp32 run flips no mask bit.  Inputs are stored as fp32, results as fp64.  No reference text is stored.

    python tests/golden/make_golden_gn_act.py        -> tests/golden/gn_act_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import gn_act_ref as R  # noqa: E402

MAX_BYTES = 360 * 1024


def reference_modules(C, G, act, eps, weight, bias, dtype):
    """-> (GroupNorm, activation module or None) of the reference, with the drawn parameters"""
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.exp.unicorn_track import convert_bn_model_to_gn
    if act == "silu":
        from unicorn.models.backbone.network_blocks import BaseConv
        m = BaseConv(C, C, 1, 1)
        m.bn.eps = eps
        m = convert_bn_model_to_gn(m, num_groups=G)
        gn, a = m.bn, m.act
        assert isinstance(a, torch.nn.SiLU)
    elif act == "relu":
        from unicorn.models.condinst.conv_with_kaiming_uniform import conv_with_kaiming_uniform
        m = convert_bn_model_to_gn(conv_with_kaiming_uniform("BN", activation=True)(C, C, 3), num_groups=G)
        gn, a = m[1], m[2]
        assert isinstance(a, torch.nn.ReLU) and len(m) == 3
    else:
        gn, a = torch.nn.GroupNorm(G, C, eps=eps), None
    assert isinstance(gn, torch.nn.GroupNorm) and gn.num_groups == G and gn.num_channels == C and gn.eps == eps and gn.affine
    gn = gn.to(dtype)
    with torch.no_grad():
        gn.weight.copy_(weight.to(dtype)), gn.bias.copy_(bias.to(dtype))
    return gn, a


def evaluate(x, weight, bias, grad_out, G, act, eps, dtype):
    gn, a = reference_modules(x.shape[1], G, act, eps, weight, bias, dtype)
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    z = gn(xl)
    zmin = float(z.detach().abs().min())
    y = z if a is None else a(z)                 # in place, as the reference runs it
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_x": xl.grad, "g_weight": gn.weight.grad, "g_bias": gn.bias.grad}, zmin


def main():
    for k, tag in enumerate(R.CASES):
        (N, C, H, W), G, act, eps = R.CASES[tag]
        seed = 100 * k + 11
        while True:
            ins = R.draw(tag, seed)
            ref, zmin = evaluate(*ins, G, act, eps, torch.float64)
            if act != "relu" or zmin >= 1e-5:
                break
            seed += 1
        f32, _ = evaluate(*ins, G, act, eps, torch.float32)
        res = {"shape": np.array([N, C, H, W], dtype=np.int64), "seed": np.int64(seed), "groups": np.int64(G), "eps": np.float64(eps)}
        for n, t in zip(R.INPUTS, ins):
            assert t.dtype == torch.float32
            res[n] = t.numpy()
        for n in R.RESULTS:
            assert ref[n].dtype == torch.float64 and f32[n].dtype == torch.float32 and torch.isfinite(ref[n]).all()
            res[n] = ref[n].numpy()
            err = res[n + "_fp32_ref_err"] = np.float64(R.rel_err(f32[n], ref[n]))
            assert 0 < err < (1e-2 if tag == "offset" else 1e-3), (tag, n, err)
            print("%-8s %-10s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(ref[n].abs().max()), err))
        path = os.path.join(HERE, "gn_act_%s.npz" % tag)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        print("%-8s seed %d  min|z| %.3g  %s %d bytes" % (tag, seed, zmin, path, size))
        assert size <= MAX_BYTES, "fixture of %d bytes" % size


if __name__ == "__main__":
    main()
