#!/usr/bin/env python
"""Generate tests/golden/msda_backward.npz: forward value and the three gradients of multi-scale deformable attention, from the REAL
reference's own pure-PyTorch core (`ms_deform_attn_core_pytorch`, ops/functions/ms_deform_attn_func.py:41-61) under autograd.

The reference is imported through oracle/ref_bootstrap.py (like make_golden.py::run_msda_known_answer); only tensors are stored.

Cases
  a  the shapes and seed of the reference's ops/test.py:21-36 (N=1, M=2, D=2, Lq=2, L=2, P=2, maps (6,4),(3,2))
  b  two equal levels (5,8) at Unicorn's head shape M=8, D=32, P=4, locations in [-0.2, 1.2] (samples outside the map)
  c  ragged: three levels (7,5),(4,9),(3,3), M=3, D=71, P=3, N=2, locations in [-0.3, 1.3]

Inputs and grad_output are stored as fp32; `out` and the three gradients as fp64, evaluated in fp64 ON those fp32-representable inputs.
`fp32_ref_err_<case>` = for (grad_value, grad_sampling_loc, grad_attn_weight): max |reference core in fp32 - in fp64| / max |fp64|,
the reference's own fp32 error and the yardstick of the fp32 HIP tests.

Lattice condition: grad_sampling_loc is discontinuous where a pixel coordinate loc*n - 0.5 is an integer (fp32 and fp64 may floor
differently there), so the inputs are CONSTRUCTED such that no sample has frac(loc*n - 0.5) within MARGIN of 0 or 1: such a sample is
shifted by 0.37/n and re-checked after the fp32 rounding.  No sample is left out of any comparison.  `lattice_ok` is asserted here and
re-asserted by the tests on the loaded file."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))

MARGIN = 1e-3


def lattice_bad(loc, shapes):
    """loc (N,Lq,M,L,P,2) any float dtype -> bool mask of coordinates whose pixel position is within MARGIN of an integer (in fp64)."""
    loc = loc.double()
    n = torch.tensor([[float(w), float(h)] for (h, w) in shapes], dtype=torch.float64)[None, None, None, :, None, :]
    f = loc * n - 0.5
    f = f - torch.floor(f)
    return (f < MARGIN) | (f > 1 - MARGIN)


def lattice_ok(loc, shapes):
    return not bool(lattice_bad(loc, shapes).any())


def make_lattice_safe(loc, shapes):
    """fp32 locations -> fp32 locations satisfying the lattice condition (shift by 0.37/n, re-check after the fp32 rounding)."""
    loc = loc.float().clone()
    n = torch.tensor([[float(w), float(h)] for (h, w) in shapes], dtype=torch.float64)[None, None, None, :, None, :]
    for _ in range(8):
        bad = lattice_bad(loc, shapes)
        if not bad.any():
            return loc
        loc = torch.where(bad, (loc.double() + 0.37 / n).float(), loc)
    raise RuntimeError("lattice construction did not terminate")


def cases():
    out = {}
    # a: ops/test.py:21-36
    torch.manual_seed(3)
    shapes = [(6, 4), (3, 2)]
    S = sum(h * w for h, w in shapes)
    value = torch.rand(1, S, 2, 2) * 0.01
    loc = torch.rand(1, 2, 2, 2, 2, 2)
    attn = torch.rand(1, 2, 2, 2, 2) + 1e-5
    attn /= attn.sum(-1, keepdim=True).sum(-2, keepdim=True)
    out["a"] = (shapes, value, loc, attn, torch.randn(1, 2, 2 * 2))
    # b: Unicorn's head shape, two equal levels, samples outside the map
    torch.manual_seed(5)
    shapes = [(5, 8), (5, 8)]
    N, Lq, M, D, P = 1, 16, 8, 32, 4
    value = torch.randn(N, 80, M, D)
    loc = torch.rand(N, Lq, M, 2, P, 2) * 1.4 - 0.2
    attn = torch.softmax(torch.randn(N, Lq, M, 2 * P), -1).view(N, Lq, M, 2, P)
    out["b"] = (shapes, value, loc, attn, torch.randn(N, Lq, M * D))
    # c: ragged
    torch.manual_seed(6)
    shapes = [(7, 5), (4, 9), (3, 3)]
    N, Lq, M, D, P = 2, 9, 3, 71, 3
    value = torch.randn(N, 80, M, D)
    loc = torch.rand(N, Lq, M, 3, P, 2) * 1.6 - 0.3
    attn = torch.softmax(torch.randn(N, Lq, M, 3 * P), -1).view(N, Lq, M, 3, P)
    out["c"] = (shapes, value, loc, attn, torch.randn(N, Lq, M * D))
    return out


def grads(core, dtype, shapes, value, loc, attn, gout):
    v, l, a = (t.to(dtype).clone().requires_grad_(True) for t in (value, loc, attn))
    o = core(v, torch.as_tensor(shapes, dtype=torch.long), l, a)
    o.backward(gout.to(dtype))
    return o.detach(), v.grad, l.grad, a.grad


def main():
    import ref_bootstrap as rb
    rb.boot()
    from unicorn.models.ops.functions.ms_deform_attn_func import ms_deform_attn_core_pytorch as core
    store = {"margin": np.float64(MARGIN)}
    for name, (shapes, value, loc, attn, gout) in cases().items():
        loc = make_lattice_safe(loc, shapes)
        assert lattice_ok(loc, shapes), name
        o64, gv64, gl64, ga64 = grads(core, torch.float64, shapes, value, loc, attn, gout)
        _, gv32, gl32, ga32 = grads(core, torch.float32, shapes, value, loc, attn, gout)
        err = [float((g32.double() - g64).abs().max() / g64.abs().max()) for g32, g64 in ((gv32, gv64), (gl32, gl64), (ga32, ga64))]
        print("case %s: fp32_ref_err (grad_value, grad_sampling_loc, grad_attn_weight) = %s" % (name, ["%.3e" % e for e in err]))
        for key, t in (("value", value), ("loc", loc), ("attn", attn), ("grad_out", gout)):
            assert t.dtype == torch.float32
            store["%s_%s" % (key, name)] = t.numpy()
        for key, t in (("out", o64), ("grad_value", gv64), ("grad_loc", gl64), ("grad_attn", ga64)):
            assert t.dtype == torch.float64
            store["%s_%s" % (key, name)] = t.numpy()
        store["shapes_%s" % name] = np.array(shapes, dtype=np.int64)
        store["fp32_ref_err_%s" % name] = np.array(err, dtype=np.float64)
    path = os.path.join(HERE, "msda_backward.npz")
    np.savez_compressed(path, **store)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
