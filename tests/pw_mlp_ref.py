"""The point-wise middle of a ConvNeXt block (unicorn/models/backbone/convnext.py:46-48) restated in torch -- x = pwconv1(x); x = act(x);
x = pwconv2(x) with act the exact (erf) GELU -- plus the cases and the draws of tests/golden/pw_mlp_*.npz (written by
tests/golden/make_golden_pw_mlp.py from the reference's own Block).  Autograd gives the five gradients; the hidden maps h = pwconv1(t),
a = gelu(h), grad_a and grad_h are returned as well, because the kernels are checked on them without the GEMMs.

Every draw is a plain fp32 normal draw, not on a binary grid: on a grid the sums would be exact in fp32 and the fp32 yardstick zero.

The stand-ins of the drop-in tests are block_tail_ref.StandInBlock and lncf_ref.MiniBackbone."""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from block_tail_ref import StandInBlock  # noqa: F401
from lncf_ref import MiniBackbone  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# tag -> ((N, H, W), C, Hd, Co) and what the case can catch
CASES = {
    "small": ((1, 3, 5), 4, 16, 4),         # the smallest width: four lanes' worth of hidden units
    "c24": ((2, 3, 7), 24, 96, 24),         # 42 rows, a multiple of no rows-per-block value
    "h100": ((2, 3, 7), 20, 100, 12),       # Hd % 8 == 4: a half type stays at 4 columns per lane; Co != C
    "c48": ((3, 4, 8), 48, 192, 48),
}
INPUTS = ("t", "w1", "b1", "w2", "b2", "grad_out")
RESULTS = ("y", "g_t", "g_w1", "g_b1", "g_w2", "g_b2")
HIDDEN = ("h", "a", "grad_a", "grad_h")


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "pw_mlp_%s.npz" % tag)))


def draw(tag, seed, shape=None):
    """-> t (N, H, W, C) = n, w1 (Hd, C) = n / sqrt(C), b1 (Hd,) = 0.1 n, w2 (Co, Hd) = n / sqrt(Hd), b2 (Co,) = 0.1 n, grad_out (N, H, W, Co) = n,
    all fp32; shape: ((N, H, W), C, Hd, Co) for shapes outside CASES"""
    nhw, C, Hd, Co = CASES[tag] if shape is None else shape
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(*nhw, C, generator=g)
    w1 = torch.randn(Hd, C, generator=g) / math.sqrt(C)
    b1 = 0.1 * torch.randn(Hd, generator=g)
    w2 = torch.randn(Co, Hd, generator=g) / math.sqrt(Hd)
    b2 = 0.1 * torch.randn(Co, generator=g)
    grad_out = torch.randn(*nhw, Co, generator=g)
    return t, w1, b1, w2, b2, grad_out


def draw_maps(M, Hd, Co):
    """the kernels' own inputs without the GEMMs -> h, grad_a (M, Hd), grad_y (M, Co): plain fp32 normal draws, seeded by the shape"""
    g = torch.Generator().manual_seed(1000003 * M + 4099 * Hd + Co)
    return torch.randn(M, Hd, generator=g), torch.randn(M, Hd, generator=g), torch.randn(M, Co, generator=g)


def exact_maps(M, Hd, Co, dtype, device="cpu"):
    """-> h = 30 everywhere, grad_a[r, c] = 1 + (r + c) % 3, grad_y[r, c] = 1 + (2 r + c) % 3, and the integer column sums of the two in fp64.
    gelu(30) == 30 and gelu'(30) == 1 in fp64, fp32, fp16 and bf16 arithmetic (Phi(30) rounds to 1, 30 phi(30) = 1e-195 vanishes next to it),
    1, 2, 3 and 30 are numbers of every type and every sum stays below 2^24: a == h, grad_h == grad_a and the sums hold to the last bit, so a
    row or a vector that is dropped, doubled or read from the wrong place changes an integer"""
    r, c = torch.arange(M, device=device)[:, None], torch.arange(max(Hd, Co), device=device)[None, :]
    ga, gy = 1 + (r + c[:, :Hd]) % 3, 1 + (2 * r + c[:, :Co]) % 3
    assert 3 * M < 2 ** 24
    return torch.full((M, Hd), 30.0, device=device, dtype=dtype), ga.to(dtype), gy.to(dtype), ga.double().sum(0), gy.double().sum(0)


def gelu(h, tanh=False):
    """h Phi(h), the exact form; tanh: the approximation, for the test that tells the two apart"""
    if tanh:
        return 0.5 * h * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (h + 0.044715 * h ** 3)))
    return 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))


def gelu_grad(h):
    """Phi(h) + h phi(h)"""
    return 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)


def act_maps(h, grad_a, tanh=False):
    """what the kernels compute from h and grad_a (any shape (..., Hd)), in their dtype: a, grad_h, grad_b1"""
    if tanh:
        hl = h.detach().clone().requires_grad_(True)
        a = gelu(hl, True)
        a.backward(grad_a)
        a, grad_h = a.detach(), hl.grad
    else:
        a, grad_h = gelu(h), grad_a * gelu_grad(h)
    return {"a": a, "grad_h": grad_h, "g_b1": grad_h.reshape(-1, h.shape[-1]).sum(0)}


def value_and_grads(t, w1, b1, w2, b2, grad_out, dtype=None, tanh=False):
    """-> {y, g_t, g_w1, g_b1, g_w2, g_b2, h, a, grad_a, grad_h} of the three lines, computed in `dtype` (default: that of t)"""
    dtype = t.dtype if dtype is None else dtype
    tl, w1l, b1l, w2l, b2l = (x.detach().to(dtype).clone().requires_grad_(True) for x in (t, w1, b1, w2, b2))
    h = F.linear(tl, w1l, b1l)
    a = gelu(h, tanh)
    h.retain_grad(), a.retain_grad()
    y = F.linear(a, w2l, b2l)
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_t": tl.grad, "g_w1": w1l.grad, "g_b1": b1l.grad, "g_w2": w2l.grad, "g_b2": b2l.grad,
            "h": h.detach(), "a": a.detach(), "grad_a": a.grad, "grad_h": h.grad}


def rel_err(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())
