"""The opening of a ConvNeXt block (unicorn/models/backbone/convnext.py:32-33,43-45) restated in torch -- F.conv2d (depthwise 7x7, padding 3),
permute to (N, H, W, C), F.layer_norm over C -- plus the cases and the draws of tests/golden/dwln_train_*.npz (written by
tests/golden/make_golden_dwln_train.py from the reference's own Block).  Autograd gives the five gradients.

x and the parameters are drawn on a coarse binary grid (x multiples of 2^-6, the 7x7 weights of 2^-8, the vectors of 2^-10, the `offset` case
finer) so that the fixture files stay small; grad_y is a plain fp32 draw (on a grid its sums would be exact in fp32 and the fp32 yardstick of
gbeta zero).  Every input is fp32."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-6

# tag -> (B, C, H, W) and what the case can catch
CASES = {
    "small": (1, 4, 3, 5),          # map smaller than the window, smallest C
    "c96": (2, 96, 9, 7),           # halo across the image boundary of a batch
    "c192": (1, 192, 5, 13),        # ragged width
    "c1536": (1, 1536, 2, 3),       # widest stage
    "c100": (3, 100, 4, 8),         # C not a multiple of 8 or 64, three images
    "offset": (1, 64, 8, 8),        # conv weight std 0.002, bias 100 + 0.01 noise: a one-pass variance
}
INPUTS = ("x", "weight", "bias", "ln_weight", "ln_bias", "grad_y")
RESULTS = ("y", "gx", "gw", "gb", "ggamma", "gbeta")


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "dwln_train_%s.npz" % tag)))


def _grid(t, bits):
    return torch.round(t * 2.0 ** bits) / 2.0 ** bits


def draw(kind, seed, shape=None):
    """-> x (B, C, H, W), weight (C, 1, 7, 7), bias, ln_weight, ln_bias (C,), grad_y (B, H, W, C), all fp32; kind `offset` draws that case's
    statistics, anything else the plain ones; shape: (B, C, H, W) for shapes outside CASES"""
    B, C, H, W = CASES[kind] if shape is None else shape
    g = torch.Generator().manual_seed(seed)
    x = _grid(torch.randn(B, C, H, W, generator=g), 6)
    if kind == "offset":
        weight = _grid(0.002 * torch.randn(C, 1, 7, 7, generator=g), 16)
        bias = 100 + _grid(0.01 * torch.randn(C, generator=g), 14)
    else:
        weight = _grid(torch.randn(C, 1, 7, 7, generator=g) / 7, 8)
        bias = _grid(0.1 * torch.randn(C, generator=g), 10)
    ln_weight = 1 + _grid(0.1 * torch.randn(C, generator=g), 10)
    ln_bias = _grid(0.1 * torch.randn(C, generator=g), 10)
    grad_y = torch.randn(B, H, W, C, generator=g)
    return x, weight, bias, ln_weight, ln_bias, grad_y


def forward(x, weight, bias, ln_weight, ln_bias, eps=EPS):
    """the three lines: (N, C, H, W) -> (N, H, W, C)"""
    C = x.shape[1]
    u = F.conv2d(x, weight, bias, padding=3, groups=C)
    return F.layer_norm(u.permute(0, 2, 3, 1), (C,), ln_weight, ln_bias, eps)


def value_and_grads(x, weight, bias, ln_weight, ln_bias, grad_y, eps=EPS, fn=forward):
    """-> {y, gx, gw, gb, ggamma, gbeta} of fn in the dtype of the inputs for the upstream gradient grad_y"""
    leaves = [t.detach().clone().requires_grad_(True) for t in (x, weight, bias, ln_weight, ln_bias)]
    y = fn(*leaves, eps)
    y.backward(grad_y.to(y.dtype))
    return dict(zip(RESULTS, [y.detach()] + [t.grad for t in leaves]))


def rel_err(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())
