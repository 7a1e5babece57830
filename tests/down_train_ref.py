"""The downsample layers of the ConvNeXt backbone (unicorn/models/backbone/convnext.py:77-87) restated in torch:

  downsample_ln   the LayerNorm lines of convnext.py:180-183 (lncf_ref.forward) followed by F.conv2d(stride=2) with the 2x2 weight
  stem_conv       F.conv2d(stride=4) with the 4x4 weight

and the PATCH-MATRIX form of both, which is what the HIP kernels compute between the vendor GEMMs: `ln_patches` gives A (M, 4C) and the
statistics, `patches4` the stem's A (M, 16 Cin); `patch_grads` pushes a drawn grad_A back through them with autograd.  The GPU tests hold the
kernels to these without any GEMM.  Autograd gives every gradient.

Every draw is a plain fp32 normal draw, not on a binary grid (on a grid the sums would be exact in fp32 and the yardstick zero); the
convolution weights are n / sqrt(fan_in).  The case `offset` draws x = 10 + 0.01 n: a one-pass E[x^2] - E[x]^2 variance is off by ~18 % there.

The drop-in tests reuse lncf_ref.MiniBackbone (stem + norm, block, norm + downsample, block, output norm)."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import lncf_ref
from lncf_ref import MiniBackbone, rel_err  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-6

# tag -> ((N, C, H, W), Co) and what the case can catch
CASES = {
    "small": ((1, 4, 4, 6), 4),         # smallest C; more than one output pixel, so that grad_bias has a rounding error to measure
    "odd": ((2, 8, 5, 7), 12),          # dropped last row and column: grad_x exact zeros there, nothing of it in A; Co % 8 != 0
    "c96": ((2, 96, 6, 10), 8),         # 60 pixels per image: a 32-pixel group straddles two images and row pairs
    "c100": ((1, 100, 4, 6), 12),       # C % 8 == 4: half x stays at 4 channels per lane
    "c768": ((1, 768, 2, 4), 4),        # many vectors per lane on a map smaller than a group
    "offset": ((1, 64, 4, 4), 8),       # x = 10 + 0.01 n: catches a one-pass variance
}
STEM_CASES = {
    "stem_small": ((1, 3, 8, 12), 4),
    "stem_crop": ((2, 3, 9, 14), 8),    # margins of 1 and 2 dropped
    "stem_c1": ((1, 1, 8, 8), 4),
    "stem_c96": ((1, 3, 8, 12), 96),
}
INPUTS = ("x", "ln_weight", "ln_bias", "weight", "bias", "grad_out")
RESULTS = ("y", "g_x", "g_ln_weight", "g_ln_bias", "g_weight", "g_bias")
STEM_INPUTS = ("x", "weight", "bias", "grad_out")
STEM_RESULTS = ("y", "g_x", "g_weight", "g_bias")


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, fixture_name(tag))))


def fixture_name(tag):
    """`odd` -> down_train_odd.npz, `stem_crop` -> stem_conv_crop.npz"""
    return "stem_conv_%s.npz" % tag[5:] if tag.startswith("stem_") else "down_train_%s.npz" % tag


def draw(tag, seed, shape=None, Co=None):
    """-> x (N, C, H, W), ln_weight (C,) = 1 + 0.1 n, ln_bias (C,) = 0.1 n, weight (Co, C, 2, 2) = n / sqrt(4 C), bias (Co,) = 0.1 n, grad_out
    (N, Co, H // 2, W // 2) = n, all fp32; shape, Co: for shapes outside CASES"""
    (N, C, H, W), Co = (CASES[tag] if shape is None else (shape, Co))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    if tag == "offset":
        x = 10.0 + 0.01 * x
    ln_weight = 1.0 + 0.1 * torch.randn(C, generator=g)
    ln_bias = 0.1 * torch.randn(C, generator=g)
    weight = torch.randn(Co, C, 2, 2, generator=g) / (4 * C) ** 0.5
    bias = 0.1 * torch.randn(Co, generator=g)
    grad_out = torch.randn(N, Co, H // 2, W // 2, generator=g)
    return x, ln_weight, ln_bias, weight, bias, grad_out


def draw_stem(tag, seed, shape=None, Co=None):
    """-> x (N, Cin, H, W), weight (Co, Cin, 4, 4) = n / sqrt(16 Cin), bias (Co,) = 0.1 n, grad_out (N, Co, H // 4, W // 4), all fp32"""
    (N, C, H, W), Co = (STEM_CASES[tag] if shape is None else (shape, Co))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    weight = torch.randn(Co, C, 4, 4, generator=g) / (16 * C) ** 0.5
    bias = 0.1 * torch.randn(Co, generator=g)
    grad_out = torch.randn(N, Co, H // 4, W // 4, generator=g)
    return x, weight, bias, grad_out


def forward(x, ln_weight, ln_bias, weight, bias, eps=EPS):
    """convnext.py:180-183, then the convolution of convnext.py:85"""
    return F.conv2d(lncf_ref.forward(x, ln_weight, ln_bias, eps), weight, bias, stride=2)


def stem_forward(x, weight, bias):
    return F.conv2d(x, weight, bias, stride=4)


def _grads(fn, ins, names, grad_out, dtype):
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in ins]
    y = fn(*leaves)
    y.backward(grad_out.to(dtype))
    out = {"y": y.detach()}
    out.update({"g_" + n: t.grad for n, t in zip(names, leaves)})
    return out


def value_and_grads(x, ln_weight, ln_bias, weight, bias, grad_out, dtype=None, eps=EPS, fn=None):
    """-> {y, g_x, g_ln_weight, g_ln_bias, g_weight, g_bias} of `forward` (or of `fn` with the same arguments), computed in `dtype`"""
    dtype = x.dtype if dtype is None else dtype
    f = (lambda *a: forward(*a, eps)) if fn is None else fn
    return _grads(f, (x, ln_weight, ln_bias, weight, bias), INPUTS[:5], grad_out, dtype)


def stem_value_and_grads(x, weight, bias, grad_out, dtype=None, fn=None):
    dtype = x.dtype if dtype is None else dtype
    return _grads(stem_forward if fn is None else fn, (x, weight, bias), STEM_INPUTS[:3], grad_out, dtype)


# ------------------------------------------------------------------------------------------------ the patch-matrix form
def to_patches(z, k):
    """(N, C, H, W) -> A (N Ho Wo, k k C) of a k x k / stride-k convolution; k == 2: column ((h & 1) 2 + (w & 1)) C + c (a patch is four runs
    of C channels-last elements); k == 4: column (c 4 + kh) 4 + kw (the order of weight.reshape(Co, Cin 16)).  The margin is dropped."""
    N, C, H, W = z.shape
    Ho, Wo = H // k, W // k
    p = z[:, :, :Ho * k, :Wo * k].reshape(N, C, Ho, k, Wo, k)                     # n c ho kh wo kw
    if k == 2:
        return p.permute(0, 2, 4, 3, 5, 1).reshape(N * Ho * Wo, k * k * C)        # n ho wo kh kw c
    return p.permute(0, 2, 4, 1, 3, 5).reshape(N * Ho * Wo, C * k * k)            # n ho wo c kh kw


def weight_matrix(weight):
    """the (Co, K) matrix that multiplies the rows of to_patches"""
    Co, C, k, _ = weight.shape
    return weight.permute(0, 2, 3, 1).reshape(Co, k * k * C) if k == 2 else weight.reshape(Co, C * k * k)


def stats(x, eps=EPS):
    """-> (N H W, 2): mean and 1 / sqrt(var + eps) of every pixel, pixels in (n, h, w) order"""
    u = x.mean(1)
    s = (x - u[:, None]).pow(2).mean(1)
    return torch.stack((u.reshape(-1), 1.0 / torch.sqrt(s.reshape(-1) + eps)), 1)


def ln_patches(x, ln_weight, ln_bias, eps=EPS):
    return to_patches(lncf_ref.forward(x, ln_weight, ln_bias, eps), 2)


def forward_patch(x, ln_weight, ln_bias, weight, bias, eps=EPS):
    """`forward` through the patch matrix: A W2^T + bias, viewed back as (N, Co, Ho, Wo)"""
    N, _, H, W = x.shape
    y = ln_patches(x, ln_weight, ln_bias, eps) @ weight_matrix(weight).t() + bias
    return y.reshape(N, H // 2, W // 2, -1).permute(0, 3, 1, 2)


def stem_forward_patch(x, weight, bias):
    N, _, H, W = x.shape
    y = to_patches(x, 4) @ weight_matrix(weight).t() + bias
    return y.reshape(N, H // 4, W // 4, -1).permute(0, 3, 1, 2)


def patch_grads(x, ln_weight, ln_bias, grad_A, dtype=None, eps=EPS):
    """-> {A, stats, g_x, g_ln_weight, g_ln_bias}: grad_A (M, 4C) pushed back through ln_patches, in `dtype`"""
    dtype = x.dtype if dtype is None else dtype
    xl, wl, bl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, ln_weight, ln_bias))
    A = ln_patches(xl, wl, bl, eps)
    A.backward(grad_A.to(dtype))
    return {"A": A.detach(), "stats": stats(xl.detach(), eps), "g_x": xl.grad, "g_ln_weight": wl.grad, "g_ln_bias": bl.grad}
