"""The channels-first LayerNorm of the ConvNeXt backbone (unicorn/models/backbone/convnext.py:160-184, the data_format == "channels_first"
branch) restated in torch -- mean over the channels, biased variance of the centred map, division by sqrt(var + eps), weight[:, None, None] *
x + bias[:, None, None] -- plus the cases and the draws of tests/golden/lncf_train_*.npz (written by tests/golden/make_golden_lncf_train.py
from the reference's own LayerNorm class).  Autograd gives the three gradients.

Every draw is a plain fp32 normal draw, not on a binary grid: on a grid the sums would be exact in fp32 and the fp32 yardstick zero.  The
case `offset` draws x = 100 + 0.01 n: a one-pass E[x^2] - E[x]^2 variance loses every digit there.

Also the stand-ins of the drop-in tests: a module with the reference LayerNorm's attributes and forward, and a mini-backbone built from it
and block_tail_ref.StandInBlock."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from block_tail_ref import StandInBlock

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-6

# tag -> (N, C, H, W) and what the case can catch
CASES = {
    "small": (1, 4, 3, 5),          # smallest C, one lane's worth of channels
    "c96": (2, 96, 9, 7),           # 63 pixels per image: NCHW rows unaligned, a pixel tile that would run into image 2
    "c100": (3, 100, 4, 8),         # C no multiple of 8 or 64 (half x falls back to 4 per lane)
    "c1536": (1, 1536, 2, 3),       # widest stage, map smaller than any tile, most values per lane / slices per column
    "hw130": (1, 8, 10, 13),        # pixels cross a 64- and a 128-pixel edge with few channels, 130 % 4 != 0
    "offset": (1, 64, 8, 8),        # x = 100 + 0.01 n: catches a one-pass variance
}
INPUTS = ("x", "weight", "bias", "grad_out")
RESULTS = ("y", "g_x", "g_weight", "g_bias")


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "lncf_train_%s.npz" % tag)))


def draw(tag, seed, shape=None):
    """-> x (N, C, H, W), weight (C,) = 1 + 0.1 n, bias (C,) = 0.1 n, grad_out (N, C, H, W) = n, all fp32; shape: for shapes outside CASES"""
    N, C, H, W = CASES[tag] if shape is None else shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    if tag == "offset":
        x = 100.0 + 0.01 * x
    weight = 1.0 + 0.1 * torch.randn(C, generator=g)
    bias = 0.1 * torch.randn(C, generator=g)
    grad_out = torch.randn(N, C, H, W, generator=g)
    return x, weight, bias, grad_out


def forward(x, weight, bias, eps=EPS):
    """the four lines of convnext.py:180-183"""
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    x = (x - u) / torch.sqrt(s + eps)
    return weight[:, None, None] * x + bias[:, None, None]


def value_and_grads(x, weight, bias, grad_out, dtype=None, eps=EPS):
    """-> {y, g_x, g_weight, g_bias} of `forward`, computed in `dtype` (default: that of x)"""
    dtype = x.dtype if dtype is None else dtype
    xl, wl, bl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, weight, bias))
    y = forward(xl, wl, bl, eps)
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_x": xl.grad, "g_weight": wl.grad, "g_bias": bl.grad}


def rel_err(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ stand-ins for the drop-in tests
class StandInNorm(nn.Module):
    """the reference's LayerNorm class: the same attributes, the same two branches"""

    def __init__(self, normalized_shape, eps=EPS, data_format="channels_last"):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(normalized_shape))
        self.bias = nn.Parameter(torch.zeros(normalized_shape))
        self.eps = eps
        self.data_format = data_format
        self.normalized_shape = (normalized_shape,)

    def forward(self, x):
        if self.data_format == "channels_last":
            return F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        return forward(x, self.weight, self.bias, self.eps)


def _cf(C):
    m = StandInNorm(C, data_format="channels_first")
    with torch.no_grad():
        m.weight.normal_(1, 0.1), m.bias.normal_(0, 0.1)
    return m


class MiniBackbone(nn.Module):
    """stem convolution + norm, one block, norm + downsample convolution, one block, output norm: the places of the channels-first norm in
    convnext.py:79-106 at two stages"""

    def __init__(self, C=16):
        super().__init__()
        self.stem = nn.Sequential(nn.Conv2d(3, C, kernel_size=4, stride=4), _cf(C))
        self.block1 = StandInBlock(C)
        self.down = nn.Sequential(_cf(C), nn.Conv2d(C, 2 * C, kernel_size=2, stride=2))
        self.block2 = StandInBlock(2 * C)
        self.norm_out = _cf(2 * C)

    def forward(self, x):
        return self.norm_out(self.block2(self.down(self.block1(self.stem(x)))))
