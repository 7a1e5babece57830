"""GroupNorm followed by an activation (unicorn/models/backbone/network_blocks.py:29-51 after convert_bn_model_to_gn: act(bn(conv(x))) with
bn = GroupNorm(16, C, eps=1e-3) and act = SiLU; the CondInst mask branch: GroupNorm + ReLU; unicorn.py:38: GroupNorm(32, C) alone) restated
in torch -- F.group_norm + the activation under autograd, in a given dtype -- plus the cases and the draws of tests/golden/gn_act_*.npz
(written by tests/golden/make_golden_gn_act.py from the reference's own modules).

Every draw is a plain fp32 normal draw, not on a binary grid: on a grid the sums would be exact in fp32 and the fp32 yardstick zero.  The
case `offset` draws x = 100 + 0.01 n: a one-pass E[x^2] - E[x]^2 variance loses every digit there.

Also the stand-ins of the drop-in tests: BaseConv after the conversion, the two Sequential patterns and a mini-neck built from them."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# tag -> ((N, C, H, W), G, act, eps) and what the case can catch
CASES = {
    "small": ((1, 4, 3, 5), 1, "silu", 1e-3),          # smallest C, one group over everything
    "c96": ((2, 96, 9, 7), 16, "silu", 1e-3),          # cpg = 6: a 4-channel vector straddles two groups; 63 pixels per image; unaligned NCHW rows
    "c100": ((3, 100, 4, 8), 5, "relu", 1e-5),         # C no multiple of 8, cpg = 20, three images
    "c1536": ((1, 1536, 2, 3), 16, "silu", 1e-3),      # widest neck width, map smaller than any tile
    "hw130": ((1, 8, 10, 13), 2, "none", 1e-5),        # pixels cross 64- and 128-pixel edges, 130 % 4 != 0
    "cpg1": ((2, 16, 5, 5), 16, "silu", 1e-3),         # one channel per group
    "g32": ((2, 256, 3, 3), 32, "none", 1e-5),         # unicorn.py:38
    "relu128": ((1, 128, 6, 6), 16, "relu", 1e-5),     # the mask branch
    "offset": ((1, 64, 8, 8), 16, "none", 1e-3),       # x = 100 + 0.01 n: catches a one-pass variance
}
INPUTS = ("x", "weight", "bias", "grad_out")
RESULTS = ("y", "g_x", "g_weight", "g_bias")
ACTS = {"none": lambda z: z, "relu": F.relu, "silu": F.silu}


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "gn_act_%s.npz" % tag)))


def draw(tag, seed, shape=None):
    """-> x (N, C, H, W), weight (C,) = 1 + 0.1 n, bias (C,) = 0.1 n, grad_out (N, C, H, W) = n, all fp32; shape: for shapes outside CASES"""
    N, C, H, W = CASES[tag][0] if shape is None else shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    if tag == "offset":
        x = 100.0 + 0.01 * x
    weight = 1.0 + 0.1 * torch.randn(C, generator=g)
    bias = 0.1 * torch.randn(C, generator=g)
    grad_out = torch.randn(N, C, H, W, generator=g)
    return x, weight, bias, grad_out


def forward(x, weight, bias, G, act, eps):
    return ACTS[act](F.group_norm(x, G, weight, bias, eps))


def pre_activation(x, weight, bias, G, eps, dtype=torch.float64):
    """z, the input of the activation"""
    return F.group_norm(x.to(dtype), G, weight.to(dtype), bias.to(dtype), eps)


def value_and_grads(x, weight, bias, grad_out, G, act, eps, dtype=None):
    """-> {y, g_x, g_weight, g_bias} of `forward`, computed in `dtype` (default: that of x)"""
    dtype = x.dtype if dtype is None else dtype
    xl, wl, bl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (x, weight, bias))
    y = forward(xl, wl, bl, G, act, eps)
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_x": xl.grad, "g_weight": wl.grad, "g_bias": bl.grad}


def rel_err(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ stand-ins for the drop-in tests
def _shake(gn):
    with torch.no_grad():
        gn.weight.normal_(1, 0.1), gn.bias.normal_(0, 0.1)
    return gn


class StandInBaseConv(nn.Module):
    """BaseConv (network_blocks.py:29-51) after convert_bn_model_to_gn: conv / bn = GroupNorm(16, C, eps=1e-3) / act, in place"""

    def __init__(self, cin, cout, ksize=1, stride=1, act="silu", groups=16):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, ksize, stride, (ksize - 1) // 2, bias=False)
        self.bn = _shake(nn.GroupNorm(groups, cout, eps=1e-3))
        self.act = {"silu": nn.SiLU(inplace=True), "relu": nn.ReLU(inplace=True), "lrelu": nn.LeakyReLU(0.1, inplace=True)}[act]

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


def mask_conv(cin, cout):
    """conv_with_kaiming_uniform("BN", activation=True) after the conversion: Sequential(conv, GroupNorm(16, C, eps=1e-5), ReLU(inplace))"""
    return nn.Sequential(nn.Conv2d(cin, cout, 3, padding=1, bias=False), _shake(nn.GroupNorm(16, cout)), nn.ReLU(inplace=True))


def proj_conv(cin, cout):
    """unicorn.py:38: Sequential(conv, GroupNorm(32, C)), no activation"""
    return nn.Sequential(nn.Conv2d(cin, cout, 1), _shake(nn.GroupNorm(32, cout)))


class MiniNeck(nn.Module):
    """two pyramid levels through the patterns above: a lateral BaseConv, an upsample and a concat (PAFPN), a 3x3 BaseConv, a residual add
    (Bottleneck), the mask-branch Sequential and the projection Sequential"""

    def __init__(self, C=32):
        super().__init__()
        self.lateral = StandInBaseConv(2 * C, C)
        self.merge = StandInBaseConv(2 * C, C, ksize=3)
        self.bott = StandInBaseConv(C, C, ksize=3)
        self.mask = mask_conv(C, C)
        self.proj = proj_conv(C, 2 * C)
        self.up = nn.Upsample(scale_factor=2, mode="nearest")

    def forward(self, fine, coarse):
        x = self.merge(torch.cat([self.up(self.lateral(coarse)), fine], 1))
        x = x + self.bott(x)
        return self.proj(self.mask(x))
