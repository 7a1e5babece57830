"""The close of a ConvNeXt block (unicorn/models/backbone/convnext.py:49-53) restated in torch with an explicit per-sample drop-path factor --
gamma * x, permute to (N, C, H, W), input + x * scale[n] (timm's drop_path multiplies by bernoulli(keep) / keep per sample) -- plus the cases
and the draws of tests/golden/block_tail_*.npz (written by tests/golden/make_golden_block_tail.py from the reference's own Block).  Autograd
gives the three gradients.

Every draw is a plain fp32 normal draw, not on a binary grid: on a grid the products and sums would be exact in fp32 and the fp32 yardstick
zero.  scale entries come from {0, 1 / keep}.

Also the stand-ins of the drop-in tests: timm's DropPath restated and a block with the reference Block's modules and forward."""
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# tag -> (N, C, H, W) and what the case can catch
CASES = {
    "small": (1, 4, 3, 5),          # smallest C
    "c96": (2, 96, 9, 7),           # H W = 63, two images with different factors
    "c100": (3, 100, 4, 8),         # C not a multiple of 8 or 64, middle image dropped
    "c1536": (1, 1536, 2, 3),       # widest stage, map smaller than a transpose tile
    "hw130": (1, 8, 10, 13),        # pixels cross a 64- and a 128-pixel tile edge with few channels
    "nogamma": (2, 8, 3, 3),        # gamma and scale absent
}
# per-sample factors (0 or 1 / keep); None: no drop path
SCALES = {"small": (1 / 0.7,), "c96": (0.0, 1 / 0.7), "c100": (1 / 0.7, 0.0, 1 / 0.7), "c1536": (1 / 0.3,), "hw130": (2.0,), "nogamma": None}
INPUTS = ("y", "residual", "gamma", "scale", "grad_out")
RESULTS = ("out", "g_residual", "g_y", "g_gamma")


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "block_tail_%s.npz" % tag)))


def draw(tag, seed, shape=None, scale="case", gamma=True):
    """-> y (N, H, W, C), residual (N, C, H, W), gamma (C,) or None, scale (N,) or None, grad_out (N, C, H, W), all fp32.  tag `nogamma` draws
    neither gamma nor scale; shape: (N, C, H, W) for shapes outside CASES, then scale is a tuple of N factors or None"""
    N, C, H, W = CASES[tag] if shape is None else shape
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(N, H, W, C, generator=g)
    residual = torch.randn(N, C, H, W, generator=g)
    gam = 0.5 * torch.randn(C, generator=g)
    grad_out = torch.randn(N, C, H, W, generator=g)
    if scale == "case":
        scale = SCALES[tag]
    if tag == "nogamma" or not gamma:
        gam = None
    sc = None if scale is None else torch.tensor(scale, dtype=torch.float32)
    assert sc is None or tuple(sc.shape) == (N,)
    return y, residual, gam, sc, grad_out


def forward(y, residual, gamma, scale):
    """the lines 49-53: (N, H, W, C), (N, C, H, W) -> (N, C, H, W)"""
    x = y
    if gamma is not None:
        x = gamma * x
    x = x.permute(0, 3, 1, 2)
    if scale is not None:
        x = x * scale.view(-1, 1, 1, 1)
    return residual + x


def value_and_grads(y, residual, gamma, scale, grad_out, dtype=None):
    """-> {out, g_residual, g_y, g_gamma (absent without gamma)} of `forward`, computed in `dtype` (default: that of y)"""
    dtype = y.dtype if dtype is None else dtype
    yl, rl = (t.detach().to(dtype).clone().requires_grad_(True) for t in (y, residual))
    gl = None if gamma is None else gamma.detach().to(dtype).clone().requires_grad_(True)
    out = forward(yl, rl, gl, None if scale is None else scale.to(dtype))
    out.backward(grad_out.to(dtype))
    res = {"out": out.detach(), "g_residual": rl.grad, "g_y": yl.grad}
    if gl is not None:
        res["g_gamma"] = gl.grad
    return res


def rel_err(got, ref):
    """max |got - ref| / max |ref| in fp64"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------------------------------------ stand-ins for the drop-in tests
class DropPath(nn.Module):
    """timm's DropPath restated (timm/layers/drop.py: drop_path): per-sample bernoulli(keep) of shape (N, 1, 1, 1), divided by keep.  timm draws
    with x.new_empty, i.e. in the dtype of x, which is fp32 in the block (gamma * x is fp32 even under autocast); this stand-in draws in fp32 for
    every dtype of x, so that an fp64 run of a test drops the samples an fp32 run drops."""

    def __init__(self, drop_prob=0.0, scale_by_keep=True):
        super().__init__()
        self.drop_prob, self.scale_by_keep = drop_prob, scale_by_keep

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = torch.empty((x.shape[0],) + (1,) * (x.ndim - 1), dtype=torch.float32, device=x.device).bernoulli_(keep)
        if keep > 0.0 and self.scale_by_keep:
            mask.div_(keep)
        return x * mask.to(x.dtype)


class StandInBlock(nn.Module):
    """the reference's Block with nn.LayerNorm for its own LayerNorm class"""

    def __init__(self, C, drop_path=0.0, gamma=True, pwconv2=True, dp=None):
        super().__init__()
        self.dwconv = nn.Conv2d(C, C, kernel_size=7, padding=3, groups=C)
        self.norm = nn.LayerNorm(C, eps=1e-6)
        self.pwconv1 = nn.Linear(C, 4 * C)
        self.act = nn.GELU()
        if pwconv2:
            self.pwconv2 = nn.Linear(4 * C, C)
        else:
            self.pw2 = nn.Linear(4 * C, C)
        self.gamma = gamma if isinstance(gamma, nn.Parameter) else nn.Parameter(0.5 * torch.randn(C)) if gamma else None
        self.drop_path = dp if dp is not None else DropPath(drop_path) if drop_path > 0.0 else nn.Identity()

    def forward(self, x):
        input = x
        x = self.dwconv(x)
        x = x.permute(0, 2, 3, 1)
        x = self.norm(x)
        x = self.pwconv1(x)
        x = self.act(x)
        x = self.pwconv2(x) if hasattr(self, "pwconv2") else self.pw2(x)
        if self.gamma is not None:
            x = self.gamma * x
        x = x.permute(0, 3, 1, 2)
        return input + self.drop_path(x)
