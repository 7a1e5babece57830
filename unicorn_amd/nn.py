"""Drop-ins for an existing torch model (training side; operator only, the model-level engine stays inference only).

fuse_dwconv_ln(model) routes the opening of every ConvNeXt block (convnext.py:43-45)

    x = self.dwconv(x); x = x.permute(0, 2, 3, 1); x = self.norm(x)

through unicorn_amd.ops.dwconv7_ln without restating the block's forward: the block's `dwconv` gets an instance-level `forward` that returns
the fused result as an (N, C, H, W) view (`y.permute(0, 3, 1, 2)`), so the block's own permute yields the contiguous (N, H, W, C) tensor, and
its `norm` gets one that hands that tensor on unchanged.  Module tree, parameter names and state_dict() stay as they were.  The two callables
are plain objects that hold the two modules, so copy.deepcopy(model) (ModelEMA) gives a copy whose fused blocks use the copy's parameters.
Outside training mode, and for CPU tensors, both fall back to the modules' original forwards."""
import torch

from . import ops


def _active(dwconv, norm, x):
    return dwconv.training and norm.training and x.is_cuda


class _FusedDwConv:
    """instance-level `forward` of a block's dwconv"""
    __slots__ = ("dwconv", "norm")

    def __init__(self, dwconv, norm):
        self.dwconv, self.norm = dwconv, norm

    def __call__(self, x):
        if not _active(self.dwconv, self.norm, x):
            return type(self.dwconv).forward(self.dwconv, x)
        y = ops.dwconv7_ln(x, self.dwconv.weight, self.dwconv.bias, self.norm.weight, self.norm.bias, self.norm.eps)
        return y.permute(0, 3, 1, 2)


class _FusedNorm:
    """instance-level `forward` of a block's norm: the identity behind a fused dwconv"""
    __slots__ = ("dwconv", "norm")

    def __init__(self, dwconv, norm):
        self.dwconv, self.norm = dwconv, norm

    def __call__(self, x):
        if not _active(self.dwconv, self.norm, x):
            return type(self.norm).forward(self.norm, x)
        return x


def _fusable(block):
    conv, norm = getattr(block, "dwconv", None), getattr(block, "norm", None)
    if not isinstance(conv, torch.nn.Conv2d) or not isinstance(norm, torch.nn.Module):
        return False
    Cc = conv.in_channels
    if not (conv.kernel_size == (7, 7) and conv.padding == (3, 3) and conv.stride == (1, 1) and conv.dilation == (1, 1)
            and conv.padding_mode == "zeros" and conv.groups == Cc == conv.out_channels and conv.bias is not None):
        return False
    if Cc % 4 or not 4 <= Cc <= ops.DWLN_MAX_C:
        return False
    w, b = getattr(norm, "weight", None), getattr(norm, "bias", None)
    if not isinstance(w, torch.Tensor) or not isinstance(b, torch.Tensor) or not isinstance(getattr(norm, "eps", None), float):
        return False
    # normalises the last dimension of C elements: the reference's LayerNorm says so in data_format, nn.LayerNorm in normalized_shape
    if getattr(norm, "data_format", "channels_last") != "channels_last" or tuple(getattr(norm, "normalized_shape", (Cc,))) != (Cc,):
        return False
    return tuple(w.shape) == (Cc,) and tuple(b.shape) == (Cc,)


def fuse_dwconv_ln(model):
    """Fuse every block of `model` that has a depthwise `dwconv` (Conv2d, kernel 7, padding 3, groups == in == out channels, with bias) and a
    channels-last `norm` over its C channels (weight, bias, eps); C % 4 == 0, C <= 2048.  Returns the number of blocks fused (blocks that are
    fused already are counted).  The block is expected to run dwconv -> permute(0, 2, 3, 1) -> norm, as convnext.py:43-45 does."""
    n = 0
    for block in model.modules():
        if not _fusable(block):
            continue
        if not isinstance(block.dwconv.__dict__.get("forward"), _FusedDwConv):
            block.dwconv.forward = _FusedDwConv(block.dwconv, block.norm)
            block.norm.forward = _FusedNorm(block.dwconv, block.norm)
        n += 1
    return n


def unfuse_dwconv_ln(model):
    """Remove what fuse_dwconv_ln set; returns the number of blocks restored."""
    n = 0
    for m in model.modules():
        f = m.__dict__.get("forward")
        if isinstance(f, (_FusedDwConv, _FusedNorm)):
            del m.__dict__["forward"]
            n += isinstance(f, _FusedDwConv)
    return n
