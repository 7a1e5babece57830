"""Drop-ins for an existing torch model (training side; operator only, the model-level engine stays inference only).

fuse_dwconv_ln(model) routes the opening of every ConvNeXt block (convnext.py:43-45)

    x = self.dwconv(x); x = x.permute(0, 2, 3, 1); x = self.norm(x)

through unicorn_amd.ops.dwconv7_ln without restating the block's forward: the block's `dwconv` gets an instance-level `forward` that returns
the fused result as an (N, C, H, W) view (`y.permute(0, 3, 1, 2)`), so the block's own permute yields the contiguous (N, H, W, C) tensor, and
its `norm` gets one that hands that tensor on unchanged.  Module tree, parameter names and state_dict() stay as they were.  The two callables
are plain objects that hold the two modules, so copy.deepcopy(model) (ModelEMA) gives a copy whose fused blocks use the copy's parameters.
Outside training mode, and for CPU tensors, both fall back to the modules' original forwards.

fuse_block_tail(model) routes the close of the same block (convnext.py:49-53)

    if self.gamma is not None: x = self.gamma * x
    x = x.permute(0, 3, 1, 2); x = input + self.drop_path(x)

through unicorn_amd.ops.block_tail.  `self.gamma * x` cannot be reached through a submodule, so the BLOCK gets the instance-level `forward`: it
calls the block's own submodules in the reference's order (dwconv -> permute -> norm -> pwconv1 -> act -> pwconv2; fuse_dwconv_ln and module
hooks keep working) and then the operator, whose output is channels-last memory: what the next block's dwconv7_ln reads in place.  The
drop-path mask is drawn as timm's DropPath draws it, so a seeded run drops the same samples fused and unfused.  fuse_convnext applies both.

fuse_layernorm_cf(model) routes the channels-first LayerNorm between the stages (convnext.py:160-184; after the stem, before each downsample
convolution, on the stage outputs) through unicorn_amd.ops.layernorm_cf, which reads channels-last memory (the output of block_tail) and
NCHW memory (the output of the stem convolution) in place and answers in the same layout.  fuse_backbone applies all three.

fuse_pw_mlp(model, keep) routes the point-wise middle of the block (convnext.py:46-48)

    x = self.pwconv1(x); x = self.act(x); x = self.pwconv2(x)

through unicorn_amd.ops.pw_mlp, which keeps one hidden map (keep="hidden") or none (keep="input") for the backward where the eager lines keep
two.  The technique is that of fuse_dwconv_ln: pwconv1 and act get instance-level `forward`s that hand their input on unchanged, pwconv2 one
that runs the operator with both Linears' parameters, so the block's own forward and fuse_block_tail's work unmodified.  fuse_backbone_mlp
applies all four.

fuse_groupnorm_act(model) routes the GroupNorm + SiLU / ReLU lines behind the backbone (BaseConv of the YOLOX-PAFPN and of the head after
convert_bn_model_to_gn, network_blocks.py:29-51; the CondInst mask branch; unicorn.py:38) through unicorn_amd.ops.group_norm_act by the same
technique: the norm runs the operator with the activation, the activation module hands its input on.  fuse_model applies all five.

fuse_downsample(model) routes the four downsample layers (convnext.py:77-87)

    nn.Sequential(nn.Conv2d(in_chans, dims[0], kernel_size=4, stride=4), LayerNorm(dims[0], data_format="channels_first"))
    nn.Sequential(LayerNorm(dims[i], data_format="channels_first"), nn.Conv2d(dims[i], dims[i+1], kernel_size=2, stride=2))

through unicorn_amd.ops.stem_conv and ops.downsample_ln: a convolution whose kernel equals its stride is a GEMM over patches, the GEMM stays
with the vendor library, the LayerNorm is written straight into the patch matrix and rebuilt in the backward, and the result is channels-last
memory, which the next block's dwconv7_ln reads in place.  The paired norm hands its input on unchanged and belongs to the pair:
fuse_layernorm_cf skips it.  fuse_model_down applies all six."""
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
    if Cc % 4 or not 4 <= Cc <= ops.TRAIN_MAX_C:
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


def _drop_path_ok(dp):
    if isinstance(dp, torch.nn.Identity):
        return True
    p = getattr(dp, "drop_prob", None)
    return isinstance(dp, torch.nn.Module) and isinstance(p, float) and 0.0 <= p < 1.0 and isinstance(getattr(dp, "scale_by_keep", True), bool)


def _drop_path_scale(dp, x):
    """the per-sample factor of timm's drop_path (0 or 1 / keep) as an (N, 1, 1, 1) tensor, or None where timm returns its input"""
    if isinstance(dp, torch.nn.Identity) or dp.drop_prob == 0.0 or not dp.training:
        return None
    keep = 1.0 - dp.drop_prob
    mask = torch.empty((x.shape[0], 1, 1, 1), dtype=torch.float32, device=x.device).bernoulli_(keep)
    if keep > 0.0 and getattr(dp, "scale_by_keep", True):
        mask.div_(keep)
    return mask


class _FusedBlockTail:
    """instance-level `forward` of a block: its own submodules, then ops.block_tail"""
    __slots__ = ("block",)

    def __init__(self, block):
        self.block = block

    def __call__(self, x):
        b = self.block
        if not (b.training and x.is_cuda):
            return type(b).forward(b, x)
        y = b.pwconv2(b.act(b.pwconv1(b.norm(b.dwconv(x).permute(0, 2, 3, 1)))))
        scale = _drop_path_scale(b.drop_path, x)
        if scale is not None and x.dtype == torch.float64:
            scale = scale.double()
        return ops.block_tail(y, x, b.gamma, scale)


def _tail_fusable(block):
    if not all(isinstance(getattr(block, n, None), torch.nn.Module) for n in ("dwconv", "norm", "pwconv1", "act", "pwconv2", "drop_path")):
        return False
    Cc = getattr(block.dwconv, "in_channels", None)
    if not isinstance(block.pwconv2, torch.nn.Linear) or not isinstance(Cc, int) or block.pwconv2.out_features != Cc:
        return False
    if Cc % 4 or not 4 <= Cc <= ops.TRAIN_MAX_C or not hasattr(block, "gamma"):
        return False
    g = block.gamma
    if g is not None and not (isinstance(g, torch.nn.Parameter) and tuple(g.shape) == (Cc,)):
        return False
    return _drop_path_ok(block.drop_path)


def fuse_block_tail(model):
    """Fuse the close of every block of `model` that has the modules dwconv, norm, pwconv1, act, pwconv2 (a Linear onto dwconv's C channels;
    C % 4 == 0, C <= 2048) and drop_path (nn.Identity, or a module with a float drop_prob in [0, 1) and an optional scale_by_keep: timm's
    DropPath) and an attribute gamma that is None or a (C,) parameter.  Anything else is left alone.  Returns the number of blocks fused
    (blocks that are fused already are counted).  The block is expected to run the lines of convnext.py:41-54."""
    n = 0
    for block in model.modules():
        if not _tail_fusable(block):
            continue
        if not isinstance(block.__dict__.get("forward"), _FusedBlockTail):
            block.forward = _FusedBlockTail(block)
        n += 1
    return n


def unfuse_block_tail(model):
    """Remove what fuse_block_tail set; returns the number of blocks restored."""
    n = 0
    for m in model.modules():
        if isinstance(m.__dict__.get("forward"), _FusedBlockTail):
            del m.__dict__["forward"]
            n += 1
    return n


def fuse_convnext(model):
    """fuse_dwconv_ln + fuse_block_tail -> (blocks whose opening is fused, blocks whose close is fused)"""
    return fuse_dwconv_ln(model), fuse_block_tail(model)


class _FusedLayerNormCF:
    """instance-level `forward` of a channels-first LayerNorm"""
    __slots__ = ("norm",)

    def __init__(self, norm):
        self.norm = norm

    def __call__(self, x):
        m = self.norm
        if not (m.training and isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda):
            return type(m).forward(m, x)
        return ops.layernorm_cf(x, m.weight, m.bias, m.eps)


def _lncf_fusable(m):
    if not isinstance(m, torch.nn.Module) or getattr(m, "data_format", None) != "channels_first":
        return False
    w, b = getattr(m, "weight", None), getattr(m, "bias", None)
    if not isinstance(w, torch.Tensor) or not isinstance(b, torch.Tensor) or w.dim() != 1 or not isinstance(getattr(m, "eps", None), float):
        return False
    Cc = w.shape[0]
    if tuple(b.shape) != (Cc,) or tuple(getattr(m, "normalized_shape", ())) != (Cc,):
        return False
    return Cc % 4 == 0 and 4 <= Cc <= ops.TRAIN_MAX_C


def fuse_layernorm_cf(model):
    """Route every channels-first LayerNorm of `model` (convnext.py:160-184: data_format == "channels_first", weight and bias (C,), a float eps,
    normalized_shape == (C,); C % 4 == 0, 4 <= C <= 2048) through unicorn_amd.ops.layernorm_cf: the module gets an instance-level `forward`
    that is active in training mode for 4-D device tensors and calls the module's own forward otherwise.  Channels-last norms (the blocks'
    `norm`) and nn.LayerNorm are not touched.  Module tree, parameter names and state_dict() stay as they were.  Returns the number of
    modules fused (modules that are fused already are counted)."""
    n = 0
    for m in model.modules():
        if not _lncf_fusable(m) or isinstance(m.__dict__.get("forward"), _FusedDown):       # fuse_downsample owns the norm of a fused pair
            continue
        if not isinstance(m.__dict__.get("forward"), _FusedLayerNormCF):
            m.forward = _FusedLayerNormCF(m)
        n += 1
    return n


def unfuse_layernorm_cf(model):
    """Remove what fuse_layernorm_cf set; returns the number of modules restored."""
    n = 0
    for m in model.modules():
        if isinstance(m.__dict__.get("forward"), _FusedLayerNormCF):
            del m.__dict__["forward"]
            n += 1
    return n


class _FusedDown:
    """instance-level `forward` of the channels-first LayerNorm (`role` 0: hands its input on unchanged) and of the 2x2 / stride-2 Conv2d behind it
    (`role` 1: runs ops.downsample_ln with both modules' parameters) in a downsample layer"""
    __slots__ = ("norm", "conv", "role")

    def __init__(self, norm, conv, role):
        self.norm, self.conv, self.role = norm, conv, role

    def __call__(self, x):
        n, c = self.norm, self.conv
        if not (n.training and c.training and isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda):
            m = c if self.role else n
            return type(m).forward(m, x)
        if self.role == 0:
            return x
        return ops.downsample_ln(x, n.weight, n.bias, c.weight, c.bias, n.eps)


class _FusedStem:
    """instance-level `forward` of the stem's 4x4 / stride-4 Conv2d: ops.stem_conv; the norm behind it is fuse_layernorm_cf's"""
    __slots__ = ("conv", "norm")

    def __init__(self, conv, norm):
        self.conv, self.norm = conv, norm

    def __call__(self, x):
        c = self.conv
        if not (c.training and self.norm.training and isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda):
            return type(c).forward(c, x)
        return ops.stem_conv(x, c.weight, c.bias)


def _patch_conv_ok(conv, k):
    return (isinstance(conv, torch.nn.Conv2d) and conv.kernel_size == (k, k) and conv.stride == (k, k) and conv.padding == (0, 0)
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.bias is not None and conv.out_channels % 4 == 0
            and 4 <= conv.out_channels <= ops.PW_MLP_MAX_H)


def _down_kind(seq):
    """1: (channels-first LayerNorm, Conv2d 2/2), 2: (Conv2d 4/4 of at most 4 channels, channels-first LayerNorm), 0: neither, or a module
    carries an instance-level forward of somebody else's"""
    if not isinstance(seq, torch.nn.Sequential) or len(seq) != 2:
        return 0
    a, b = seq[0], seq[1]
    if _lncf_fusable(a) and _patch_conv_ok(b, 2) and b.in_channels == a.weight.shape[0]:
        ok = (isinstance(a.__dict__.get("forward"), (_FusedDown, _FusedLayerNormCF, type(None)))
              and isinstance(b.__dict__.get("forward"), (_FusedDown, type(None))))
        return 1 if ok else 0
    if _patch_conv_ok(a, 4) and a.in_channels <= ops.STEM_MAX_CIN and _lncf_fusable(b) and b.weight.shape[0] == a.out_channels:
        return 2 if isinstance(a.__dict__.get("forward"), (_FusedStem, type(None))) else 0
    return 0


def fuse_downsample(model):
    """Route the downsample layers of a ConvNeXt backbone (convnext.py:77-87) through unicorn_amd.ops.downsample_ln and ops.stem_conv, by the
    technique of fuse_pw_mlp.  Two patterns, each an nn.Sequential of exactly two modules:
      - a channels-first LayerNorm that fuse_layernorm_cf would accept, then Conv2d(C, Co, 2, stride=2) with padding 0, dilation 1, groups 1, a
        bias, in_channels == C and Co % 4 == 0: the norm gets an instance-level `forward` that hands x on UNCHANGED, the convolution one that
        runs ops.downsample_ln with both modules' parameters.  A `forward` that fuse_layernorm_cf set on that norm is replaced: the pair owns
        its norm, and fuse_layernorm_cf skips (and does not count) a norm that carries the pair's forward;
      - Conv2d(Cin, Co, 4, stride=4) with padding 0, groups 1, a bias, Cin <= 4 and Co % 4 == 0, then a channels-first LayerNorm over Co: the
        convolution runs ops.stem_conv, whose channels-last result fuse_layernorm_cf's norm reads in place; the norm is left to it.
    Both are active only when both modules are in training mode and x is a 4-D device tensor; otherwise each module runs its own forward.  So
    a forward hook on the norm of a fused pair sees the un-normalised tensor as its output.  No site is skipped by shape.  Module tree,
    parameter names and state_dict() stay as they were; copy.deepcopy(model) gives a copy that uses the copy's parameters.  Returns the
    number of Sequentials fused (those fused already are counted)."""
    n = 0
    for seq in model.modules():
        kind = _down_kind(seq)
        if kind == 1:
            seq[0].forward = _FusedDown(seq[0], seq[1], 0)
            seq[1].forward = _FusedDown(seq[0], seq[1], 1)
        elif kind == 2:
            seq[0].forward = _FusedStem(seq[0], seq[1])
        n += kind != 0
    return n


def unfuse_downsample(model):
    """Remove what fuse_downsample set (and nothing else: a norm it took over from fuse_layernorm_cf runs its own forward until that is
    called again); returns the number of Sequentials restored."""
    n = 0
    for m in model.modules():
        f = m.__dict__.get("forward")
        if isinstance(f, (_FusedDown, _FusedStem)):
            del m.__dict__["forward"]
            n += isinstance(f, _FusedStem) or f.role == 1
    return n


def fuse_backbone(model):
    """fuse_convnext + fuse_layernorm_cf -> (blocks whose opening is fused, blocks whose close is fused, channels-first norms fused)"""
    return fuse_convnext(model) + (fuse_layernorm_cf(model),)


class _FusedPw:
    """instance-level `forward` of one of a block's pwconv1, act, pwconv2 (`role` 0, 1, 2): the first two hand their input on unchanged, the
    third runs ops.pw_mlp with both Linears' parameters"""
    __slots__ = ("pw1", "act", "pw2", "role", "keep")

    def __init__(self, pw1, act, pw2, role, keep):
        self.pw1, self.act, self.pw2, self.role, self.keep = pw1, act, pw2, role, keep

    def __call__(self, x):
        if not (self.pw1.training and self.pw2.training and isinstance(x, torch.Tensor) and x.is_cuda):
            m = (self.pw1, self.act, self.pw2)[self.role]
            return type(m).forward(m, x)
        if self.role < 2:
            return x
        return ops.pw_mlp(x, self.pw1.weight, self.pw1.bias, self.pw2.weight, self.pw2.bias, self.keep)


def _pw_fusable(block):
    p1, act, p2 = (getattr(block, n, None) for n in ("pwconv1", "act", "pwconv2"))
    if not isinstance(p1, torch.nn.Linear) or not isinstance(p2, torch.nn.Linear) or not isinstance(act, torch.nn.GELU):
        return False
    if p1.bias is None or p2.bias is None or p1.out_features != p2.in_features or getattr(act, "approximate", "none") != "none":
        return False
    if any(v % 4 or not 4 <= v <= ops.PW_MLP_MAX_H for v in (p1.out_features, p2.out_features)):
        return False
    return all(isinstance(m.__dict__.get("forward"), (_FusedPw, type(None))) for m in (p1, act, p2))


def fuse_pw_mlp(model, keep="hidden"):
    """Route the point-wise middle `pwconv2(act(pwconv1(x)))` (convnext.py:46-48) of every block of `model` through unicorn_amd.ops.pw_mlp,
    which keeps one hidden map (keep="hidden") or none (keep="input": the backward repeats pwconv1's GEMM) between forward and backward
    where the eager lines keep two.  A block is fused when pwconv1 and pwconv2 are nn.Linear with bias, pwconv1.out_features ==
    pwconv2.in_features, both output widths are multiples of 4 in [4, 8192], act is nn.GELU with approximate == "none", and none of the three
    modules carries an instance-level forward of somebody else's.  The three modules get instance-level `forward`s: in training mode on a
    device tensor pwconv1 and act hand their input on UNCHANGED and pwconv2 runs the operator on both Linears' parameters; otherwise each
    calls its module's own forward.  So a forward hook on pwconv1 or act of a fused block sees the un-transformed tensor (the LayerNorm
    output), and the block is expected to run pwconv1 -> act -> pwconv2 back to back.  Module tree, parameter names and state_dict() stay as
    they were; copy.deepcopy(model) gives a copy that uses the copy's parameters.  Returns the number of blocks that are fused (blocks fused
    earlier are counted; they take the `keep` given now)."""
    if keep not in ops.PW_MLP_KEEP:
        raise ops.L.UnicornHipError("fuse_pw_mlp: keep = %r is not one of %s" % (keep, ", ".join(repr(k) for k in ops.PW_MLP_KEEP)))
    n = 0
    for block in model.modules():
        if not _pw_fusable(block):
            continue
        mods = (block.pwconv1, block.act, block.pwconv2)
        for role, m in enumerate(mods):
            m.forward = _FusedPw(*mods, role, keep)
        n += 1
    return n


def unfuse_pw_mlp(model):
    """Remove what fuse_pw_mlp set; returns the number of blocks restored."""
    n = 0
    for m in model.modules():
        f = m.__dict__.get("forward")
        if isinstance(f, _FusedPw):
            del m.__dict__["forward"]
            n += f.role == 2
    return n


def fuse_backbone_mlp(model, keep="hidden"):
    """fuse_backbone + fuse_pw_mlp -> (blocks whose opening is fused, blocks whose close is fused, channels-first norms fused, blocks whose
    point-wise middle is fused): a fused block then runs no eager point-wise line"""
    return fuse_backbone(model) + (fuse_pw_mlp(model, keep),)


class _FusedGroupNormAct:
    """instance-level `forward` of a GroupNorm (`role` 0: runs ops.group_norm_act with the activation `act`, which may be None) or of the
    activation module behind it (`role` 1: hands its input on unchanged)"""
    __slots__ = ("norm", "act", "role")

    def __init__(self, norm, act, role):
        self.norm, self.act, self.role = norm, act, role

    def __call__(self, x):
        n, a = self.norm, self.act
        m = a if self.role else n
        if not (n.training and (a is None or a.training) and isinstance(x, torch.Tensor) and x.dim() == 4 and x.is_cuda):
            return type(m).forward(m, x)
        if self.role:
            return x
        return ops.group_norm_act(x, n.num_groups, n.weight, n.bias, n.eps, _gn_act_name(a))


def _gn_act_name(a):
    return "none" if a is None else "silu" if isinstance(a, torch.nn.SiLU) else "relu"


def _gn_fusable(m):
    if not isinstance(m, torch.nn.GroupNorm) or not m.affine or m.weight is None or m.bias is None:
        return False
    Cc = m.num_channels
    return Cc % 4 == 0 and 4 <= Cc <= ops.TRAIN_MAX_C and isinstance(m.__dict__.get("forward"), (_FusedGroupNormAct, type(None)))


def _gn_pairs(model):
    """[(norm, activation module or None)] of the three patterns of fuse_groupnorm_act, every norm once, in the order of model.modules()"""
    seen = {}
    for _, m in model.named_modules(remove_duplicate=False):
        seen[id(m)] = seen.get(id(m), 0) + 1
    pairs, done = [], set()

    def add(norm, act):
        if id(norm) in done or not _gn_fusable(norm):
            return
        done.add(id(norm))
        ok = (isinstance(act, (torch.nn.SiLU, torch.nn.ReLU)) and seen[id(norm)] == 1 and seen[id(act)] == 1
              and isinstance(act.__dict__.get("forward"), (_FusedGroupNormAct, type(None))))
        pairs.append((norm, act if ok else None))

    for m in model.modules():
        if isinstance(m, torch.nn.Sequential):
            kids = list(m)
            for i, k in enumerate(kids):
                if isinstance(k, torch.nn.GroupNorm):
                    add(k, kids[i + 1] if i + 1 < len(kids) else None)
        elif isinstance(getattr(m, "bn", None), torch.nn.GroupNorm) and isinstance(getattr(m, "act", None), torch.nn.Module):
            add(m.bn, m.act)
    return pairs


def fuse_groupnorm_act(model):
    """Route the GroupNorm + activation lines of `model` through unicorn_amd.ops.group_norm_act, which keeps x and two numbers per (sample,
    group) for the backward where the eager lines keep two or three maps.  Three patterns are fused:
      - a module with the children `bn` (nn.GroupNorm) and `act` (nn.SiLU or nn.ReLU, in place or not) that runs act(bn(conv(x))): BaseConv
        (network_blocks.py:29-51) after convert_bn_model_to_gn;
      - inside an nn.Sequential, a GroupNorm directly followed by nn.SiLU / nn.ReLU (the CondInst mask branch);
      - a GroupNorm that ends an nn.Sequential or is followed there by anything else (unicorn.py:38): act="none".
    A norm qualifies with affine parameters, C % 4 == 0 and 4 <= C <= 2048; other norms are left alone.  The norm gets an instance-level
    `forward` that runs the operator WITH the activation, the activation module one that hands its input on unchanged; both call their module's
    own forward outside training mode, for CPU tensors and for input that is not 4-D.  The activation module is made the identity only if
    that module object (and the norm) occurs exactly once in model.named_modules(remove_duplicate=False) and it carries no instance-level
    forward of somebody else's; otherwise, and for LeakyReLU and every other activation, the norm alone is fused (act="none") and the activation
    stays eager.  So a forward hook on a fused activation sees the ACTIVATED tensor as its input.  Module tree, parameter names and
    state_dict() stay as they were; copy.deepcopy(model) gives a copy that uses the copy's parameters.  Returns the number of norms fused
    (norms fused earlier are counted)."""
    pairs = _gn_pairs(model)
    for norm, act in pairs:
        norm.forward = _FusedGroupNormAct(norm, act, 0)
        if act is not None:
            act.forward = _FusedGroupNormAct(norm, act, 1)
    return len(pairs)


def unfuse_groupnorm_act(model):
    """Remove what fuse_groupnorm_act set; returns the number of norms restored."""
    n = 0
    for m in model.modules():
        f = m.__dict__.get("forward")
        if isinstance(f, _FusedGroupNormAct):
            del m.__dict__["forward"]
            n += f.role == 0
    return n


def fuse_model(model, keep="hidden"):
    """fuse_backbone_mlp + fuse_groupnorm_act -> the four counts of fuse_backbone_mlp and the number of GroupNorms fused"""
    return fuse_backbone_mlp(model, keep) + (fuse_groupnorm_act(model),)


def fuse_model_down(model, keep="hidden"):
    """fuse_model + fuse_downsample -> the five counts of fuse_model and the number of downsample layers fused (of which fuse_model's count of
    channels-first norms still holds the paired ones: they were fused when it counted them): between the image and the stage outputs no eager
    line, no vendor convolution and no layout conversion is left"""
    return fuse_model(model, keep) + (fuse_downsample(model),)
