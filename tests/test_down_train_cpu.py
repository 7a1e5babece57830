"""CPU half of the differentiable downsample layers (ops.downsample_ln, ops.stem_conv, nn.fuse_downsample): the fixtures equal the restatement
and its patch-matrix form, the yardsticks are positive, the drop-in leaves the module tree alone and shares the channels-first norms with
fuse_layernorm_cf in either order, argument errors come before the library is touched, and an addressing defect is far outside rounding."""
import copy

import numpy as np
import pytest
import torch

import down_train_ref as R
from unicorn_amd import _lib, nn as unn, ops


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fixture_equals_the_restatement(tag):
    c = R.load_case(tag)
    ins = [torch.from_numpy(c[n]) for n in R.INPUTS]
    assert tuple(c["shape"]) == R.CASES[tag][0] + (R.CASES[tag][1],)
    for got, again in zip(ins, R.draw(tag, int(c["seed"]))):
        assert torch.equal(got, again)
    for fn in (None, lambda *a: R.forward_patch(*a)):
        ref = R.value_and_grads(*ins, dtype=torch.float64, fn=fn)
        for k in R.RESULTS:
            assert R.rel_err(ref[k], torch.from_numpy(c[k])) <= 1e-12, (tag, k)
    for k in R.RESULTS:
        assert c[k].dtype == np.float64 and 0 < float(c[k + "_fp32_ref_err"]) < 1e-3, (tag, k)
    if tag == "odd":                                  # the dropped row and column receive exact zeros
        assert not c["g_x"][:, :, 4:, :].any() and not c["g_x"][:, :, :, 6:].any() and c["g_x"][:, :, :4, :6].all()


@pytest.mark.parametrize("tag", list(R.STEM_CASES))
def test_stem_fixture_equals_the_restatement(tag):
    c = R.load_case(tag)
    ins = [torch.from_numpy(c[n]) for n in R.STEM_INPUTS]
    for got, again in zip(ins, R.draw_stem(tag, int(c["seed"]))):
        assert torch.equal(got, again)
    for fn in (None, R.stem_forward_patch):
        ref = R.stem_value_and_grads(*ins, dtype=torch.float64, fn=fn)
        for k in R.STEM_RESULTS:
            assert R.rel_err(ref[k], torch.from_numpy(c[k])) <= 1e-12, (tag, k)
    for k in R.STEM_RESULTS:
        assert 0 < float(c[k + "_fp32_ref_err"]) < 1e-3, (tag, k)
    if tag == "stem_crop":
        assert not c["g_x"][:, :, 8:, :].any() and not c["g_x"][:, :, :, 12:].any()


def test_an_addressing_defect_is_far_outside_rounding():
    """one 4-channel vector of x lost, or one patch quadrant swapped with its neighbour: y and grad_x move by more than 100 x the fp32 bound"""
    c = R.load_case("c96")
    ins = [torch.from_numpy(c[n]).double() for n in R.INPUTS]
    x, lw, lb, w, b, go = ins
    ref = R.value_and_grads(*ins)

    def zeroed(x_, *rest):
        x_ = x_.clone()
        x_[0, 8:12, 2, 3] = 0
        return R.forward(x_, *rest)

    def swapped(x_, lw_, lb_, w_, b_):
        A = R.ln_patches(x_, lw_, lb_)
        C = x_.shape[1]
        A = torch.cat((A[:, C:2 * C], A[:, :C], A[:, 2 * C:]), 1)
        y = A @ R.weight_matrix(w_).t() + b_
        return y.reshape(x_.shape[0], x_.shape[2] // 2, x_.shape[3] // 2, -1).permute(0, 3, 1, 2)

    for fn in (zeroed, swapped):
        bad = R.value_and_grads(*ins, fn=fn)
        for k in ("y", "g_x"):
            assert R.rel_err(bad[k], ref[k]) > 100 * 4 * float(c[k + "_fp32_ref_err"]), (fn.__name__, k)


def _forwards(net):
    return {n: type(m.__dict__["forward"]).__name__ for n, m in net.named_modules() if "forward" in m.__dict__}


def test_fuse_downsample_leaves_the_module_tree_alone():
    torch.manual_seed(3)
    net, plain = R.MiniBackbone(), None
    plain = copy.deepcopy(net)
    keys, tree = list(net.state_dict()), [n for n, _ in net.named_modules()]
    assert unn.fuse_downsample(net) == 2 and unn.fuse_downsample(net) == 2
    assert list(net.state_dict()) == keys and [n for n, _ in net.named_modules()] == tree
    assert _forwards(net) == {"stem.0": "_FusedStem", "down.0": "_FusedDown", "down.1": "_FusedDown"}
    x = torch.randn(2, 3, 16, 24)
    assert torch.equal(net(x), plain(x))                                   # CPU tensors: every module runs its own forward
    net.eval(), plain.eval()
    assert torch.equal(net(x), plain(x))
    dup = copy.deepcopy(net)
    f = dup.down[1].__dict__["forward"]
    assert f.norm is dup.down[0] and f.conv is dup.down[1] and f.conv is not net.down[1]
    assert dup.stem[0].__dict__["forward"].conv is dup.stem[0]
    with torch.no_grad():
        dup.down[1].weight.zero_(), dup.down[1].bias.zero_()
    assert net.down[1].weight.abs().sum() > 0
    assert unn.unfuse_downsample(net) == 2 and _forwards(net) == {} and unn.unfuse_downsample(net) == 0


def test_fuse_order_with_layernorm_cf():
    net = R.MiniBackbone()
    # fuse_downsample first: fuse_layernorm_cf counts the unpaired norms (stem.1, norm_out) and overwrites nothing
    assert unn.fuse_downsample(net) == 2
    assert unn.fuse_layernorm_cf(net) == 2
    want = {"stem.0": "_FusedStem", "stem.1": "_FusedLayerNormCF", "down.0": "_FusedDown", "down.1": "_FusedDown", "norm_out": "_FusedLayerNormCF"}
    assert _forwards(net) == want
    # unfuse_downsample removes only its own forwards; the paired norm is then free again
    assert unn.unfuse_downsample(net) == 2
    assert _forwards(net) == {"stem.1": "_FusedLayerNormCF", "norm_out": "_FusedLayerNormCF"}
    assert unn.fuse_layernorm_cf(net) == 3
    # the other way round: fuse_downsample takes the paired norm over
    assert unn.fuse_downsample(net) == 2 and _forwards(net) == want
    assert unn.unfuse_layernorm_cf(net) == 2
    assert _forwards(net) == {"stem.0": "_FusedStem", "down.0": "_FusedDown", "down.1": "_FusedDown"}
    assert unn.unfuse_downsample(net) == 2 and _forwards(net) == {}


def test_existing_counts_are_unchanged():
    net = R.MiniBackbone()
    assert unn.fuse_backbone(net) == (2, 2, 3)
    net = R.MiniBackbone()
    assert unn.fuse_model_down(net) == unn.fuse_model(R.MiniBackbone()) + (2,)
    assert unn.fuse_model_down(net)[-1] == 2
    assert unn.fuse_layernorm_cf(net) == 2                                 # down.0 belongs to the pair now


def test_what_is_not_a_downsample_layer_is_left_alone():
    nn = torch.nn
    cf = lambda C: R.lncf_ref.StandInNorm(C, data_format="channels_first")   # noqa: E731
    for seq in (nn.Sequential(cf(8), nn.Conv2d(8, 16, 2, 2, bias=False)), nn.Sequential(cf(8), nn.Conv2d(8, 16, 2, 2, padding=1)),
                nn.Sequential(cf(8), nn.Conv2d(8, 16, 3, 2)), nn.Sequential(cf(8), nn.Conv2d(8, 18, 2, 2)),
                nn.Sequential(cf(4), nn.Conv2d(8, 16, 2, 2)), nn.Sequential(cf(8), nn.Conv2d(8, 16, 2, 2), nn.ReLU()),
                nn.Sequential(nn.Conv2d(8, 16, 4, 4), cf(16)), nn.Sequential(nn.Conv2d(3, 16, 4, 4), nn.ReLU()),
                nn.Sequential(R.lncf_ref.StandInNorm(8), nn.Conv2d(8, 16, 2, 2)), nn.Sequential(cf(8), nn.Conv2d(8, 16, 2, 2, groups=2))):
        assert unn.fuse_downsample(seq) == 0 and _forwards(seq) == {}


def test_argument_errors_come_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    E = _lib.UnicornHipError
    x, lw, lb, w, b = torch.zeros(1, 8, 4, 4), torch.ones(8), torch.zeros(8), torch.zeros(16, 8, 2, 2), torch.zeros(16)
    bad = [((x[0], lw, lb, w, b), "is not \\(N, C, H, W\\)"), ((x, lw, lb, w[:, :, :1], b), "weight of shape"), ((x, lw, lb, w[:, :4], b), "weight of shape"),
           ((x, lw[:4], lb, w, b), "ln_weight of shape"), ((x, lw, lb, w, b[:4]), "bias of shape"), ((x[:, :, :1], lw, lb, w, b), "smaller than"),
           ((x[:, :, :, :1], lw, lb, w, b), "smaller than"), ((x, lw, lb, w[:6], b[:6]), "Co = 6"), ((x, lw, lb, w.double(), b), "dtypes"),
           ((x.double(), lw, lb, w, b), "dtypes"), ((x.long(), lw, lb, w, b), "dtypes"), ((x, lw, lb, w, b), "HIP device tensors"),
           ((x, lw, None, w, b), "ln_bias is not a tensor")]
    for args, what in bad:
        with pytest.raises(E, match="downsample_ln: .*" + what if "HIP device" not in what else what):
            ops.downsample_ln(*args)
    with pytest.raises(E, match="downsample_ln: eps"):
        ops.downsample_ln(x, lw, lb, w, b, eps=0.0)
    x6 = torch.zeros(1, 6, 4, 4)
    with pytest.raises(E, match="downsample_ln: C = 6"):
        ops.downsample_ln(x6, torch.ones(6), torch.ones(6), torch.zeros(16, 6, 2, 2), b)
    xs, ws, bs = torch.zeros(1, 3, 8, 8), torch.zeros(16, 3, 4, 4), torch.zeros(16)
    for args, what in [((xs, ws[:, :, :2, :2], bs), "weight of shape"), ((xs[:, :, :3], ws, bs), "smaller than"), ((xs, ws, bs[:4]), "bias of shape"),
                       ((torch.zeros(1, 5, 8, 8), torch.zeros(16, 5, 4, 4), bs), "Cin = 5"), ((xs, ws.half(), bs), "dtypes"),
                       ((xs, ws, bs), "HIP device tensors")]:
        with pytest.raises(E, match="stem_conv: .*" + what if "HIP device" not in what else what):
            ops.stem_conv(*args)


def test_weight_gradient_in_row_slices():
    """ops._wgrad_mm: fp32 maps of at least 2048 rows are multiplied in slices of 1024 rows and added in fp64 (with the rows left over): the
    value of gy.t() @ A, nearer to fp64 than the single mm's bound of M terms; short, half and fp64 maps are the single mm"""
    g = torch.Generator().manual_seed(2)
    gy, A = torch.randn(5000, 8, generator=g), torch.randn(5000, 12, generator=g)
    ref = gy.double().t() @ A.double()
    got = ops._wgrad_mm(gy, A)
    assert got.dtype == torch.float32 and tuple(got.shape) == (8, 12)
    assert R.rel_err(got, ref) <= 1024 * 2.0 ** -24                               # the worst case of a 1024-term fp32 sum, relative to max |ref|
    for a, b in ((gy[:2047], A[:2047]), (gy.double(), A.double()), (gy.bfloat16(), A.bfloat16())):
        assert torch.equal(ops._wgrad_mm(a, b), a.t() @ b)
