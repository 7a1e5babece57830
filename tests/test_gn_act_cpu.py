"""CPU half of the differentiable GroupNorm + activation (ops.group_norm_act, unicorn_amd.nn.fuse_groupnorm_act / fuse_model): the
restatement of tests/gn_act_ref.py against the fixtures written from the reference's own modules, the argument errors (raised before any
device work), the workspace size function against the plan listing, the fuse / unfuse drop-in on stand-in modules, and the size of the defect
that the `c96` case exists for."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gn_act_ref as R
import train_plans as P


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_matches_the_fixture(tag):
    c = R.load_case(tag)
    shape, G, act, eps = R.CASES[tag]
    assert tuple(c["shape"]) == shape and int(c["groups"]) == G and float(c["eps"]) == eps
    drawn = R.draw(tag, int(c["seed"]))
    for n, t in zip(R.INPUTS, drawn):                                   # the stored inputs are the draw
        assert c[n].dtype.name == "float32" and torch.equal(torch.from_numpy(c[n]), t), n
    got = R.value_and_grads(*drawn, G, act, eps, dtype=torch.float64)
    assert sorted(got) == sorted(R.RESULTS)
    for n in got:
        ref = torch.from_numpy(c[n])
        assert ref.dtype == torch.float64 and got[n].shape == ref.shape
        assert R.rel_err(got[n], ref) <= 1e-12, n
        assert 0 < float(c[n + "_fp32_ref_err"]) < (1e-2 if tag == "offset" else 1e-3), n
    if act == "relu":                                                   # no mask bit within reach of an fp32 rounding
        assert float(R.pre_activation(*drawn[:3], G, eps).abs().min()) >= 1e-5


def test_fixture_results_are_laid_out_as_documented():
    c = R.load_case("c100")
    (N, C, H, W), _, _, _ = R.CASES["c100"]
    assert c["x"].shape == c["grad_out"].shape == c["y"].shape == c["g_x"].shape == (N, C, H, W)
    assert c["weight"].shape == c["bias"].shape == c["g_weight"].shape == c["g_bias"].shape == (C,)
    assert sorted(c) == sorted(("shape", "seed", "groups", "eps") + R.INPUTS + R.RESULTS + tuple(n + "_fp32_ref_err" for n in R.RESULTS))
    x = R.load_case("offset")["x"]
    assert 99.9 < x.min() and x.max() < 100.1                           # the case that a one-pass variance fails


def _args(C=8, N=2, dtype=torch.float32):
    return [torch.zeros(N, C, 3, 3, dtype=dtype), 2, torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype)]


def test_argument_errors_are_raised_without_a_device():
    from unicorn_amd._lib import UnicornHipError
    from unicorn_amd.ops import group_norm_act
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        group_norm_act(*_args())
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        group_norm_act(*_args(dtype=torch.float64), act="none")
    for half in (torch.float16, torch.bfloat16):
        a = _args()
        a[0] = a[0].to(half)
        with pytest.raises(UnicornHipError, match="CPU tensor"):        # a half x next to fp32 parameters is a supported combination
            group_norm_act(*a, act="relu")
    for i, name in ((0, "x"), (2, "weight"), (3, "bias")):
        a = _args()
        a[i] = None
        with pytest.raises(UnicornHipError, match="%s is not a tensor" % name):
            group_norm_act(*a)
    for bad in (torch.zeros(8, 3, 3), torch.zeros(2, 8, 3, 3, 1)):
        with pytest.raises(UnicornHipError, match="not \\(N, C, H, W\\)"):
            group_norm_act(bad, *_args()[1:])
    for i, name in ((2, "weight"), (3, "bias")):
        for bad in (torch.zeros(4), torch.zeros(8, 1, 1)):
            a = _args()
            a[i] = bad
            with pytest.raises(UnicornHipError, match="%s of shape .* is not \\(8,\\)" % name):
                group_norm_act(*a)
    for C in (6, 2, 2052):
        with pytest.raises(UnicornHipError, match="C = %d is outside" % C):
            group_norm_act(*_args(C))
    with pytest.raises(UnicornHipError, match="non-empty map"):
        group_norm_act(torch.zeros(2, 8, 0, 3), *_args()[1:])
    for G in (0, -1, 3, 16, 2.0, True, None):
        a = _args()
        a[1] = G
        with pytest.raises(UnicornHipError, match="num_groups = .* is not an integer in \\[1, C\\] that divides C = 8"):
            group_norm_act(*a)
    for eps in (0.0, -1e-6, float("nan")):
        with pytest.raises(UnicornHipError, match="eps = .* is not positive"):
            group_norm_act(*_args(), eps=eps)
    for act in ("gelu", "SiLU", None, 3):
        with pytest.raises(UnicornHipError, match="act = .* is not one of 'none', 'relu', 'silu'"):
            group_norm_act(*_args(), act=act)
    for i, dt in ((0, torch.float64), (2, torch.float64), (3, torch.float16), (2, torch.float16), (0, torch.int32)):
        a = _args()
        a[i] = a[i].to(dt)
        with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
            group_norm_act(*a)
    a = _args(dtype=torch.float64)
    a[0] = a[0].half()
    with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
        group_norm_act(*a)


def test_different_devices_are_refused_without_a_device():
    """a tensor subclass that reports a HIP device index stands in for tensors of two devices: the check needs no device"""
    from unicorn_amd._lib import UnicornHipError
    from unicorn_amd.ops import group_norm_act

    class OtherDevice(torch.Tensor):
        """reports a HIP device without having one"""
        @staticmethod
        def __new__(cls, t, index):
            r = torch.Tensor._make_subclass(cls, t)
            r._index = index
            return r

        @property
        def is_cuda(self):
            return True

        @property
        def device(self):
            return torch.device("cuda", self._index)

    a = _args()
    with pytest.raises(UnicornHipError, match="different devices"):
        group_norm_act(OtherDevice(a[0], 0), 2, OtherDevice(a[2], 1), OtherDevice(a[3], 0))


def test_workspace_bytes_are_zero_outside_the_limits_and_the_plan_listing_inside():
    from unicorn_amd import _lib
    wsb = _lib.lib().uni_gn_act_train_workspace_bytes
    for bad in ((1, 4, 4, 6, 1), (1, 4, 4, 2052, 4), (1, 4, 4, 0, 1), (0, 4, 4, 8, 2), (1, 0, 4, 8, 2), (1, 4, 0, 8, 2), (1 << 11, 1 << 10, 1 << 10, 8, 2),
                (1, 4, 4, 8, 0), (1, 4, 4, 8, -1), (1, 4, 4, 8, 3), (1, 4, 4, 8, 16), (1, 4, 4, 96, 36)):
        assert wsb(*bad) == 0, bad
    plans, _ = P.plan_list()
    for C in (4, 96, 100, 1536, 2048):                                   # the listing states the bytes of the map (2, 9, 7) at G = 4
        for layout in ("cl", "nchw"):
            cls, extra = plans[("gn_act", layout, "f32", C)]
            assert extra["ws"] == wsb(2, 9, 7, C, 4) > 0, (C, layout)
    # maps of at most 16 x 512 pixels take units of 16 pixels: ceil(63 / 16) = 4 rows of partials per image.  [8 rows][2][C] rounded up to 64
    # elements, then the group sums [2 G][2], in fp32 elements
    assert wsb(2, 9, 7, 96, 16) == 4 * (8 * 2 * 96 + 2 * 16 * 2)
    assert wsb(2, 9, 7, 100, 5) == 4 * (8 * 2 * 100 + 2 * 5 * 2)
    assert wsb(1, 16, 32, 8, 2) == 4 * (32 * 2 * 8 + 1 * 2 * 2)                                # 512 pixels: 32 rows
    # two frames at stride 8: 32000 pixels take units of 64 (about 512 rows in all), 250 rows per image; 16 images of 16000 pixels units of 256,
    # 63 rows of the 64 allowed
    assert wsb(2, 100, 160, 192, 16) == 4 * (500 * 2 * 192 + 2 * 16 * 2)
    assert wsb(16, 100, 160, 8, 2) == 4 * (16 * 63 * 2 * 8 + 16 * 2 * 2)


def test_plan_listing_has_a_line_per_width_layout_and_type():
    plans, _ = P.plan_list()
    keys = [k for k in plans if k[0] == "gn_act"]
    assert len(keys) == 2 * 4 * len(P.SWEEP_C)
    # the lane mapping of pw_plan: 12 vectors of 8 fill 16 lanes (no power of two >= 8 fills better), 25 vectors of 4 fill 32
    assert plans[("gn_act", "cl", "f16", 96)][0] == "cl<f16,V=8> L=16" and plans[("gn_act", "cl", "f16", 100)][0] == "cl<f16,V=4> L=32"
    assert plans[("gn_act", "cl", "f32", 192)][0] == "cl<f32,V=4> L=16" and plans[("gn_act", "nchw", "bf16", 192)][0] == "nchw<bf16> CT=16"
    assert plans[("gn_act", "cl", "f32", 192)][1]["gy"] == 3 and plans[("gn_act", "nchw", "f64", 100)][1]["gy"] == 7


# ------------------------------------------------------------------------------------------------ fuse / unfuse on stand-in modules
def _model():
    torch.manual_seed(0)
    shared = nn.ReLU()
    return nn.Sequential(
        R.StandInBaseConv(3, 32),                                                                # 0  bn + act (SiLU)
        R.StandInBaseConv(32, 32, act="relu"),                                                   # 1  bn + act (ReLU)
        R.StandInBaseConv(32, 32, act="lrelu"),                                                  # 2  the norm alone, LeakyReLU stays eager
        R.mask_conv(32, 32),                                                                     # 3  Sequential: norm + ReLU
        R.proj_conv(32, 64),                                                                     # 4  Sequential: the norm ends it
        nn.Sequential(nn.Conv2d(64, 32, 1), nn.GroupNorm(16, 32), shared),                       # 5  the norm alone: `shared` occurs twice
        nn.Sequential(nn.Conv2d(32, 32, 1), nn.GroupNorm(16, 32), shared, nn.Conv2d(32, 6, 1)),  # 6  the norm alone
        nn.Sequential(nn.GroupNorm(3, 6), nn.SiLU()),                                            # 7  C % 4 != 0: left alone
        nn.Sequential(nn.Conv2d(6, 8, 1), nn.GroupNorm(2, 8, affine=False), nn.ReLU()),          # 8  no affine parameters: left alone
        nn.Sequential(nn.Conv2d(8, 8, 1), nn.GroupNorm(2, 8), nn.GELU(), nn.GroupNorm(4, 8)))    # 9  two norms, both alone


FUSED = {"0.bn": "silu", "1.bn": "relu", "2.bn": "none", "3.1": "relu", "4.1": "none", "5.1": "none", "6.1": "none", "9.1": "none", "9.3": "none"}
IDENTITY = ["0.act", "1.act", "3.2"]


def _fused(m):
    from unicorn_amd.nn import _FusedGroupNormAct, _gn_act_name
    norms = {n: _gn_act_name(mod.__dict__["forward"].act) for n, mod in m.named_modules()
             if isinstance(mod.__dict__.get("forward"), _FusedGroupNormAct) and mod.__dict__["forward"].role == 0}
    acts = [n for n, mod in m.named_modules() if isinstance(mod.__dict__.get("forward"), _FusedGroupNormAct) and mod.__dict__["forward"].role == 1]
    return norms, acts


def test_fuse_counts_modules_and_keeps_the_state_dict():
    from unicorn_amd.nn import _FusedGroupNormAct, fuse_groupnorm_act, fuse_model, unfuse_groupnorm_act
    m = _model()
    keys, names = list(m.state_dict()), [n for n, _ in m.named_modules()]
    assert fuse_groupnorm_act(m) == len(FUSED) and fuse_groupnorm_act(m) == len(FUSED)          # idempotent
    assert list(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == names
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in _model().named_parameters()]
    assert _fused(m) == (FUSED, IDENTITY)
    assert m[5][2] is m[6][2] and "forward" not in m[5][2].__dict__                             # the shared activation is not the identity
    assert "forward" not in m[2].act.__dict__ and "forward" not in m[7][0].__dict__ and "forward" not in m[8][1].__dict__
    f = m[0].bn.forward                                                                         # a plain object: no module, no closure
    assert not isinstance(f, nn.Module) and type(f).__call__.__closure__ is None and f.norm is m[0].bn and f.act is m[0].act
    assert type(f).__slots__ == ("norm", "act", "role")
    assert unfuse_groupnorm_act(m) == len(FUSED) and unfuse_groupnorm_act(m) == 0
    assert all("forward" not in mod.__dict__ for mod in m.modules()) and list(m.state_dict()) == keys
    assert fuse_model(m) == (0, 0, 0, 0, len(FUSED)) and fuse_model(m, keep="input") == (0, 0, 0, 0, len(FUSED))
    assert list(m.state_dict()) == keys
    # a forward of somebody else's on the activation: the norm alone
    assert unfuse_groupnorm_act(m) == len(FUSED)
    m[0].act.forward = lambda x: F.silu(x)
    assert fuse_groupnorm_act(m) == len(FUSED) and _fused(m)[0]["0.bn"] == "none" and not isinstance(m[0].act.forward, _FusedGroupNormAct)


def test_cpu_and_eval_fall_back_to_the_unfused_modules():
    from unicorn_amd.nn import fuse_groupnorm_act
    plain = _model()
    m = copy.deepcopy(plain)
    assert fuse_groupnorm_act(m) == len(FUSED)
    x = torch.randn(2, 3, 6, 5, generator=torch.Generator().manual_seed(1))
    for mode in (True, False):
        m.train(mode), plain.train(mode)
        assert torch.equal(m(x), plain(x)), mode
    assert torch.equal(m[4][1](torch.ones(2, 64)), plain[4][1](torch.ones(2, 64)))               # not 4-D: the module's own forward
    xg = x.clone().requires_grad_(True)
    m.train()
    m(xg).sum().backward()                      # the fallback is differentiable like the modules it is
    assert xg.grad is not None and m[0].bn.weight.grad is not None and m[3][1].bias.grad is not None


def test_deepcopy_of_a_fused_model_uses_its_own_parameters():
    from unicorn_amd.nn import _FusedGroupNormAct, fuse_groupnorm_act
    m = _model()[:2]
    assert fuse_groupnorm_act(m) == 2
    c = copy.deepcopy(m)
    f, fa = c[0].bn.__dict__["forward"], c[0].act.__dict__["forward"]
    assert isinstance(f, _FusedGroupNormAct) and f.norm is c[0].bn and f.act is c[0].act and f.norm is not m[0].bn
    assert isinstance(fa, _FusedGroupNormAct) and fa.role == 1 and fa.norm is c[0].bn and fa.act is c[0].act
    x = torch.randn(1, 3, 4, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(c(x), m(x))
    with torch.no_grad():
        c[0].bn.weight.mul_(2.0)
    assert not torch.equal(c(x), m(x))
    assert list(c.state_dict()) == list(m.state_dict())


# ------------------------------------------------------------------------------------------------ what the case `c96` can see
def _lookup_norm(x, weight, bias, G, eps, lookup):
    """GroupNorm + SiLU with the statistics of group lookup[c] applied to channel c"""
    N, C, H, W = x.shape
    xg = x.reshape(N, G, -1)
    mean, rstd = xg.mean(2), (xg.var(2, unbiased=False) + eps).rsqrt()
    z = (x - mean[:, lookup, None, None]) * rstd[:, lookup, None, None] * weight[:, None, None] + bias[:, None, None]
    return F.silu(z)


def test_a_vector_normalised_with_its_neighbours_statistics_is_far_outside_the_fp32_bound():
    """cpg = 6: the 4-channel vector of channels 4 .. 7 holds channels 6 and 7 of group 1.  A kernel that looks the statistics up once per
    vector normalises them with those of group 0; on the restatement that moves y and g_x by more than 100 x the bound of the fp32 GPU test."""
    c = R.load_case("c96")
    (N, C, H, W), G, act, eps = R.CASES["c96"]
    assert act == "silu" and C // G == 6
    x, w, b, g = (torch.from_numpy(c[n]).double() for n in R.INPUTS)
    right = torch.arange(C) // 6
    wrong = right.clone()
    wrong[4:8] = 0
    for lookup, defect in ((right, False), (wrong, True)):
        xl = x.clone().requires_grad_(True)
        y = _lookup_norm(xl, w, b, G, eps, lookup)
        y.backward(g)
        for n, got in (("y", y), ("g_x", xl.grad)):
            err, bound = R.rel_err(got, torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
            assert (err > 100 * bound) if defect else (err <= 1e-12), (n, defect, err, bound)
