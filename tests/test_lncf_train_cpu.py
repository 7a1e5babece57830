"""CPU half of the differentiable channels-first LayerNorm (ops.layernorm_cf, unicorn_amd.nn.fuse_layernorm_cf / fuse_backbone): the
restatement of tests/lncf_ref.py against the fixtures written from the reference's own LayerNorm class, the argument errors (raised before any
device work), and the fuse / unfuse drop-in on stand-in modules."""
import copy

import pytest
import torch
import torch.nn as nn

import lncf_ref as R


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_matches_the_fixture(tag):
    c = R.load_case(tag)
    assert tuple(c["shape"]) == R.CASES[tag]
    drawn = R.draw(tag, int(c["seed"]))
    for n, t in zip(R.INPUTS, drawn):                                   # the stored inputs are the draw
        assert c[n].dtype.name == "float32" and torch.equal(torch.from_numpy(c[n]), t), n
    got = R.value_and_grads(*drawn, dtype=torch.float64)
    assert sorted(got) == sorted(R.RESULTS)
    for n in got:
        ref = torch.from_numpy(c[n])
        assert ref.dtype == torch.float64 and got[n].shape == ref.shape
        assert R.rel_err(got[n], ref) <= 1e-12, n
        assert 0 < float(c[n + "_fp32_ref_err"]) < 1e-3, n


def test_fixture_results_are_laid_out_as_documented():
    c = R.load_case("c100")
    N, C, H, W = R.CASES["c100"]
    assert c["x"].shape == c["grad_out"].shape == c["y"].shape == c["g_x"].shape == (N, C, H, W)
    assert c["weight"].shape == c["bias"].shape == c["g_weight"].shape == c["g_bias"].shape == (C,)
    assert sorted(c) == sorted(("shape", "seed") + R.INPUTS + R.RESULTS + tuple(n + "_fp32_ref_err" for n in R.RESULTS))
    x = R.load_case("offset")["x"]
    assert 99.9 < x.min() and x.max() < 100.1                           # the case that a one-pass variance fails


def _args(C=8, N=2, dtype=torch.float32):
    return [torch.zeros(N, C, 3, 3, dtype=dtype), torch.ones(C, dtype=dtype), torch.zeros(C, dtype=dtype)]


def test_argument_errors_are_raised_without_a_device():
    from unicorn_amd._lib import UnicornHipError
    from unicorn_amd.ops import layernorm_cf
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        layernorm_cf(*_args())
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        layernorm_cf(*_args(dtype=torch.float64))
    for half in (torch.float16, torch.bfloat16):
        a = _args()
        a[0] = a[0].to(half)
        with pytest.raises(UnicornHipError, match="CPU tensor"):        # a half x next to fp32 parameters is a supported combination
            layernorm_cf(*a)
    for i, name in enumerate(("x", "weight", "bias")):
        a = _args()
        a[i] = None
        with pytest.raises(UnicornHipError, match="%s is not a tensor" % name):
            layernorm_cf(*a)
    for bad in (torch.zeros(8, 3, 3), torch.zeros(2, 8, 3, 3, 1)):
        with pytest.raises(UnicornHipError, match="not \\(N, C, H, W\\)"):
            layernorm_cf(bad, *_args()[1:])
    for i, name in ((1, "weight"), (2, "bias")):
        for bad in (torch.zeros(4), torch.zeros(8, 1, 1)):
            a = _args()
            a[i] = bad
            with pytest.raises(UnicornHipError, match="%s of shape .* is not \\(8,\\)" % name):
                layernorm_cf(*a)
    for C in (6, 2, 2052):
        with pytest.raises(UnicornHipError, match="C = %d is outside" % C):
            layernorm_cf(*_args(C))
    with pytest.raises(UnicornHipError, match="non-empty map"):
        layernorm_cf(torch.zeros(2, 8, 0, 3), *_args()[1:])
    for eps in (0.0, -1e-6, float("nan")):
        with pytest.raises(UnicornHipError, match="eps = .* is not positive"):
            layernorm_cf(*_args(), eps=eps)
    for i, dt in ((0, torch.float64), (1, torch.float64), (2, torch.float16), (1, torch.float16), (0, torch.int32)):
        a = _args()
        a[i] = a[i].to(dt)
        with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
            layernorm_cf(*a)
    a = _args(dtype=torch.float64)
    a[0] = a[0].half()
    with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
        layernorm_cf(*a)


def test_different_devices_are_refused_without_a_device():
    """a tensor subclass that reports a HIP device index stands in for tensors of two devices: the check needs no device"""
    from unicorn_amd._lib import UnicornHipError
    from unicorn_amd.ops import layernorm_cf

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
        layernorm_cf(OtherDevice(a[0], 0), OtherDevice(a[1], 1), OtherDevice(a[2], 0))


# ------------------------------------------------------------------------------------------------ fuse / unfuse on stand-in modules
def _model():
    torch.manual_seed(0)
    odd = R.StandInNorm(8, data_format="channels_first")
    odd.weight = nn.Parameter(torch.ones(8, 1, 1))                                          # weight of the wrong shape
    return nn.Sequential(nn.Conv2d(3, 8, kernel_size=2, stride=2),
                         R.StandInNorm(8, data_format="channels_first"),                    # qualifies
                         R.StandInBlock(8),                                                 # its norm is an nn.LayerNorm
                         R.StandInNorm(8, data_format="channels_first"),                    # qualifies
                         nn.Conv2d(8, 12, kernel_size=1),
                         R.StandInNorm(12, data_format="channels_first"),                   # qualifies
                         nn.Conv2d(12, 6, kernel_size=1),
                         R.StandInNorm(6, data_format="channels_first"),                    # C = 6
                         nn.Conv2d(6, 8, kernel_size=1),
                         odd,
                         nn.Sequential(R.StandInNorm(8, data_format="channels_last")))      # channels-last: normalises the last dimension


def test_fuse_counts_modules_and_keeps_the_state_dict():
    from unicorn_amd.nn import (_FusedLayerNormCF, fuse_backbone, fuse_convnext, fuse_layernorm_cf, unfuse_block_tail, unfuse_dwconv_ln,
                                unfuse_layernorm_cf)
    m = _model()
    keys, names = list(m.state_dict()), [n for n, _ in m.named_modules()]
    assert fuse_layernorm_cf(m) == 3 and fuse_layernorm_cf(m) == 3                              # idempotent
    assert list(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == names
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in _model().named_parameters()]
    fused = [n for n, mod in m.named_modules() if isinstance(mod.__dict__.get("forward"), _FusedLayerNormCF)]
    assert fused == ["1", "3", "5"], fused
    assert "forward" not in m[2].norm.__dict__ and "forward" not in m[10][0].__dict__
    f = m[1].forward                                                                            # a plain object: no module, no closure
    assert not isinstance(f, nn.Module) and type(f).__call__.__closure__ is None and f.norm is m[1] and type(f).__slots__ == ("norm",)
    assert unfuse_layernorm_cf(m) == 3 and unfuse_layernorm_cf(m) == 0
    assert all("forward" not in mod.__dict__ for mod in m.modules()) and list(m.state_dict()) == keys
    assert fuse_backbone(m) == (1, 1, 3) and fuse_backbone(m) == (1, 1, 3)
    assert list(m.state_dict()) == keys
    assert unfuse_layernorm_cf(m) == 3
    assert fuse_convnext(m) == (1, 1)                                                           # still the 2-tuple, and no norm with it
    assert not any(isinstance(mod.__dict__.get("forward"), _FusedLayerNormCF) for mod in m.modules())
    assert unfuse_block_tail(m) == 1 and unfuse_dwconv_ln(m) == 1
    assert all("forward" not in mod.__dict__ for mod in m.modules())


def test_cpu_and_eval_fall_back_to_the_unfused_modules():
    from unicorn_amd.nn import fuse_backbone
    m, plain = _model()[:6], _model()[:6]
    assert fuse_backbone(m) == (1, 1, 3)
    x = torch.randn(2, 3, 10, 12, generator=torch.Generator().manual_seed(1))
    for mode in (True, False):
        m.train(mode), plain.train(mode)
        assert torch.equal(m(x), plain(x)), mode
    xg = x.clone().requires_grad_(True)
    m.train()
    m(xg).sum().backward()                      # the fallback is differentiable like the module it is
    assert xg.grad is not None and m[1].weight.grad is not None and m[5].bias.grad is not None


def test_deepcopy_of_a_fused_model_uses_its_own_parameters():
    from unicorn_amd.nn import _FusedLayerNormCF, fuse_layernorm_cf
    m = _model()[:2]
    assert fuse_layernorm_cf(m) == 1
    c = copy.deepcopy(m)
    f = c[1].__dict__["forward"]
    assert isinstance(f, _FusedLayerNormCF) and f.norm is c[1] and f.norm is not m[1]
    x = torch.randn(1, 3, 4, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(c(x), m(x))
    with torch.no_grad():
        c[1].weight.mul_(2.0)
    assert not torch.equal(c(x), m(x))
    assert list(c.state_dict()) == list(m.state_dict())
