"""CPU half of the differentiable depthwise 7x7 + LayerNorm operator (ops.dwconv7_ln, unicorn_amd.nn.fuse_dwconv_ln): the restatement of
tests/dwln_train_ref.py against the fixtures written from the reference's own Block, the argument errors (raised before any device work),
and the fuse / unfuse drop-in on a stand-in block."""
import copy

import pytest
import torch
import torch.nn as nn

import dwln_train_ref as R


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_matches_the_fixture(tag):
    c = R.load_case(tag)
    B, C, H, W = R.CASES[tag]
    assert tuple(c["shape"]) == (B, C, H, W) and float(c["eps"]) == R.EPS
    drawn = R.draw(tag, int(c["seed"]))
    for n, t in zip(R.INPUTS, drawn):
        assert c[n].dtype.name == "float32" and torch.equal(torch.from_numpy(c[n]), t), n       # the stored inputs are the draw
    got = R.value_and_grads(*(t.double() for t in drawn))
    for n in R.RESULTS:
        ref = torch.from_numpy(c[n])
        assert ref.dtype == torch.float64 and got[n].shape == ref.shape
        assert R.rel_err(got[n], ref) <= 1e-12, n
        assert 0 < float(c[n + "_fp32_ref_err"]) < (2e-3 if tag == "offset" else 1e-6), n


def test_fixture_results_are_laid_out_as_documented():
    c = R.load_case("c100")
    B, C, H, W = R.CASES["c100"]
    assert c["y"].shape == (B, H, W, C) and c["gx"].shape == (B, C, H, W) and c["gw"].shape == (C, 1, 7, 7)
    assert c["gb"].shape == c["ggamma"].shape == c["gbeta"].shape == (C,) and c["grad_y"].shape == (B, H, W, C)


def _args(C=8, dtype=torch.float32):
    return [torch.zeros(1, C, 3, 3, dtype=dtype), torch.zeros(C, 1, 7, 7, dtype=dtype)] + [torch.zeros(C, dtype=dtype) for _ in range(3)]


def test_argument_errors_are_raised_without_a_device():
    from unicorn_amd._lib import UnicornHipError
    from unicorn_amd.ops import dwconv7_ln
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        dwconv7_ln(*_args())
    a = _args()
    a[3] = a[3].double()
    with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
        dwconv7_ln(*a)
    with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
        dwconv7_ln(*_args(dtype=torch.float16))
    for bad in (torch.zeros(8, 1, 3, 3), torch.zeros(8, 8, 7, 7), torch.zeros(16, 1, 7, 7)):
        a = _args()
        a[1] = bad
        with pytest.raises(UnicornHipError, match="not the depthwise 7x7 weight"):
            dwconv7_ln(*a)
    a = _args()
    a[4] = torch.zeros(4)
    with pytest.raises(UnicornHipError, match=r"ln_bias of shape \(4,\)"):
        dwconv7_ln(*a)
    for C in (6, 2, 2052):
        with pytest.raises(UnicornHipError, match="C = %d is outside" % C):
            dwconv7_ln(*_args(C))
    with pytest.raises(UnicornHipError, match="not \\(N, C, H, W\\)"):
        dwconv7_ln(torch.zeros(8, 3, 3), *_args()[1:])
    with pytest.raises(UnicornHipError, match="not a tensor"):
        dwconv7_ln(None, *_args()[1:])
    with pytest.raises(UnicornHipError, match="eps"):
        dwconv7_ln(*_args(), eps=0.0)


# ------------------------------------------------------------------------------------------------ fuse / unfuse on a stand-in block
class LastDimNorm(nn.Module):
    """a norm of the reference's kind: weight, bias, eps, data_format"""

    def __init__(self, C, data_format="channels_last"):
        super().__init__()
        self.weight, self.bias = nn.Parameter(torch.ones(C)), nn.Parameter(torch.zeros(C))
        self.eps, self.data_format, self.normalized_shape = 1e-6, data_format, (C,)

    def forward(self, x):
        return torch.nn.functional.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)


class StandInBlock(nn.Module):
    def __init__(self, C, norm=None, **conv):
        super().__init__()
        self.dwconv = nn.Conv2d(C, C, **dict(dict(kernel_size=7, padding=3, groups=C), **conv))
        self.norm = LastDimNorm(C) if norm is None else norm
        self.pw = nn.Linear(C, C)

    def forward(self, x):
        y = self.norm(self.dwconv(x).permute(0, 2, 3, 1))
        return x + self.pw(y).permute(0, 3, 1, 2)


def _model():
    torch.manual_seed(0)
    return nn.Sequential(StandInBlock(8), StandInBlock(8, norm=nn.LayerNorm(8, eps=1e-6)),
                         StandInBlock(8, kernel_size=3, padding=1),                             # not a 7x7
                         StandInBlock(8, groups=1),                                             # not depthwise
                         StandInBlock(8, norm=LastDimNorm(8, "channels_first")),                # not over the last dimension
                         StandInBlock(8, bias=False), StandInBlock(6))                          # no bias; C % 4 != 0


def test_fuse_counts_blocks_and_keeps_the_state_dict():
    from unicorn_amd.nn import _FusedDwConv, _FusedNorm, fuse_dwconv_ln, unfuse_dwconv_ln
    m = _model()
    keys, names = list(m.state_dict()), [n for n, _ in m.named_modules()]
    assert fuse_dwconv_ln(m) == 2 and fuse_dwconv_ln(m) == 2                                    # idempotent
    assert list(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == names
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in _model().named_parameters()]
    for i, blk in enumerate(m):
        fused = i < 2
        assert isinstance(blk.dwconv.__dict__.get("forward"), _FusedDwConv) == fused and isinstance(blk.norm.__dict__.get("forward"), _FusedNorm) == fused
    for f in (m[0].dwconv.forward, m[0].norm.forward):                                          # plain objects: no module, no closure
        assert not isinstance(f, nn.Module) and type(f).__call__.__closure__ is None and f.dwconv is m[0].dwconv and f.norm is m[0].norm
    assert unfuse_dwconv_ln(m) == 2 and unfuse_dwconv_ln(m) == 0
    for blk in m:
        assert "forward" not in blk.dwconv.__dict__ and "forward" not in blk.norm.__dict__
    assert list(m.state_dict()) == keys


def test_cpu_and_eval_fall_back_to_the_original_forwards():
    from unicorn_amd.nn import fuse_dwconv_ln
    m, plain = _model(), _model()
    assert fuse_dwconv_ln(m) == 2
    x = torch.randn(2, 8, 5, 6, generator=torch.Generator().manual_seed(1))
    for mode in (True, False):
        m.train(mode), plain.train(mode)
        assert torch.equal(m[:2](x), plain[:2](x))
    xg = x.clone().requires_grad_(True)
    m.train()
    m[:2](xg).sum().backward()                  # the fallback is differentiable like the module it is
    assert xg.grad is not None and m[0].dwconv.weight.grad is not None


def test_deepcopy_of_a_fused_model_uses_its_own_parameters():
    from unicorn_amd.nn import _FusedDwConv, fuse_dwconv_ln
    m = _model()[:2]
    fuse_dwconv_ln(m)
    c = copy.deepcopy(m)
    f = c[0].dwconv.__dict__["forward"]
    assert isinstance(f, _FusedDwConv) and f.dwconv is c[0].dwconv and f.norm is c[0].norm and f.dwconv is not m[0].dwconv
    assert c[0].norm.__dict__["forward"].norm is c[0].norm and c[1].dwconv.__dict__["forward"].norm is c[1].norm
    x = torch.randn(1, 8, 4, 4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(c(x), m(x))
    with torch.no_grad():
        c[0].dwconv.weight.mul_(2.0)
        c[0].norm.bias.add_(1.0)
    assert not torch.equal(c(x), m(x))
    assert list(c.state_dict()) == list(m.state_dict())
