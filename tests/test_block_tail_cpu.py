"""CPU half of the differentiable ConvNeXt block tail (ops.block_tail, unicorn_amd.nn.fuse_block_tail / fuse_convnext): the restatement of
tests/block_tail_ref.py against the fixtures written from the reference's own Block, the argument errors (raised before any device work),
and the fuse / unfuse drop-in on a stand-in block with a stand-in DropPath."""
import copy

import pytest
import torch
import torch.nn as nn

import block_tail_ref as R


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_matches_the_fixture(tag):
    c = R.load_case(tag)
    assert tuple(c["shape"]) == R.CASES[tag]
    drawn = R.draw(tag, int(c["seed"]))
    for n, t in zip(R.INPUTS, drawn):                                   # the stored inputs are the draw
        if t is None:
            assert n not in c and tag == "nogamma"
        else:
            assert c[n].dtype.name == "float32" and torch.equal(torch.from_numpy(c[n]), t), n
    if drawn[3] is not None:
        assert all(float(v) == 0.0 or float(v) > 1.0 for v in drawn[3])
    got = R.value_and_grads(*drawn, dtype=torch.float64)
    assert sorted(got) == sorted(n for n in R.RESULTS if n in c)
    for n in got:
        ref = torch.from_numpy(c[n])
        assert ref.dtype == torch.float64 and got[n].shape == ref.shape
        assert R.rel_err(got[n], ref) <= 1e-12, n
        copied = n == "g_residual" or (n == "g_y" and tag == "nogamma")
        err = float(c[n + "_fp32_ref_err"])
        assert err == 0.0 if copied else 0 < err < 1e-6, (n, err)


def test_fixture_results_are_laid_out_as_documented():
    c = R.load_case("c100")
    N, C, H, W = R.CASES["c100"]
    assert c["y"].shape == c["g_y"].shape == (N, H, W, C) and c["gamma"].shape == c["g_gamma"].shape == (C,) and c["scale"].shape == (N,)
    assert c["residual"].shape == c["grad_out"].shape == c["out"].shape == c["g_residual"].shape == (N, C, H, W)
    assert not c["g_y"][1].any() and c["g_y"][0].any() and (c["out"][1] == c["residual"][1]).all()          # the middle image is dropped


def _args(C=8, N=2, dtype=torch.float32):
    return [torch.zeros(N, 3, 3, C, dtype=dtype), torch.zeros(N, C, 3, 3, dtype=dtype), torch.zeros(C, dtype=dtype), torch.ones(N, dtype=dtype)]


def test_argument_errors_are_raised_without_a_device():
    from unicorn_amd._lib import UnicornHipError
    from unicorn_amd.ops import block_tail
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        block_tail(*_args())
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        block_tail(*_args(dtype=torch.float64))
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        block_tail(*_args()[:2])
    for i, name in ((0, "y"), (1, "residual")):
        a = _args()
        a[i] = None
        with pytest.raises(UnicornHipError, match="%s is not a tensor" % name):
            block_tail(*a)
    for i, name in ((2, "gamma"), (3, "scale")):
        a = _args()
        a[i] = 1.0
        with pytest.raises(UnicornHipError, match="%s is not a tensor or None" % name):
            block_tail(*a)
    with pytest.raises(UnicornHipError, match="not \\(N, C, H, W\\)"):
        block_tail(torch.zeros(2, 3, 3, 8), torch.zeros(8, 3, 3))
    for bad in (torch.zeros(2, 8, 3, 3), torch.zeros(2, 3, 3, 4), torch.zeros(1, 3, 3, 8), torch.zeros(2, 3, 3)):
        with pytest.raises(UnicornHipError, match="y of shape .* is not \\(N, H, W, C\\)"):
            block_tail(bad, *_args()[1:])
    a = _args()
    a[2] = torch.zeros(4)
    with pytest.raises(UnicornHipError, match=r"gamma of shape \(4,\)"):
        block_tail(*a)
    for bad in (torch.ones(3), torch.ones(2, 1), torch.ones(2, 1, 1, 2)):
        a = _args()
        a[3] = bad
        with pytest.raises(UnicornHipError, match="scale of shape"):
            block_tail(*a)
    for C in (6, 2, 2052):
        with pytest.raises(UnicornHipError, match="C = %d is outside" % C):
            block_tail(*_args(C))
    with pytest.raises(UnicornHipError, match="non-empty map"):
        block_tail(torch.zeros(2, 0, 3, 8), torch.zeros(2, 8, 0, 3))
    a = _args()
    a[3].requires_grad_(True)
    with pytest.raises(UnicornHipError, match="scale requires a gradient"):
        block_tail(*a)
    for i, dt in ((0, torch.float64), (1, torch.float64), (2, torch.float16), (3, torch.float64), (0, torch.int32)):
        a = _args()
        a[i] = a[i].to(dt)
        with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
            block_tail(*a)
    a = _args(dtype=torch.float64)
    a[0] = a[0].half()
    with pytest.raises(UnicornHipError, match="dtypes .* unsupported"):
        block_tail(*a)


# ------------------------------------------------------------------------------------------------ fuse / unfuse on a stand-in block
DropPath, StandInBlock = R.DropPath, R.StandInBlock


def _model():
    torch.manual_seed(0)
    return nn.Sequential(StandInBlock(8), StandInBlock(8, drop_path=0.5), StandInBlock(8, gamma=False),
                         StandInBlock(8, pwconv2=False),                                        # no pwconv2
                         StandInBlock(8, dp=nn.Dropout(0.5)),                                   # an unknown drop_path module
                         StandInBlock(8, gamma=nn.Parameter(torch.ones(8, 1, 1))),              # gamma of the wrong shape
                         StandInBlock(8, dp=DropPath(1.0)))                                     # drop_prob outside [0, 1)


def test_fuse_counts_blocks_and_keeps_the_state_dict():
    from unicorn_amd.nn import _FusedBlockTail, _FusedDwConv, fuse_block_tail, fuse_convnext, unfuse_block_tail, unfuse_dwconv_ln
    m = _model()
    keys, names = list(m.state_dict()), [n for n, _ in m.named_modules()]
    assert fuse_block_tail(m) == 3 and fuse_block_tail(m) == 3                                  # idempotent
    assert list(m.state_dict()) == keys and [n for n, _ in m.named_modules()] == names
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in _model().named_parameters()]
    for i, blk in enumerate(m):
        assert isinstance(blk.__dict__.get("forward"), _FusedBlockTail) == (i < 3), i
        assert "forward" not in blk.dwconv.__dict__
    f = m[0].forward                                                                            # a plain object: no module, no closure
    assert not isinstance(f, nn.Module) and type(f).__call__.__closure__ is None and f.block is m[0]
    assert unfuse_block_tail(m) == 3 and unfuse_block_tail(m) == 0
    assert all("forward" not in blk.__dict__ for blk in m) and list(m.state_dict()) == keys
    # both fusions: the opening of every block with a 7x7 depthwise conv and a norm over C, the close of the first three
    assert fuse_convnext(m) == (7, 3) and fuse_convnext(m) == (7, 3)
    assert isinstance(m[1].dwconv.__dict__.get("forward"), _FusedDwConv) and isinstance(m[1].__dict__.get("forward"), _FusedBlockTail)
    assert list(m.state_dict()) == keys
    assert unfuse_block_tail(m) == 3 and unfuse_dwconv_ln(m) == 7
    assert all("forward" not in mod.__dict__ for mod in m.modules())


def test_cpu_and_eval_fall_back_to_the_unfused_block():
    from unicorn_amd.nn import fuse_convnext
    m, plain = _model(), _model()
    assert fuse_convnext(m) == (7, 3)
    x = torch.randn(4, 8, 5, 6, generator=torch.Generator().manual_seed(1))
    for mode in (True, False):
        m.train(mode), plain.train(mode)
        torch.manual_seed(3)
        a = m[:3](x)
        torch.manual_seed(3)
        b = plain[:3](x)
        assert torch.equal(a, b), mode
    xg = x.clone().requires_grad_(True)
    m.train()
    m[:3](xg).sum().backward()                  # the fallback is differentiable like the block it is
    assert xg.grad is not None and m[0].gamma.grad is not None


def test_deepcopy_of_a_fused_model_uses_its_own_parameters():
    from unicorn_amd.nn import _FusedBlockTail, fuse_block_tail
    m = _model()[:3]
    assert fuse_block_tail(m) == 3
    c = copy.deepcopy(m)
    for a, b in zip(c, m):
        f = a.__dict__["forward"]
        assert isinstance(f, _FusedBlockTail) and f.block is a and f.block is not b
    x = torch.randn(1, 8, 4, 4, generator=torch.Generator().manual_seed(2))
    m.eval(), c.eval()
    assert torch.equal(c(x), m(x))
    with torch.no_grad():
        c[0].gamma.mul_(2.0)
    assert not torch.equal(c(x), m(x))
    assert list(c.state_dict()) == list(m.state_dict())
