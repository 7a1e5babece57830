"""The recomputing pwconv1-GELU-pwconv2 operator without a GPU: the restatement (tests/pw_mlp_ref.py) against the fixtures written from the
reference's own Block, the fixtures themselves, what the fp32 yardstick of the kernel-level results can tell apart (a tanh GELU in place of the
erf one), the argument checks of ops.pw_mlp, and the drop-in unicorn_amd.nn.fuse_pw_mlp / fuse_backbone_mlp on CPU tensors: eligibility,
the fallback to the modules' own forwards, deepcopy, unfuse, state_dict."""
import copy
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import pw_mlp_ref as R


# ------------------------------------------------------------------------------------------------ fixtures and restatement
def test_fixture_files_are_the_cases_and_well_formed():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(R.GOLDEN, "pw_mlp_*.npz"))) == sorted("pw_mlp_%s.npz" % t for t in R.CASES)
    for tag, (nhw, C, Hd, Co) in R.CASES.items():
        assert os.path.getsize(os.path.join(R.GOLDEN, "pw_mlp_%s.npz" % tag)) <= 360 * 1024, tag
        c = R.load_case(tag)
        assert tuple(c["shape"]) == tuple(nhw) + (C, Hd, Co)
        shapes = {"t": nhw + (C,), "w1": (Hd, C), "b1": (Hd,), "w2": (Co, Hd), "b2": (Co,), "grad_out": nhw + (Co,),
                  "y": nhw + (Co,), "g_t": nhw + (C,), "g_w1": (Hd, C), "g_b1": (Hd,), "g_w2": (Co, Hd), "g_b2": (Co,)}
        for n in R.INPUTS:
            assert c[n].dtype == np.float32 and c[n].shape == shapes[n], (tag, n)
            # off any binary grid: the low mantissa bits are in use
            assert (np.abs(c[n]).view(np.uint32) & 0xFF).any(), (tag, n)
        for n in R.RESULTS:
            assert c[n].dtype == np.float64 and c[n].shape == shapes[n] and np.isfinite(c[n]).all(), (tag, n)
        for n in R.RESULTS + ("a", "grad_h"):
            assert 0 < float(c[n + "_fp32_ref_err"]) < 1e-6, (tag, n, c[n + "_fp32_ref_err"])
        assert not any(c[k].dtype.kind in "SUO" for k in c), "no text is stored"
        drawn = R.draw(tag, int(c["seed"]))
        for n, t in zip(R.INPUTS, drawn):
            assert np.array_equal(t.numpy(), c[n]), (tag, n)
    src = open(os.path.join(R.GOLDEN, "make_golden_pw_mlp.py")).read()
    assert "ref_bootstrap" in src and "blk.pwconv1(" in src and "blk.act(" in src and "blk.pwconv2(" in src


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_equals_the_fixture(tag):
    c = R.load_case(tag)
    got = R.value_and_grads(*(torch.from_numpy(c[n]) for n in R.INPUTS), dtype=torch.float64)
    for n in R.RESULTS:
        err = R.rel_err(got[n], torch.from_numpy(c[n]))
        assert got[n].shape == c[n].shape and err <= 1e-12, (n, err)
    # the closed forms the kernels use are what autograd gives
    maps = R.act_maps(got["h"], got["grad_a"])
    assert R.rel_err(maps["a"], got["a"]) <= 1e-14 and R.rel_err(maps["grad_h"], got["grad_h"]) <= 1e-13
    assert R.rel_err(maps["g_b1"], got["g_b1"]) <= 1e-13


def test_fp32_yardstick_of_the_kernel_level_results_tells_erf_from_tanh():
    """a, grad_h and grad_b1 from h and grad_a in fp32 against fp64 on the same (fp32) inputs: the yardstick is a few 1e-7, and a tanh GELU in
    place of the erf one moves every one of the three by more than 100 x the bound (4 x the yardstick) that the GPU tests apply"""
    for seed in (1, 2, 3):
        ins = R.draw("c24", seed)
        full = R.value_and_grads(*ins, dtype=torch.float64)
        h, ga = full["h"].float(), full["grad_a"].float()
        ref, f32, tanh = R.act_maps(h.double(), ga.double()), R.act_maps(h, ga), R.act_maps(h.double(), ga.double(), tanh=True)
        for n in ("a", "grad_h", "g_b1"):
            yard, moved = R.rel_err(f32[n], ref[n]), R.rel_err(tanh[n], ref[n])
            print("seed %d %-7s fp32 yardstick %.3e  tanh moves it by %.3e = %.0f x the bound" % (seed, n, yard, moved, moved / (4 * yard)))
            assert 0 < yard < 6e-7, (n, yard)
            assert moved > 100 * 4 * yard, (n, yard, moved)


# ------------------------------------------------------------------------------------------------ argument checks (before any device work)
def test_argument_checks():
    from unicorn_amd.ops import pw_mlp
    from unicorn_amd._lib import UnicornHipError
    t, w1, b1, w2, b2, _ = R.draw("small", 1)
    with pytest.raises(UnicornHipError, match="keep"):
        pw_mlp(t, w1, b1, w2, b2, keep="all")
    with pytest.raises(UnicornHipError, match="not a tensor"):
        pw_mlp(t, w1, None, w2, b2)
    with pytest.raises(UnicornHipError, match="do not fit"):
        pw_mlp(t, w1.t(), b1, w2, b2)
    with pytest.raises(UnicornHipError, match="do not fit"):
        pw_mlp(t, w1, b1, w2[:, :8], b2)
    with pytest.raises(UnicornHipError, match="b1 of shape"):
        pw_mlp(t, w1, b1[:8], w2, b2)
    with pytest.raises(UnicornHipError, match="b2 of shape"):
        pw_mlp(t, w1, b1, w2, b1)
    with pytest.raises(UnicornHipError, match="Hd = 6 is outside"):
        pw_mlp(t, w1[:6], b1[:6], w2[:, :6], b2)
    with pytest.raises(UnicornHipError, match="Co = 2 is outside"):
        pw_mlp(t, w1, b1, w2[:2], b2[:2])
    with pytest.raises(UnicornHipError, match="Hd = 8196 is outside"):
        pw_mlp(t, torch.zeros(8196, 4), torch.zeros(8196), torch.zeros(4, 8196), b2)
    with pytest.raises(UnicornHipError, match="dtypes"):
        pw_mlp(t, w1.double(), b1, w2, b2)
    with pytest.raises(UnicornHipError, match="dtypes"):
        pw_mlp(t.half(), w1.half(), b1.half(), w2.half(), b2.half())
    with pytest.raises(UnicornHipError, match="CPU tensor"):
        pw_mlp(t, w1, b1, w2, b2)


# ------------------------------------------------------------------------------------------------ the drop-in
def _net():
    torch.manual_seed(3)
    return R.MiniBackbone(16)


def test_fuse_backbone_mlp_counts_and_fuse_backbone_keeps_its_three_numbers():
    from unicorn_amd.nn import fuse_backbone, fuse_backbone_mlp, fuse_pw_mlp, unfuse_pw_mlp
    net = _net()
    keys = list(net.state_dict())
    names = [n for n, _ in net.named_modules()]
    assert fuse_backbone(net) == (2, 2, 3)
    assert fuse_backbone_mlp(net) == (2, 2, 3, 2)
    assert fuse_pw_mlp(net, keep="input") == 2                       # blocks fused earlier are counted
    assert net.block1.pwconv2.__dict__["forward"].keep == "input"
    assert list(net.state_dict()) == keys and [n for n, _ in net.named_modules()] == names
    assert unfuse_pw_mlp(net) == 2 and unfuse_pw_mlp(net) == 0
    for blk in (net.block1, net.block2):
        assert not any("forward" in m.__dict__ for m in (blk.pwconv1, blk.act, blk.pwconv2))
    assert fuse_backbone(net) == (2, 2, 3)
    with pytest.raises(RuntimeError, match="keep"):
        fuse_pw_mlp(net, keep="everything")


def test_eligibility():
    from unicorn_amd.nn import fuse_pw_mlp

    def foreign(x):
        return x

    def blocks():
        ok = R.StandInBlock(8)
        tanh = R.StandInBlock(8)
        tanh.act = nn.GELU(approximate="tanh")
        relu = R.StandInBlock(8)
        relu.act = nn.ReLU()
        nobias = R.StandInBlock(8)
        nobias.pwconv1 = nn.Linear(8, 32, bias=False)
        mismatch = R.StandInBlock(8)
        mismatch.pwconv2 = nn.Linear(16, 8)
        odd = R.StandInBlock(8)
        odd.pwconv1, odd.pwconv2 = nn.Linear(8, 30), nn.Linear(30, 8)
        wide = R.StandInBlock(8)
        wide.pwconv1, wide.pwconv2 = nn.Linear(8, 8196), nn.Linear(8196, 8)
        hooked = R.StandInBlock(8)
        hooked.act.forward = foreign
        other = R.StandInBlock(8, pwconv2=False)                     # no module called pwconv2
        conv = R.StandInBlock(8)
        conv.pwconv1 = nn.Conv2d(8, 32, 1)
        return dict(ok=ok, tanh=tanh, relu=relu, nobias=nobias, mismatch=mismatch, odd=odd, wide=wide, hooked=hooked, other=other, conv=conv)

    for name, blk in blocks().items():
        assert fuse_pw_mlp(blk) == int(name == "ok"), name
        if name == "hooked":
            assert blk.act.__dict__["forward"] is foreign
        elif name != "ok":
            assert not any("forward" in m.__dict__ for m in blk.modules()), name
    # Hd = 5 C and Co != C are inside the limits
    free = R.StandInBlock(8)
    free.pwconv1, free.pwconv2 = nn.Linear(8, 40), nn.Linear(40, 12)
    assert fuse_pw_mlp(free) == 1


@pytest.mark.parametrize("keep", ["hidden", "input"])
def test_fused_model_on_the_cpu_is_the_unfused_one_bit_for_bit(keep):
    """CPU tensors are not `active`: every fused module calls its own forward, in training and in eval mode, values and gradients alike"""
    from unicorn_amd.nn import fuse_backbone_mlp
    plain = _net()
    fused = copy.deepcopy(plain)
    assert fuse_backbone_mlp(fused, keep) == (2, 2, 3, 2)
    x = torch.randn(2, 3, 16, 24, generator=torch.Generator().manual_seed(2))
    for train in (True, False):
        plain.train(train), fused.train(train)
        plain.zero_grad(), fused.zero_grad()
        a, b = plain(x), fused(x)
        assert torch.equal(a, b)
        a.square().sum().backward(), b.square().sum().backward()
        for (n, p), (_, q) in zip(plain.named_parameters(), fused.named_parameters()):
            assert torch.equal(p.grad, q.grad), n


def test_deepcopy_uses_the_parameters_of_the_copy():
    from unicorn_amd.nn import _FusedPw, fuse_pw_mlp
    net = _net()
    assert fuse_pw_mlp(net, keep="input") == 2
    twin = copy.deepcopy(net)
    for a, b in ((net.block1, twin.block1), (net.block2, twin.block2)):
        for role, name in enumerate(("pwconv1", "act", "pwconv2")):
            f = getattr(b, name).__dict__["forward"]
            assert isinstance(f, _FusedPw) and f.role == role and f.keep == "input"
            assert f.pw1 is b.pwconv1 and f.act is b.act and f.pw2 is b.pwconv2
            assert f.pw1 is not a.pwconv1 and f.pw2.weight is not a.pwconv2.weight
    with torch.no_grad():
        twin.block1.pwconv2.bias.add_(1.0)
    x = torch.randn(1, 3, 8, 8, generator=torch.Generator().manual_seed(4))
    assert not torch.equal(net(x), twin(x))
