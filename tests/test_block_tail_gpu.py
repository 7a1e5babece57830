"""The differentiable ConvNeXt block tail on the GPU (ops.block_tail, csrc/block_tail.hip, unicorn_amd.nn.fuse_block_tail): the fixtures written
from the reference's own Block in fp64 (1e-12) and fp32 (4 x the reference's own fp32 deviation) with residual and grad_out in both layouts,
gradcheck, fp16 / bf16 y, bitwise reproducibility, the need flags with the variant trace, a dropped sample that holds Inf, larger shapes against
the eager lines, what autograd keeps, a fused stand-in block against the unfused one (fp64, and fp32 under autocast) and a stand-in stage
that stays channels-last under FusedAdamWEMA."""
import copy
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

import block_tail_ref as R  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
CL, NCHW = torch.channels_last, torch.contiguous_format
LAYOUTS = [(CL, CL), (CL, NCHW), (NCHW, CL), (NCHW, NCHW)]
LAYOUT_IDS = ["res_cl-g_cl", "res_cl-g_nchw", "res_nchw-g_cl", "res_nchw-g_nchw"]


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def run_op(ins, dtype, layouts=(CL, CL), y_dtype=None, need=(True, True, True)):
    """ops.block_tail + backward on the device -> {out, g_residual, g_y, g_gamma} (None where not needed or absent).  The gradient that the
    residual receives must be grad_out itself: the same memory, no copy."""
    from unicorn_amd.ops import block_tail
    y, res, gamma, scale, g = (None if t is None else t.detach() for t in ins)
    y = y.to(DEV, y_dtype or dtype, copy=True).requires_grad_(need[0])              # copies: the inputs may be shared between tests
    res = res.to(DEV, dtype, copy=True).contiguous(memory_format=layouts[0]).requires_grad_(need[1])
    gamma = None if gamma is None else gamma.to(DEV, dtype, copy=True).requires_grad_(need[2])
    scale = None if scale is None else scale.to(DEV, dtype)
    g = g.to(DEV, dtype).contiguous(memory_format=layouts[1])
    seen = []
    if need[1]:
        res.register_hook(seen.append)
    out = block_tail(y, res, gamma, scale)
    assert out.dtype == dtype and out.shape == res.shape and out.is_contiguous(memory_format=CL)
    out.backward(g)
    torch.cuda.synchronize()
    if need[1]:
        assert len(seen) == 1 and seen[0].data_ptr() == g.data_ptr() and seen[0].stride() == g.stride()
    if need[0]:
        assert y.grad.dtype == y.dtype and y.grad.is_contiguous() and y.grad.shape == y.shape
    return {"out": out.detach(), "g_residual": res.grad, "g_y": y.grad, "g_gamma": None if gamma is None else gamma.grad}


def fixture_inputs(c):
    return [torch.from_numpy(c[n]) if n in c else None for n in R.INPUTS]


@pytest.mark.parametrize("layouts", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp64_matches_the_fixture(L, tag, layouts):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float64, layouts)
    for n in R.RESULTS:
        if n not in c:
            assert got[n] is None
            continue
        err = R.rel_err(got[n], torch.from_numpy(c[n]))
        print("%s fp64 %-10s err %.3e" % (tag, n, err))
        assert got[n].shape == c[n].shape and err <= 1e-12, (n, err)


@pytest.mark.parametrize("layouts", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp32_within_four_times_the_reference_fp32_deviation(L, tag, layouts):
    """the yardstick of a result that is a copy of grad_out is 0: that result is held to the exact bits"""
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float32, layouts)
    bad = {}
    for n in R.RESULTS:
        if n not in c:
            continue
        err, bound = R.rel_err(got[n], torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
        print("%s fp32 %-10s err %.3e  bound %.3e" % (tag, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


@pytest.mark.parametrize("layouts", [(CL, CL), (NCHW, NCHW)], ids=["cl", "nchw"])
@pytest.mark.parametrize("tag", ["small", "nogamma"])
def test_gradcheck_fp64(L, tag, layouts):
    from unicorn_amd.ops import block_tail
    y, res, gamma, scale, _ = R.draw(tag, 7)
    leaves = [y.to(DEV, torch.float64).requires_grad_(True), res.to(DEV, torch.float64).contiguous(memory_format=layouts[0]).requires_grad_(True)]
    if gamma is not None:
        leaves.append(gamma.to(DEV, torch.float64).requires_grad_(True))
    sc = None if scale is None else scale.to(DEV, torch.float64)
    fn = (lambda a, b, g: block_tail(a, b, g, sc)) if gamma is not None else (lambda a, b: block_tail(a, b, None, sc))
    assert torch.autograd.gradcheck(fn, leaves, nondet_tol=0.0)


# ------------------------------------------------------------------------------------------------ half y
@pytest.mark.parametrize("layouts", [(CL, CL), (NCHW, NCHW)], ids=["cl", "nchw"])
@pytest.mark.parametrize("half,ulp", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c96", "c100"])
def test_half_y(L, tag, half, ulp, layouts):
    """y in fp16 / bf16 next to fp32 tensors (what pwconv2 hands over under autocast), against the restatement in fp64 on the ROUNDED y.  out
    and g_gamma are fp32 results of fp32 arithmetic: 4 x the deviation of the same restatement in fp32 on the CPU.  g_y is that fp32 result
    rounded once to the dtype of y: one rounding of that dtype relative to max|ref| (2^-11 fp16, 2^-8 bf16) on top of the fp32 bound.
    c96 has C % 8 == 0 (8 channels per lane in the channels-last path), c100 has not (4 per lane)."""
    ins = fixture_inputs(R.load_case(tag))
    ins[0] = ins[0].to(half).float()
    ref = R.value_and_grads(*ins, dtype=torch.float64)
    f32 = R.value_and_grads(*ins, dtype=torch.float32)
    got = run_op(ins, torch.float32, layouts, y_dtype=half)
    assert got["g_y"].dtype == half
    bad = {}
    for n in ("out", "g_y", "g_gamma"):
        err = R.rel_err(got[n], ref[n])
        bound = 4 * R.rel_err(f32[n], ref[n]) + (ulp if n == "g_y" else 0.0)
        print("%s %s %-8s err %.3e  bound %.3e" % (tag, half, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad
    assert torch.equal(got["g_residual"].cpu(), ins[4])


def test_half_residual_is_promoted_like_the_eager_lines(L):
    from unicorn_amd.ops import block_tail
    y, res, gamma, scale, g = (t.to(DEV) for t in R.draw("c96", 5))
    yh, rh = y.half().requires_grad_(True), res.half().requires_grad_(True)
    out = block_tail(yh, rh, gamma, scale)
    eager = R.forward(yh, rh, gamma, scale)
    assert out.dtype == eager.dtype == torch.float32
    ref = run_op([yh.detach().float(), rh.detach().float(), gamma, scale, g], torch.float32)
    assert torch.equal(out, ref["out"])
    out.backward(g)
    assert rh.grad.dtype == torch.float16 and torch.equal(rh.grad, g.half()) and yh.grad.dtype == torch.float16


# ------------------------------------------------------------------------------------------------ reproducibility, need flags, dropped samples
BIG = (2, 192, 50, 80)
STRADDLE = (3, 8, 300, 301)


@pytest.mark.parametrize("layouts", [(CL, CL), (NCHW, NCHW)], ids=["cl", "nchw"])
@pytest.mark.parametrize("shape", [R.CASES["c96"], BIG])
def test_two_runs_are_bitwise_equal(L, shape, layouts):
    ins = R.draw("plain", 11, shape, scale=(1 / 0.7,) * shape[0])
    a, b = run_op(ins, torch.float32, layouts), run_op(ins, torch.float32, layouts)
    for n in R.RESULTS:
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize("layouts", [(CL, CL), (NCHW, NCHW)], ids=["cl", "nchw"])
@pytest.mark.parametrize("need_y,need_g", [(True, False), (False, True)])
def test_need_flags(L, need_y, need_g, layouts):
    """only what autograd asks for is computed: the other gradient is None, the wanted one keeps its bits, and without the gamma gradient the
    reduce launch is gone"""
    ins = fixture_inputs(R.load_case("c96"))
    full = run_op(ins, torch.float32, layouts)
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        got = run_op(ins, torch.float32, layouts, need=(need_y, True, need_g))
    finally:
        lib.uni_variant_trace(0)
    tags = {t: v for t, v in vc.read_trace(lib).items() if t.startswith("block_tail ")}
    for n, k in (("g_y", need_y), ("g_gamma", need_g)):
        if k:
            assert torch.equal(got[n], full[n]), n
        else:
            assert got[n] is None, n
    assert torch.equal(got["out"], full["out"]) and torch.equal(got["g_residual"], full["g_residual"])
    kind = "nchw" if layouts[0] is NCHW else "cl"
    count = lambda key: sum(v for t, v in tags.items() if t.startswith("block_tail " + key))        # noqa: E731
    assert count("fwd_" + kind) == 1 and count("bwd_" + kind) == 1 and count("reduce") == int(need_g) and sum(tags.values()) == 2 + int(need_g), tags
    assert ("gy=%d gg=%d" % (need_y, need_g)) in [t for t in tags if t.startswith("block_tail bwd")][0], tags


def test_residual_alone_needs_no_launch(L):
    ins = fixture_inputs(R.load_case("small"))
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        got = run_op(ins, torch.float32, need=(False, True, False))
    finally:
        lib.uni_variant_trace(0)
    tags = {t: v for t, v in vc.read_trace(lib).items() if t.startswith("block_tail ")}
    assert sum(tags.values()) == 1 and got["g_y"] is None and got["g_gamma"] is None, tags


@pytest.mark.parametrize("layouts", [(CL, CL), (NCHW, NCHW)], ids=["cl", "nchw"])
@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_dropped_sample_is_not_read(L, bad, layouts):
    """The one deliberate difference to the eager lines (0 * Inf = NaN there): a sample with scale 0 whose y holds Inf / NaN gives out = residual,
    grad_y = 0 and adds exactly 0 to grad_gamma: every result has the bits of the run on the finite y."""
    ins = fixture_inputs(R.load_case("c100"))
    assert float(ins[3][1]) == 0.0
    clean = run_op(ins, torch.float32, layouts)
    ins[0] = ins[0].clone()
    ins[0][1] = bad
    got = run_op(ins, torch.float32, layouts)
    eager = R.value_and_grads(*ins)
    assert not torch.isfinite(eager["g_gamma"]).all() and not torch.isfinite(eager["out"][1]).any()
    for n in R.RESULTS:
        assert torch.isfinite(got[n]).all() and torch.equal(got[n], clean[n]), n
    assert not got["g_y"][1].any() and torch.equal(got["out"][1].cpu(), ins[1][1])


# ------------------------------------------------------------------------------------------------ larger shapes against the eager lines
@functools.lru_cache(maxsize=None)
def large_case(shape, scale):
    """inputs on the device, the eager lines there in fp64, and their own deviation in fp32 (computed once per shape, shared, never modified)"""
    ins = [None if t is None else t.to(DEV) for t in R.draw("plain", sum(shape), shape, scale=scale)]
    ref = R.value_and_grads(*ins, dtype=torch.float64)
    f32 = R.value_and_grads(*ins, dtype=torch.float32)
    return ins, ref, {n: R.rel_err(f32[n], ref[n]) for n in R.RESULTS}


@pytest.mark.parametrize("layouts", [(CL, CL), (NCHW, NCHW)], ids=["cl", "nchw"])
@pytest.mark.parametrize("shape,scale", [(BIG, (1 / 0.7, 1 / 0.7)), (STRADDLE, (1 / 0.7, 0.0, 1 / 0.7))], ids=["c192", "straddle"])
def test_larger_shapes_against_the_eager_lines(L, shape, scale, layouts):
    """A block of the channels-last kernels takes PP = 512 / (C / 4) pixels at once and a contiguous range of pixels, at most 1024 blocks; the
    NCHW kernels walk tiles of 64 pixels x 64 channels, at most 1024 blocks along the pixels.
      (2, 192, 50, 80)   PP = 10, 800 blocks of one step each, 800 rows of grad_gamma partials; 126 tiles in three channel tiles
      (3, 8, 300, 301)   PP = 256, 1059 steps: 530 blocks of two steps whose pixel ranges straddle the image boundaries (H W = 90300 is no
                         multiple of 512), the middle image dropped; 1411 tiles per image: blocks take a fifth tile, the last tile of an
                         image has 60 pixels
    fp32 bound: 4 x the distance of the eager fp32 lines on the same device from their fp64 run (g_residual: a copy, exact); fp64: 1e-12."""
    ins, ref, dev = large_case(shape, scale)
    got = run_op(ins, torch.float32, layouts)
    got64 = run_op(ins, torch.float64, layouts)
    bad = {}
    for n in R.RESULTS:
        err, bound, err64 = R.rel_err(got[n], ref[n]), 4 * dev[n], R.rel_err(got64[n], ref[n])
        print("%s %-10s fp32 err %.3e bound %.3e   fp64 err %.3e" % (shape, n, err, bound, err64))
        if not (err <= bound and err64 <= 1e-12):
            bad[n] = (err, bound, err64)
    assert not bad, bad


def test_autograd_keeps_y_gamma_scale_and_never_out(L):
    from unicorn_amd.ops import block_tail
    N, C, H, W = R.CASES["c100"]
    y, res, gamma, scale, _ = (t.to(DEV) for t in fixture_inputs(R.load_case("c100")))
    y.requires_grad_(True), res.requires_grad_(True), gamma.requires_grad_(True)
    out = block_tail(y, res, gamma, scale.view(N, 1, 1, 1))
    saved = out.grad_fn.saved_tensors
    assert sorted(t.numel() for t in saved) == sorted([N * H * W * C, C, N])
    ptrs = {t.data_ptr() for t in saved}
    assert y.data_ptr() in ptrs and gamma.data_ptr() in ptrs and out.data_ptr() not in ptrs and res.data_ptr() not in ptrs


def test_other_strides_are_converted_once(L):
    from unicorn_amd.ops import block_tail
    ins = fixture_inputs(R.load_case("c96"))
    ref = run_op(ins, torch.float32)
    y, res, gamma, scale, g = (t.to(DEV) for t in ins)
    wide = torch.zeros(res.shape[0], res.shape[1], res.shape[2], res.shape[3] + 3, device=DEV)
    wide[..., :-3] = res
    res_s = wide[..., :-3]                                           # neither NCHW-contiguous nor channels-last
    y_s = y.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)     # (N, H, W, C) but not contiguous
    assert not res_s.is_contiguous() and not res_s.is_contiguous(memory_format=CL) and not y_s.is_contiguous()
    out = block_tail(y_s, res_s, gamma, scale)
    assert out.is_contiguous(memory_format=CL) and torch.equal(out, ref["out"])


def test_empty_batch(L):
    from unicorn_amd.ops import block_tail
    out = block_tail(torch.zeros(0, 3, 3, 8, device=DEV), torch.zeros(0, 8, 3, 3, device=DEV), torch.ones(8, device=DEV), torch.ones(0, device=DEV))
    assert tuple(out.shape) == (0, 8, 3, 3)


# ------------------------------------------------------------------------------------------------ the drop-in on a stand-in block
def _block(C=16, seed=5):
    torch.manual_seed(seed)
    blk = R.StandInBlock(C, drop_path=0.5)
    with torch.no_grad():
        blk.dwconv.bias.normal_(0, 0.1), blk.norm.weight.normal_(1, 0.1), blk.norm.bias.normal_(0, 0.1)
    return blk


SEED = 3


def _run_block(proto, x, t, dtype, fuse, autocast=False):
    """one seeded training forward + backward of a copy of `proto` -> out, x.grad, the parameter gradients"""
    from unicorn_amd.nn import fuse_convnext
    net = copy.deepcopy(proto).to(DEV, dtype).train()
    if fuse:
        assert fuse_convnext(net) == (1, 1)
    xi = x.to(DEV, dtype).requires_grad_(True)
    torch.manual_seed(SEED)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = net(xi)
    (out * t.to(DEV, dtype)).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach(), "x.grad": xi.grad}
    res.update({n: p.grad for n, p in net.named_parameters()})
    return res


def _dropped(out, x):
    return [bool(torch.equal(out[n].cpu().double(), x[n].double())) for n in range(x.shape[0])]


def test_fused_block_against_the_unfused_block_fp64(L):
    """fuse_convnext against the unfused stand-in block with a seeded DropPath(0.5), N = 4, in fp64: output, input gradient and every
    parameter gradient agree to 1e-12 of the largest value (inside the bound of the fused-block comparison of tests/test_dwln_train_gpu.py, which
    is 4 x an fp32 deviation), and the same samples are dropped: the mask is drawn in fp32 by both, as timm draws it for an fp32 block."""
    proto = _block()
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(4, 16, 6, 7, generator=g), torch.randn(4, 16, 6, 7, generator=g)
    torch.manual_seed(SEED)
    mask = torch.empty((4, 1, 1, 1), dtype=torch.float32, device=DEV).bernoulli_(0.5).flatten().tolist()
    assert 0.0 in mask and 1.0 in mask, mask
    fused, plain = _run_block(proto, x, t, torch.float64, True), _run_block(proto, x, t, torch.float64, False)
    assert _dropped(fused["out"], x) == _dropped(plain["out"], x) == [m == 0.0 for m in mask]
    assert fused["out"].is_contiguous(memory_format=CL)
    for n in plain:
        err = R.rel_err(fused[n], plain[n])
        print("%-16s fused vs unfused %.3e" % (n, err))
        assert err <= 1e-12, (n, err)


def test_fused_block_against_the_unfused_block_under_autocast(L):
    """The same under torch.autocast("cuda", dtype=torch.float16) with fp32 parameters.  The two blocks round differently by design (the unfused
    depthwise convolution runs in fp16 there, ops.dwconv7_ln in fp32), so they are not compared bit for bit: each is compared with the unfused
    block in fp64 without autocast on the same mask, and the fused block may be at most 4 x as far from it as the unfused autocast block is,
    per quantity.  No figure comes from the kernels."""
    proto = _block()
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(4, 16, 6, 7, generator=g), torch.randn(4, 16, 6, 7, generator=g)
    exact = _run_block(proto, x, t, torch.float64, False)
    plain = _run_block(proto, x, t, torch.float32, False, autocast=True)
    fused = _run_block(proto, x, t, torch.float32, True, autocast=True)
    assert fused["out"].dtype == plain["out"].dtype == torch.float32 and fused["out"].is_contiguous(memory_format=CL)
    assert _dropped(fused["out"], x) == _dropped(plain["out"], x) == _dropped(exact["out"], x)
    bad = {}
    for n in exact:
        err, bound = R.rel_err(fused[n], exact[n]), 4 * R.rel_err(plain[n], exact[n])
        print("%-16s fused %.3e  bound %.3e" % (n, err, bound))
        assert fused[n].dtype == plain[n].dtype
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_stand_in_stage_stays_channels_last_and_trains(L):
    """a 2x2 stride-2 convolution and two fused blocks: every block output is channels-last memory, the second block's dwconv (ops.dwconv7_ln)
    receives a tensor that is already contiguous in channels-last, and one FusedAdamWEMA step changes gamma"""
    from unicorn_amd import optim
    from unicorn_amd.nn import fuse_convnext
    torch.manual_seed(9)
    C = 16
    net = nn.Sequential(nn.Conv2d(8, C, kernel_size=2, stride=2), R.StandInBlock(C, drop_path=0.5), R.StandInBlock(C)).to(DEV).train()
    assert fuse_convnext(net) == (2, 2)
    outs, ins = [], []
    hooks = [net[1].register_forward_hook(lambda m, i, o: outs.append(o)), net[2].register_forward_hook(lambda m, i, o: outs.append(o)),
             net[2].dwconv.register_forward_pre_hook(lambda m, i: ins.append(i[0]))]
    ema = copy.deepcopy(net).eval()
    opt = optim.FusedAdamWEMA(net, ema, lr=1e-2, weight_decay=5e-4, ema_decay=0.9998)
    before = [net[1].gamma.detach().clone(), net[2].gamma.detach().clone()]
    opt.zero_grad()
    x = torch.randn(4, 8, 12, 14, device=DEV)
    out = net(x)
    (out * torch.randn_like(out)).sum().backward()
    opt.step()
    torch.cuda.synchronize()
    for h in hooks:
        h.remove()
    assert len(outs) == 2 and all(o.is_contiguous(memory_format=CL) and o.dtype == torch.float32 for o in outs)
    assert len(ins) == 1 and ins[0].is_contiguous(memory_format=CL) and ins[0].data_ptr() == outs[0].data_ptr()
    assert out.data_ptr() == outs[1].data_ptr()
    for b, blk in zip(before, (net[1], net[2])):
        assert torch.isfinite(blk.gamma).all() and not torch.equal(blk.gamma.detach(), b)
