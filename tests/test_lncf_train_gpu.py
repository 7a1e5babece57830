"""The differentiable channels-first LayerNorm on the GPU (ops.layernorm_cf, csrc/lncf_train.hip, unicorn_amd.nn.fuse_layernorm_cf): the fixtures
written from the reference's own LayerNorm class in fp64 (1e-12) and fp32 (4 x the reference's own fp32 deviation) in both memory layouts,
fp16 / bf16 x, a pixel without variance, maps with more pixel blocks than rows of partials, the need flags with the variant trace, what autograd
keeps, other strides, an empty batch, and a stand-in mini-backbone fused with fuse_backbone against the unfused one."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import lncf_ref as R  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
CL, NCHW = torch.channels_last, torch.contiguous_format
LAYOUTS = [CL, NCHW]
LAYOUT_IDS = ["cl", "nchw"]
NAMES = {"y": "y", "g_x": "x.grad", "g_weight": "weight.grad", "g_bias": "bias.grad"}


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def run_op(ins, dtype, layout=CL, x_dtype=None, need=(True, True, True), g_layout=None):
    """ops.layernorm_cf + backward on the device -> {y, g_x, g_weight, g_bias} (None where not needed); y and x.grad must come back in the
    memory layout of x, x.grad in its dtype"""
    from unicorn_amd.ops import layernorm_cf
    x, w, b, g = (t.detach() for t in ins)
    x = x.to(DEV, x_dtype or dtype, copy=True).contiguous(memory_format=layout).requires_grad_(need[0])     # copies: inputs may be shared
    w = w.to(DEV, dtype, copy=True).requires_grad_(need[1])
    b = b.to(DEV, dtype, copy=True).requires_grad_(need[2])
    g = g.to(DEV, dtype).contiguous(memory_format=g_layout or layout)
    y = layernorm_cf(x, w, b, R.EPS)
    assert y.dtype == dtype and y.shape == x.shape and y.is_contiguous(memory_format=layout)
    if any(need):
        y.backward(g)
    torch.cuda.synchronize()
    if need[0]:
        assert x.grad.dtype == x.dtype and x.grad.shape == x.shape and x.grad.is_contiguous(memory_format=layout)
    return {"y": y.detach(), "g_x": x.grad, "g_weight": w.grad, "g_bias": b.grad}


def fixture_inputs(c):
    return [torch.from_numpy(c[n]) for n in R.INPUTS]


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp64_matches_the_fixture(L, tag, layout):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float64, layout)
    bad = {}
    for n in R.RESULTS:
        err = R.rel_err(got[n], torch.from_numpy(c[n]))
        print("%s fp64 %-8s err %.3e" % (tag, n, err))
        if not (got[n].shape == c[n].shape and err <= 1e-12):
            bad[n] = err
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp32_within_four_times_the_reference_fp32_deviation(L, tag, layout):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float32, layout)
    bad = {}
    for n in R.RESULTS:
        err, bound = R.rel_err(got[n], torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
        print("%s fp32 %-8s err %.3e  bound %.3e" % (tag, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_grad_out_in_the_other_layout_is_converted_once(L):
    c = R.load_case("c96")
    ins = fixture_inputs(c)
    for layout, other in ((CL, NCHW), (NCHW, CL)):
        same, mixed = run_op(ins, torch.float32, layout), run_op(ins, torch.float32, layout, g_layout=other)
        for n in R.RESULTS:
            assert torch.equal(same[n], mixed[n]), n


# ------------------------------------------------------------------------------------------------ half x
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("half,ulp", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c96", "c100", "c1536"])
def test_half_x(L, tag, half, ulp, layout):
    """x in fp16 / bf16 next to fp32 parameters (what the stem convolution hands over under autocast), against the restatement in fp64 on the
    ROUNDED x.  y, weight.grad and bias.grad are fp32 results of fp32 arithmetic: the fp32 bound of the fixture.  x.grad is that fp32 result
    rounded once to the dtype of x: one rounding to nearest, at most half an ulp of the largest value (2^-11 fp16, 2^-8 bf16), on top of it.
    c96 and c1536 have C % 8 == 0 (8 channels per lane in the channels-last kernels), c100 has not (4 per lane)."""
    c = R.load_case(tag)
    ins = fixture_inputs(c)
    ins[0] = ins[0].to(half).float()
    ref = R.value_and_grads(*ins, dtype=torch.float64)
    got = run_op(ins, torch.float32, layout, x_dtype=half)
    assert got["g_x"].dtype == half and got["y"].dtype == torch.float32
    bad = {}
    for n in R.RESULTS:
        err = R.rel_err(got[n], ref[n])
        bound = 4 * float(c[n + "_fp32_ref_err"]) + (ulp if n == "g_x" else 0.0)
        print("%s %s %-8s err %.3e  bound %.3e" % (tag, half, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_under_autocast_dtype_and_layout_are_those_of_the_eager_module(L, layout):
    from unicorn_amd.ops import layernorm_cf
    x, w, b, _ = (t.to(DEV) for t in R.draw("c96", 5))
    x = x.half().contiguous(memory_format=layout)
    mod = R.StandInNorm(96, data_format="channels_first").to(DEV)
    with torch.no_grad():
        mod.weight.copy_(w), mod.bias.copy_(b)
    with torch.autocast("cuda", dtype=torch.float16):
        eager = mod(x)
        y = layernorm_cf(x, mod.weight, mod.bias, mod.eps)
    assert y.dtype == eager.dtype == torch.float32 and y.stride() == eager.stride() and y.is_contiguous(memory_format=layout)


# ------------------------------------------------------------------------------------------------ a pixel without variance
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_zero_variance_pixel(L, layout):
    """pixel 0 holds 0.5 in all 8 channels: the sums are exact, so x - mean is 0 there and y is bias bit for bit; rstd = 1 / sqrt(eps)"""
    x, w, b, g = R.draw("plain", 3, (1, 8, 2, 2))
    x[0, :, 0, 0] = 0.5
    ref = R.value_and_grads(x, w, b, g, dtype=torch.float64)
    got = run_op((x, w, b, g), torch.float32, layout)
    assert torch.equal(got["y"][0, :, 0, 0].cpu(), b)
    for n in R.RESULTS:
        assert torch.isfinite(got[n]).all(), n
    err, bound = R.rel_err(got["g_x"][0, :, 0, 0], ref["g_x"][0, :, 0, 0]), 4 * float(R.load_case("small")["g_x_fp32_ref_err"])
    print("zero-variance pixel g_x err %.3e bound %.3e" % (err, bound))
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ many pixels
MANY = (1, 8, 300, 300)          # 1407 tiles of 64 pixels: the NCHW blocks take a second tile
MANY_CL = (1, 4, 520, 520)       # one lane per pixel: 1057 groups of 256 pixels, the channels-last blocks take a second group


@functools.lru_cache(maxsize=None)
def large_case(shape):
    """inputs on the device, the restatement there in fp64, and its own deviation in fp32 (computed once per shape, shared, never modified)"""
    ins = [t.to(DEV) for t in R.draw("plain", sum(shape), shape)]
    ref = R.value_and_grads(*ins, dtype=torch.float64)
    f32 = R.value_and_grads(*ins, dtype=torch.float32)
    return ins, ref, {n: R.rel_err(f32[n], ref[n]) for n in R.RESULTS}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("shape", [MANY, MANY_CL], ids=["c8", "c4"])
def test_many_pixels_against_the_eager_lines(L, shape, layout):
    """more blocks' worth of pixels than the 1024 rows of partials, so a block loops.  fp32 bound: 4 x the distance of the eager fp32 lines on
    the same device from their fp64 run (the reference side); two calls are bit-equal."""
    ins, ref, dev = large_case(shape)
    got, again = run_op(ins, torch.float32, layout), run_op(ins, torch.float32, layout)
    bad = {}
    for n in R.RESULTS:
        err, bound = R.rel_err(got[n], ref[n]), 4 * dev[n]
        print("%s %-8s fp32 err %.3e bound %.3e" % (shape, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
        assert torch.equal(got[n], again[n]), n
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ need flags, saved tensors, strides, N = 0
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("need", [(True, False, False), (False, True, True), (False, True, False)], ids=["x", "weight+bias", "weight"])
def test_need_flags(L, need, layout):
    """only what autograd asks for is computed: the other gradients are None, the wanted ones keep their bits, and the launch of a skipped
    part is absent from the variant trace"""
    ins = fixture_inputs(R.load_case("c96"))
    full = run_op(ins, torch.float32, layout)
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        got = run_op(ins, torch.float32, layout, need=need)
    finally:
        lib.uni_variant_trace(0)
    tags = {t: v for t, v in vc.read_trace(lib).items() if t.startswith("lncf_train ")}
    for n, k in zip(("g_x", "g_weight", "g_bias"), need):
        if k:
            assert torch.equal(got[n], full[n]), n
        else:
            assert got[n] is None, n
    assert torch.equal(got["y"], full["y"])
    kind = "nchw" if layout is NCHW else "cl"
    need_p = need[1] or need[2]
    count = lambda key: sum(v for t, v in tags.items() if t.startswith("lncf_train " + key))          # noqa: E731
    assert count("fwd_" + kind) == 1 and count("bwd_" + kind) == 1 and count("reduce") == int(need_p), tags
    assert sum(tags.values()) == 2 + int(need_p), tags
    assert ("gx=%d gwb=%d" % (need[0], need_p)) in [t for t in tags if t.startswith("lncf_train bwd")][0], tags


def test_the_variant_tags_name_layout_dtype_and_mapping(L):
    lib = L.lib()
    want = {("c96", CL, torch.float32): "fwd_cl<f32,V=4,NV=3> G=8", ("c96", CL, torch.float16): "fwd_cl<f16,V=8,NV=3> G=4",
            ("c100", CL, torch.bfloat16): "fwd_cl<bf16,V=4,NV=1> G=32", ("c1536", CL, torch.float32): "fwd_cl<f32,V=4,NV=6> G=64",
            ("c96", NCHW, torch.float32): "fwd_nchw<f32,regs=16>", ("c1536", NCHW, torch.float16): "fwd_nchw<f16,stream=8>"}
    for (tag, layout, xd), text in want.items():
        ins = fixture_inputs(R.load_case(tag))
        lib.uni_variant_trace(1)
        try:
            run_op(ins, torch.float32, layout, x_dtype=xd, need=(False, False, False))
        finally:
            lib.uni_variant_trace(0)
        tags = [t for t in vc.read_trace(lib) if t.startswith("lncf_train ")]
        assert len(tags) == 1 and text in tags[0], (tag, tags)


def test_autograd_keeps_x_weight_and_the_statistics(L):
    from unicorn_amd.ops import layernorm_cf
    N, C, H, W = R.CASES["c100"]
    x, w, b, _ = (t.to(DEV).requires_grad_(True) for t in fixture_inputs(R.load_case("c100")))
    y = layernorm_cf(x, w, b)
    saved = y.grad_fn.saved_tensors
    assert sorted(tuple(t.shape) for t in saved) == sorted([(N, C, H, W), (C,), (N * H * W, 2)])
    ptrs = {t.data_ptr() for t in saved}
    assert x.data_ptr() in ptrs and w.data_ptr() in ptrs and y.data_ptr() not in ptrs and b.data_ptr() not in ptrs


def test_other_strides_are_converted_once(L):
    from unicorn_amd.ops import layernorm_cf
    ins = fixture_inputs(R.load_case("c96"))
    ref = run_op(ins, torch.float32, CL)
    x, w, b, g = (t.to(DEV) for t in ins)
    wide = torch.zeros(x.shape[0], x.shape[1], x.shape[2], x.shape[3] + 3, device=DEV)
    wide[..., :-3] = x
    xs = wide[..., :-3].requires_grad_(True)                         # neither NCHW-contiguous nor channels-last
    assert not xs.is_contiguous() and not xs.is_contiguous(memory_format=CL)
    y = layernorm_cf(xs, w, b)
    assert y.is_contiguous(memory_format=CL) and torch.equal(y, ref["y"])
    y.backward(g)
    assert torch.equal(xs.grad, ref["g_x"])


def test_empty_batch(L):
    from unicorn_amd.ops import layernorm_cf
    x = torch.zeros(0, 8, 3, 3, device=DEV, requires_grad=True)
    w, b = torch.ones(8, device=DEV, requires_grad=True), torch.zeros(8, device=DEV, requires_grad=True)
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        y = layernorm_cf(x, w, b)
        y.sum().backward()
    finally:
        lib.uni_variant_trace(0)
    assert not [t for t in vc.read_trace(lib) if t.startswith("lncf_train ")]
    assert tuple(y.shape) == (0, 8, 3, 3) and tuple(x.grad.shape) == (0, 8, 3, 3) and not w.grad.any() and not b.grad.any()


# ------------------------------------------------------------------------------------------------ the drop-in on a stand-in mini-backbone
def _proto():
    torch.manual_seed(5)
    net = R.MiniBackbone(16)
    with torch.no_grad():
        for blk in (net.block1, net.block2):
            blk.dwconv.bias.normal_(0, 0.1), blk.norm.weight.normal_(1, 0.1), blk.norm.bias.normal_(0, 0.1)
    return net


def _run_net(proto, x, t, dtype, fuse, autocast=False, train=True):
    """one forward (+ backward in training mode) of a copy of `proto` -> out, x.grad, the parameter gradients"""
    from unicorn_amd.nn import fuse_backbone
    net = copy.deepcopy(proto).to(DEV, dtype).train(train)
    if fuse:
        assert fuse_backbone(net) == (2, 2, 3)
    xi = x.to(DEV, dtype).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = net(xi)
    res = {"out": out.detach()}
    if train:
        (out * t.to(DEV, dtype)).sum().backward()
        res["x.grad"] = xi.grad
        res.update({n: p.grad for n, p in net.named_parameters()})
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _net_case():
    g = torch.Generator().manual_seed(1)
    x, t = torch.randn(2, 3, 36, 44, generator=g), torch.randn(2, 32, 4, 5, generator=g)
    proto = _proto()
    return proto, x, t, _run_net(proto, x, t, torch.float64, False)


def test_fused_backbone_against_the_unfused_one_fp64(L):
    proto, x, t, exact = _net_case()
    fused = _run_net(proto, x, t, torch.float64, True)
    assert sorted(fused) == sorted(exact)
    for n in exact:
        err = R.rel_err(fused[n], exact[n])
        print("%-24s fused vs unfused %.3e" % (n, err))
        assert err <= 1e-10, (n, err)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "fp16-autocast"])
def test_fused_backbone_against_the_unfused_one_fp32(L, autocast):
    """each run is compared with the unfused fp64 run, and the fused one may be at most 4 x as far from it as the unfused one is, per quantity.
    No figure comes from the kernels."""
    proto, x, t, exact = _net_case()
    plain = _run_net(proto, x, t, torch.float32, False, autocast=autocast)
    fused = _run_net(proto, x, t, torch.float32, True, autocast=autocast)
    bad = {}
    for n in exact:
        err, bound = R.rel_err(fused[n], exact[n]), 4 * R.rel_err(plain[n], exact[n])
        print("%-24s fused %.3e  bound %.3e" % (n, err, bound))
        assert fused[n].dtype == plain[n].dtype, n
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_fused_backbone_in_eval_mode_is_the_unfused_one(L):
    proto, x, t, _ = _net_case()
    fused, plain = _run_net(proto, x, t, torch.float32, True, train=False), _run_net(proto, x, t, torch.float32, False, train=False)
    assert torch.equal(fused["out"], plain["out"])
