"""The differentiable GroupNorm + activation on the GPU (ops.group_norm_act, csrc/gn_act_train.hip, unicorn_amd.nn.fuse_groupnorm_act): the
fixtures written from the reference's own modules in fp64 (1e-12; 1e-10 for `offset`) and fp32 (4 x the reference's own fp32 deviation) in both
memory layouts, fp16 / bf16 x, autocast, a group without variance, maps with more pixel units per image than rows of partials, the need flags
with the variant trace and the launch counts, what autograd keeps, other strides, an empty batch, and a stand-in mini-neck fused with
fuse_groupnorm_act against the unfused one."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gn_act_ref as R  # noqa: E402
import train_plans as P  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
CL, NCHW = torch.channels_last, torch.contiguous_format
LAYOUTS = [CL, NCHW]
LAYOUT_IDS = ["cl", "nchw"]


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def run_op(ins, G, act, eps, dtype, layout=CL, x_dtype=None, need=(True, True, True), g_layout=None):
    """ops.group_norm_act + backward on the device -> {y, g_x, g_weight, g_bias} (None where not needed); y and x.grad must come back in the
    memory layout of x, x.grad in its dtype"""
    from unicorn_amd.ops import group_norm_act
    x, w, b, g = (t.detach() for t in ins)
    x = x.to(DEV, x_dtype or dtype, copy=True).contiguous(memory_format=layout).requires_grad_(need[0])     # copies: inputs may be shared
    w = w.to(DEV, dtype, copy=True).requires_grad_(need[1])
    b = b.to(DEV, dtype, copy=True).requires_grad_(need[2])
    g = g.to(DEV, dtype).contiguous(memory_format=g_layout or layout)
    y = group_norm_act(x, G, w, b, eps, act)
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
    """1e-12; `offset` (conditioning 1e4) 1e-10, which a one-pass fp64 variance, off by about 5e-9 there, still fails"""
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), *R.CASES[tag][1:], torch.float64, layout)
    bad = {}
    for n in R.RESULTS:
        err = R.rel_err(got[n], torch.from_numpy(c[n]))
        print("%s fp64 %-8s err %.3e" % (tag, n, err))
        if not (got[n].shape == c[n].shape and err <= (1e-10 if tag == "offset" else 1e-12)):
            bad[n] = err
    assert not bad, bad


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp32_within_four_times_the_reference_fp32_deviation(L, tag, layout):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), *R.CASES[tag][1:], torch.float32, layout)
    bad = {}
    for n in R.RESULTS:
        err, bound = R.rel_err(got[n], torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
        print("%s fp32 %-8s err %.3e  bound %.3e" % (tag, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_grad_out_in_the_other_layout_is_converted_once(L):
    c = R.load_case("c96")
    ins, par = fixture_inputs(c), R.CASES["c96"][1:]
    for layout, other in ((CL, NCHW), (NCHW, CL)):
        same, mixed = run_op(ins, *par, torch.float32, layout), run_op(ins, *par, torch.float32, layout, g_layout=other)
        for n in R.RESULTS:
            assert torch.equal(same[n], mixed[n]), n


# ------------------------------------------------------------------------------------------------ half x
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("half,ulp", [(torch.float16, 2.0 ** -11), (torch.bfloat16, 2.0 ** -8)], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c96", "c100", "c1536"])
def test_half_x(L, tag, half, ulp, layout):
    """x in fp16 / bf16 next to fp32 parameters (what a convolution hands over under autocast), against the restatement in fp64 on the
    ROUNDED x.  y, weight.grad and bias.grad are fp32 results of fp32 arithmetic: the fp32 bound of the fixture.  x.grad is that fp32 result
    rounded once to the dtype of x: one rounding to nearest, at most half an ulp of the largest value (2^-11 fp16, 2^-8 bf16), on top of it.
    c96 and c1536 have C % 8 == 0 (8 channels per lane in the channels-last kernel), c100 has not (4 per lane)."""
    c = R.load_case(tag)
    G, act, eps = R.CASES[tag][1:]
    ins = fixture_inputs(c)
    ins[0] = ins[0].to(half).float()
    ref = R.value_and_grads(*ins, G, act, eps, dtype=torch.float64)
    got = run_op(ins, G, act, eps, torch.float32, layout, x_dtype=half)
    assert got["g_x"].dtype == half and got["y"].dtype == torch.float32
    bad = {}
    for n in R.RESULTS:
        err = R.rel_err(got[n], ref[n])
        bound = 4 * float(c[n + "_fp32_ref_err"]) + (ulp if n == "g_x" else 0.0)
        print("%s %s %-8s err %.3e  bound %.3e" % (tag, half, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_under_autocast_dtype_and_strides_are_those_of_the_eager_module(L):
    """what a convolution returns under fp16 autocast: a half, NCHW-contiguous map"""
    from unicorn_amd.ops import group_norm_act
    x, w, b, _ = (t.to(DEV) for t in R.draw("c96", 5))
    x = x.half()
    mod = R.StandInBaseConv(96, 96).to(DEV)
    with torch.no_grad():
        mod.bn.weight.copy_(w), mod.bn.bias.copy_(b)
    with torch.autocast("cuda", dtype=torch.float16):
        eager = mod.act(mod.bn(x))
        y = group_norm_act(x, 16, mod.bn.weight, mod.bn.bias, mod.bn.eps, "silu")
    assert y.dtype == eager.dtype == torch.float32 and y.stride() == eager.stride() and y.shape == eager.shape
    with torch.autocast("cuda", dtype=torch.float16):        # channels-last memory comes back as channels-last memory
        assert group_norm_act(x.contiguous(memory_format=CL), 16, mod.bn.weight, mod.bn.bias, mod.bn.eps, "silu").is_contiguous(memory_format=CL)


# ------------------------------------------------------------------------------------------------ a group without variance
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_zero_variance_group(L, layout):
    """group 0 of the `hw130` draw holds 0.3 everywhere: the first-pass sums are formed in double, where 520 x 0.3f is exact, so the mean is 0.3f,
    x - mean is 0 there and y is bias bit for bit; rstd = 1 / sqrt(eps)"""
    c = R.load_case("hw130")
    (N, C, H, W), G, act, eps = R.CASES["hw130"]
    assert act == "none" and G == 2
    x, w, b, g = fixture_inputs(c)
    x = x.clone()
    x[0, :C // G] = 0.3
    ref = R.value_and_grads(x, w, b, g, G, act, eps, dtype=torch.float64)
    got = run_op((x, w, b, g), G, act, eps, torch.float32, layout)
    assert torch.equal(got["y"][0, :C // G].cpu(), b[:C // G, None, None].expand(C // G, H, W))
    for n in R.RESULTS:
        assert torch.isfinite(got[n]).all(), n
    err, bound = R.rel_err(got["g_x"], ref["g_x"]), 4 * float(c["g_x_fp32_ref_err"])
    print("zero-variance group g_x err %.3e bound %.3e" % (err, bound))
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ more units per image than rows of partials
def many_shape(layout):
    """sized from the plan: B images share TRAIN_ROWS rows of partials, so an image has cap = TRAIN_ROWS / B rows; cap units of `unit` pixels
    (the most a unit takes: the listing's figure, which a map of more than TRAIN_ROWS such units has) and four pixels more make cap + 1 units,
    so row 0 takes two units, the second of four pixels.  Under 3 M elements."""
    plans, limits = P.plan_list()
    unit = plans[("gn_act", "cl" if layout == CL else "nchw", "f32", 8)][1]["unit"]
    B = 32 if layout == CL else 128
    cap = limits["TRAIN_ROWS"] // B
    C = 8 if layout == CL else 4
    shape = (B, C, 4, cap * unit // 4 + 1)
    assert shape[2] * shape[3] == cap * unit + 4 and B * C * shape[2] * shape[3] < 3e6
    return shape


@functools.lru_cache(maxsize=None)
def large_case(shape):
    """inputs on the device, the eager lines there in fp64, and their own deviation in fp32 (computed once per shape, shared, never modified)"""
    ins = [t.to(DEV) for t in R.draw("plain", sum(shape), shape)]
    ref = R.value_and_grads(*ins, 2, "silu", 1e-3, dtype=torch.float64)
    f32 = R.value_and_grads(*ins, 2, "silu", 1e-3, dtype=torch.float32)
    return ins, ref, {n: R.rel_err(f32[n], ref[n]) for n in R.RESULTS}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_more_units_than_rows_against_the_eager_lines(L, layout):
    """a block loops over two units.  fp32 bound: 4 x the distance of the eager fp32 lines on the same device from their fp64 run (the
    reference side); two calls are bit-equal."""
    shape = many_shape(layout)
    ins, ref, dev = large_case(shape)
    got, again = run_op(ins, 2, "silu", 1e-3, torch.float32, layout), run_op(ins, 2, "silu", 1e-3, torch.float32, layout)
    bad = {}
    for n in R.RESULTS:
        err, bound = R.rel_err(got[n], ref[n]), 4 * dev[n]
        print("%s %-8s fp32 err %.3e bound %.3e" % (shape, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
        assert torch.equal(got[n], again[n]), n
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ need flags, saved tensors, strides, N = 0
def traced(L, f):
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        out = f()
    finally:
        lib.uni_variant_trace(0)
    return out, {t: v for t, v in vc.read_trace(lib).items() if t.startswith("gn_act ")}


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
@pytest.mark.parametrize("need", [(True, True, True), (True, False, False), (False, True, True), (False, True, False)],
                         ids=["all", "x", "weight+bias", "weight"])
def test_need_flags_and_launch_counts(L, need, layout):
    """only what autograd asks for is computed: the other gradients are None, the wanted ones keep their bits, the launch of a skipped part is
    absent from the variant trace; at most three launches forward and three backward"""
    c = R.load_case("c96")
    ins, par = fixture_inputs(c), R.CASES["c96"][1:]
    full = run_op(ins, *par, torch.float32, layout)
    got, tags = traced(L, lambda: run_op(ins, *par, torch.float32, layout, need=need))
    for n, k in zip(("g_x", "g_weight", "g_bias"), need):
        if k:
            assert torch.equal(got[n], full[n]), n
        else:
            assert got[n] is None, n
    assert torch.equal(got["y"], full["y"])
    fwd = {t: v for t, v in tags.items() if t.startswith("gn_act fwd_")}
    bwd = {t: v for t, v in tags.items() if t.startswith("gn_act bwd_")}
    assert sorted(t.split()[1].split("_")[1].split("<")[0] for t in fwd) == ["apply", "part", "stats"] and sum(fwd.values()) == 3, fwd
    gx, gwb = int(need[0]), int(need[1] or need[2])
    flags = " gx=%d gwb=%d" % (gx, gwb)
    assert all(t.endswith(flags) for t in bwd), bwd
    kinds = sorted(t.split()[1].split("_")[1].split("<")[0] for t in bwd)
    assert kinds == (["comb", "dx", "part"] if gx else ["comb", "part"]) and sum(bwd.values()) == len(kinds) <= 3, bwd


def test_variant_tags_name_layout_dtype_and_mapping(L):
    want = {("c96", CL, torch.float32): "fwd_part_cl<f32,V=4> L=8 act=3", ("c96", CL, torch.float16): "fwd_part_cl<f16,V=8> L=16 act=3",
            ("c100", CL, torch.bfloat16): "fwd_part_cl<bf16,V=4> L=32 act=1", ("c1536", CL, torch.float32): "fwd_part_cl<f32,V=4> L=128 act=3",
            ("c96", NCHW, torch.float32): "fwd_part_nchw<f32> CT=16 act=3", ("hw130", NCHW, torch.float16): "fwd_part_nchw<f16> CT=16 act=0"}
    for (tag, layout, xd), text in want.items():
        ins, par = fixture_inputs(R.load_case(tag)), R.CASES[tag][1:]
        _, tags = traced(L, lambda: run_op(ins, *par, torch.float32, layout, x_dtype=xd, need=(False, False, False)))
        assert len(tags) == 3 and "gn_act " + text in tags and "gn_act " + text.replace("fwd_part", "fwd_apply") in tags, (tag, tags)
        cls = P.predicted("gn_act", "cl" if layout == CL else "nchw", {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[xd],
                          R.CASES[tag][0][1])
        assert cls in text                        # the class of the tag is what the plan listing says
    ins, par = fixture_inputs(R.load_case("small")), R.CASES["small"][1:]
    _, tags = traced(L, lambda: run_op(ins, *par, torch.float64, NCHW))
    assert set(tags) == {"gn_act fwd_part_nchw<f64> CT=16 act=3", "gn_act fwd_stats<f64>", "gn_act fwd_apply_nchw<f64> CT=16 act=3",
                         "gn_act bwd_part_nchw<f64> CT=16 act=3 gx=1 gwb=1", "gn_act bwd_comb<f64> gx=1 gwb=1",
                         "gn_act bwd_dx_nchw<f64> CT=16 act=3 gx=1 gwb=1"}, tags


def test_autograd_saves_x_the_parameters_and_the_statistics(L):
    from unicorn_amd.ops import group_norm_act
    (N, C, H, W), G, act, eps = R.CASES["c100"]
    x, w, b, _ = (t.to(DEV).requires_grad_(True) for t in fixture_inputs(R.load_case("c100")))
    y = group_norm_act(x, G, w, b, eps, act)
    saved = y.grad_fn.saved_tensors
    assert sorted(tuple(t.shape) for t in saved) == sorted([(N, C, H, W), (C,), (C,), (N * G, 2)])
    ptrs = {t.data_ptr() for t in saved}
    assert x.data_ptr() in ptrs and w.data_ptr() in ptrs and b.data_ptr() in ptrs and y.data_ptr() not in ptrs


def test_other_strides_are_converted_once_to_channels_last(L):
    from unicorn_amd.ops import group_norm_act
    c = R.load_case("c96")
    G, act, eps = R.CASES["c96"][1:]
    x, w, b, g = (t.to(DEV) for t in fixture_inputs(c))
    wide = torch.zeros(2, 96, 9, 14, device=DEV)
    wide[..., ::2] = x
    xs = wide[..., ::2].requires_grad_(True)                            # neither NCHW-contiguous nor channels-last
    assert not xs.is_contiguous() and not xs.is_contiguous(memory_format=CL)
    y = group_norm_act(xs, G, w, b, eps, act)
    y.backward(g)
    assert y.is_contiguous(memory_format=CL)
    ref = run_op(fixture_inputs(c), G, act, eps, torch.float32, CL)
    assert torch.equal(y.detach(), ref["y"]) and torch.equal(xs.grad, ref["g_x"])


def test_empty_batch_makes_no_library_call(L):
    from unicorn_amd.ops import group_norm_act
    x = torch.zeros(0, 8, 3, 3, device=DEV, requires_grad=True)
    w, b = torch.ones(8, device=DEV, requires_grad=True), torch.zeros(8, device=DEV, requires_grad=True)

    def go():
        y = group_norm_act(x, 2, w, b)
        y.sum().backward()
        return y
    y, tags = traced(L, go)
    assert not tags
    assert tuple(y.shape) == (0, 8, 3, 3) and tuple(x.grad.shape) == (0, 8, 3, 3) and not w.grad.any() and not b.grad.any()


# ------------------------------------------------------------------------------------------------ the drop-in on a stand-in mini-neck
def _proto():
    torch.manual_seed(5)
    return R.MiniNeck(32)


def _run_net(proto, xs, t, dtype, fuse, autocast=False, train=True):
    """one forward (+ backward in training mode) of a copy of `proto` -> out, the input gradients, the parameter gradients"""
    from unicorn_amd.nn import fuse_groupnorm_act
    net = copy.deepcopy(proto).to(DEV, dtype).train(train)
    if fuse:
        assert fuse_groupnorm_act(net) == 5
    xi = [x.to(DEV, dtype).requires_grad_(True) for x in xs]
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        out = net(*xi)
    res = {"out": out.detach()}
    if train:
        (out * t.to(DEV, dtype)).sum().backward()
        res["fine.grad"], res["coarse.grad"] = xi[0].grad, xi[1].grad
        res.update({n: p.grad for n, p in net.named_parameters()})
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _net_case():
    g = torch.Generator().manual_seed(1)
    xs = (torch.randn(2, 32, 10, 14, generator=g), torch.randn(2, 64, 5, 7, generator=g))
    t = torch.randn(2, 64, 10, 14, generator=g)
    proto = _proto()
    return proto, xs, t, _run_net(proto, xs, t, torch.float64, False)


def test_fused_neck_against_the_unfused_one_fp64(L):
    proto, xs, t, exact = _net_case()
    fused, tags = traced(L, lambda: _run_net(proto, xs, t, torch.float64, True))
    assert sum(v for k, v in tags.items() if "fwd_apply" in k) == 5                 # the operator ran at all five sites
    assert sorted(fused) == sorted(exact)
    for n in exact:
        err = R.rel_err(fused[n], exact[n])
        print("%-24s fused vs unfused %.3e" % (n, err))
        assert err <= 1e-10, (n, err)


@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "fp16-autocast"])
def test_fused_neck_against_the_unfused_one_fp32(L, autocast):
    """each run is compared with the unfused fp64 run, and the fused one may be at most 4 x as far from it as the unfused one is, per quantity.
    No figure comes from the kernels."""
    proto, xs, t, exact = _net_case()
    plain = _run_net(proto, xs, t, torch.float32, False, autocast=autocast)
    fused = _run_net(proto, xs, t, torch.float32, True, autocast=autocast)
    bad = {}
    for n in exact:
        err, bound = R.rel_err(fused[n], exact[n]), 4 * R.rel_err(plain[n], exact[n])
        print("%-24s fused %.3e  bound %.3e" % (n, err, bound))
        assert fused[n].dtype == plain[n].dtype, n
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_fused_neck_in_eval_mode_is_the_unfused_one(L):
    proto, xs, t, _ = _net_case()
    fused, plain = _run_net(proto, xs, t, torch.float32, True, train=False), _run_net(proto, xs, t, torch.float32, False, train=False)
    assert torch.equal(fused["out"], plain["out"])
