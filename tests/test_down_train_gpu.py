"""GPU half of the differentiable downsample layers: ops.downsample_ln / ops.stem_conv against the fixtures that the reference's own layers
wrote (tests/golden/make_golden_down_train.py), half x and autocast against the fp64 restatement on the rounded inputs, the kernels alone
through the C-ABI against the patch-matrix restatement (tests/down_calls.py; no GEMM), a map with more pixel groups than rows of partials, a
patch matrix past 2^31 elements, what autograd keeps and launches, and the drop-in on lncf_ref.MiniBackbone.

No bound comes from the code under test: fp64 is held to 1e-12 (1e-10 through a whole net), fp32 to 4 x the larger of the fixture's yardstick
and the deviation of the eager fp32 lines on the same device from their fp64 run (test_pw_mlp_gpu.py's rule), half and autocast runs to 4 x
the deviation of the eager lines under the same dtypes, plus half an ulp where a result is rounded once more than eager's."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import down_calls as K  # noqa: E402
import down_train_ref as R  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
CL = torch.channels_last
HALF_ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # half an ulp relative to the value: the unit roundoff of the 11- and 8-bit significands


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def traced(L, fn):
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        out = fn()
    finally:
        lib.uni_variant_trace(0)
    return out, {t: v for t, v in vc.read_trace(lib).items() if t.startswith(("down_train ", "pw_mlp "))}


def run_op(ins, dtype=None, need=None, layout=CL, stem=False):
    """the operator under autograd on device copies of `ins` (the last one is grad_out) -> {y, g_*}; need: requires_grad per input"""
    from unicorn_amd import ops
    names = (R.STEM_INPUTS if stem else R.INPUTS)[:-1]
    need = (True,) * len(names) if need is None else need
    leaves = []
    for i, (t, k) in enumerate(zip(ins[:-1], need)):
        t = t.detach().to(DEV) if dtype is None or (i == 0 and t.dtype != torch.float32) else t.detach().to(DEV, dtype)
        if i == 0 and not stem:
            t = t.contiguous(memory_format=layout)
        leaves.append(t.clone(memory_format=torch.preserve_format).requires_grad_(k))
    y = (ops.stem_conv if stem else ops.downsample_ln)(*leaves)
    if any(need):
        y.backward(ins[-1].to(DEV, y.dtype))
    out = {"y": y.detach()}
    out.update({"g_" + n: t.grad for n, t in zip(names, leaves)})
    return out


def eager_dev(ins, stem=False, autocast=None, x_dtype=None):
    """the deviation of the eager lines on this device from the fp64 restatement of the same (rounded) inputs, per result; and that fp64 run"""
    ins = [t.to(DEV) for t in ins]
    if x_dtype is not None:
        ins[0] = ins[0].to(x_dtype)
    vg = R.stem_value_and_grads if stem else R.value_and_grads
    ref = vg(*[t.float() for t in ins], dtype=torch.float64)
    if autocast is None and x_dtype is None:
        low = vg(*ins, dtype=torch.float32)
    else:
        names = (R.STEM_INPUTS if stem else R.INPUTS)[:-1]
        leaves = [t.detach().clone().requires_grad_(True) for t in ins[:-1]]
        with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            y = (R.stem_forward if stem else R.forward)(*leaves)
        y.backward(ins[-1].to(y.dtype))
        low = {"y": y.detach()}
        low.update({"g_" + n: t.grad for n, t in zip(names, leaves)})
    return {k: R.rel_err(low[k], ref[k]) for k in ref}, ref, low


def fixture_inputs(tag):
    c = R.load_case(tag)
    return c, [torch.from_numpy(c[n]) for n in (R.STEM_INPUTS if tag.startswith("stem_") else R.INPUTS)]


# ------------------------------------------------------------------------------------------------ against the fixtures
@pytest.mark.parametrize("tag", list(R.CASES) + list(R.STEM_CASES))
def test_fixture_fp64_and_fp32(L, tag):
    stem = tag.startswith("stem_")
    c, ins = fixture_inputs(tag)
    results = R.STEM_RESULTS if stem else R.RESULTS
    got = run_op(ins, torch.float64, stem=stem)
    assert got["y"].dtype == torch.float64 and got["y"].is_contiguous(memory_format=CL)
    for k in results:
        err = R.rel_err(got[k], torch.from_numpy(c[k]))
        print("%-10s fp64 %-12s err %.3g" % (tag, k, err))
        assert err <= 1e-12, (k, err)
    dev, _, _ = eager_dev(ins, stem)
    got = run_op(ins, torch.float32, stem=stem)
    assert got["y"].dtype == torch.float32 and got["y"].is_contiguous(memory_format=CL)
    for k in results:
        err, bound = R.rel_err(got[k], torch.from_numpy(c[k])), 4 * max(float(c[k + "_fp32_ref_err"]), dev[k])
        print("%-10s fp32 %-12s err %.3g bound %.3g" % (tag, k, err, bound))
        assert err <= bound, (k, err, bound)
    if tag == "odd":
        gx = got["g_x"]
        assert not gx[:, :, 4:, :].any() and not gx[:, :, :, 6:].any()
    if tag == "stem_crop":
        gx = got["g_x"]
        assert not gx[:, :, 8:, :].any() and not gx[:, :, :, 12:].any()


# ------------------------------------------------------------------------------------------------ half x and autocast
@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c96", "c100", "odd"])
def test_half_x(L, tag, half):
    """x in fp16 / bf16 next to fp32 parameters: y fp32; x.grad has the dtype of x, one rounding more than the fp64 reference"""
    _, ins = fixture_inputs(tag)
    ins[0] = ins[0].to(half)
    dev, ref, _ = eager_dev(ins, x_dtype=half)
    got = run_op(ins)
    assert got["y"].dtype == torch.float32 and got["g_x"].dtype == half
    for k in R.RESULTS:
        err, bound = R.rel_err(got[k], ref[k]), 4 * dev[k] + (HALF_ULP[half] if k == "g_x" else 0.0)
        print("%-6s x %-8s %-12s err %.3g bound %.3g" % (tag, half, k, err, bound))
        assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c96", "odd", "stem_crop"])
def test_autocast(L, tag, half):
    stem = tag.startswith("stem_")
    _, ins = fixture_inputs(tag)
    dev, ref, low = eager_dev(ins, stem, autocast=half)
    with torch.autocast("cuda", dtype=half):
        got = run_op(ins, stem=stem)
    assert got["y"].dtype == low["y"].dtype == half and got["y"].is_contiguous(memory_format=CL)
    for k in ref:
        assert got[k].dtype == low[k].dtype, k
        err, bound = R.rel_err(got[k], ref[k]), 4 * dev[k]
        print("%-10s autocast %-8s %-12s err %.3g bound %.3g" % (tag, half, k, err, bound))
        assert err <= bound, (k, err, bound)


# ------------------------------------------------------------------------------------------------ the kernels alone
@pytest.mark.parametrize("dtype,x_dtype,a_dtype", [(torch.float64, torch.float64, torch.float64), (torch.float32, torch.float32, torch.float32),
                                                   (torch.float32, torch.float32, torch.float16), (torch.float32, torch.float16, torch.float16),
                                                   (torch.float32, torch.bfloat16, torch.float32), (torch.float32, torch.float32, torch.bfloat16)],
                         ids=["f64", "f32", "f32-a16", "x16-a16", "xbf-a32", "f32-abf"])
@pytest.mark.parametrize("tag", list(R.CASES))
def test_kernels_against_the_patch_restatement(L, tag, dtype, x_dtype, a_dtype):
    c, ins = fixture_inputs(tag)
    (N, Cc, H, W), _ = R.CASES[tag]
    x = ins[0].to(DEV, x_dtype)
    w, b = ins[1].to(DEV, dtype), ins[2].to(DEV, dtype)
    g = torch.Generator().manual_seed(7)
    gA = torch.randn(N * (H // 2) * (W // 2), 4 * Cc, generator=g).to(DEV, a_dtype)
    ref = R.patch_grads(x.double(), w.double(), b.double(), gA.double())
    low = R.patch_grads(x.float(), w.float(), b.float(), gA.float())               # the eager fp32 lines on the same inputs
    got = K.run_down(L, x, w, b, gA, a_dtype)
    assert torch.equal(got["A"].view(torch.uint8), got["A2"].view(torch.uint8)), "the rebuilt A differs from the forward's"
    got["stats"] = got["stats"].clone()
    f64 = dtype == torch.float64
    for k in ("A", "stats", "g_x", "g_ln_weight", "g_ln_bias"):
        yard = {"A": "y", "stats": "y"}.get(k, k)
        ulp = HALF_ULP.get(a_dtype if k == "A" else x_dtype if k == "g_x" else None, 0.0)
        bound = 1e-12 if f64 else 4 * max(float(c[yard + "_fp32_ref_err"]), R.rel_err(low[k], ref[k])) + ulp
        err = R.rel_err(got[k], ref[k])
        print("%-6s %-8s %-12s err %.3g bound %.3g" % (tag, x_dtype, k, err, bound))
        assert err <= bound, (k, err, bound)
    if tag == "odd":
        assert not got["g_x"][:, :, 4:, :].any() and not got["g_x"][:, :, :, 6:].any()
    # the parts alone keep their bits
    lone_x = K.run_down(L, x, w, b, gA, a_dtype, need_p=False)
    lone_p = K.run_down(L, x, w, b, gA, a_dtype, need_x=False)
    assert torch.equal(lone_x["g_x"], got["g_x"]) and lone_x["g_ln_weight"] is None
    assert torch.equal(lone_p["g_ln_weight"], got["g_ln_weight"]) and torch.equal(lone_p["g_ln_bias"], got["g_ln_bias"]) and lone_p["g_x"] is None


@pytest.mark.parametrize("dtype,x_dtype,a_dtype", [(torch.float64, torch.float64, torch.float64), (torch.float32, torch.float32, torch.float32),
                                                   (torch.float32, torch.float32, torch.float16), (torch.float32, torch.bfloat16, torch.bfloat16)],
                         ids=["f64", "f32", "f32-a16", "xbf-abf"])
@pytest.mark.parametrize("tag", list(R.STEM_CASES))
def test_gather_then_scatter_is_the_identity_on_the_kept_region(L, tag, dtype, x_dtype, a_dtype):
    (N, Cin, H, W), _ = R.STEM_CASES[tag]
    x = torch.from_numpy(R.load_case(tag)["x"]).to(DEV, x_dtype)
    f64 = dtype == torch.float64
    M = N * (H // 4) * (W // 4)
    A = torch.empty(M, 16 * Cin, device=DEV, dtype=a_dtype)
    back = torch.full_like(x, float("nan"))
    K.gather(L, f64, x, K.DT[x_dtype], (N, Cin, H, W), A, K.DT[a_dtype])
    K.scatter(L, f64, A, K.DT[a_dtype], (N, Cin, H, W), back, K.DT[x_dtype])
    torch.cuda.synchronize()
    assert torch.equal(A, R.to_patches(x, 4).to(a_dtype))
    want = torch.zeros_like(x)
    hk, wk = H // 4 * 4, W // 4 * 4
    want[:, :, :hk, :wk] = x[:, :, :hk, :wk].to(a_dtype).to(x_dtype)
    assert torch.equal(back, want)


# ------------------------------------------------------------------------------------------------ many pixels
def test_more_pixel_groups_than_rows_of_partials(L):
    """(1, 4, 520, 520) -> 4: 270400 pixels in groups of 256 are 1057 groups for 1024 blocks, so a block loops; eager fp64 on the device is the
    reference, 4 x eager fp32's own deviation the bound; two calls give the same bits"""
    ins = R.draw("plain", 31, (1, 4, 520, 520), 4)
    dev, ref, _ = eager_dev(ins)
    got, again = run_op(ins, torch.float32), run_op(ins, torch.float32)
    for k in R.RESULTS:
        err = R.rel_err(got[k], ref[k])
        print("many pixels %-12s err %.3g bound %.3g" % (k, err, 4 * dev[k]))
        assert err <= 4 * dev[k], (k, err, dev[k])
        assert torch.equal(got[k], again[k]), k


# ------------------------------------------------------------------------------------------------ past 2^31 elements of A
def test_patch_matrix_past_2_31_elements(L):
    """(1, 2048, 1032, 1024) in fp16 with a fp16 patch matrix: A has 516 * 512 rows of 8192 elements = 2^31 + 2^25, element 2^31 is the first of
    row 262144 (ho = 512).  The output rows ho = 0, 510 .. 513 (both sides of the crossing) and 515 are held to the patch restatement in fp64 on
    the same fp16 inputs: A to half an ulp, the statistics and grad_x to 4 x the eager fp32 lines' own deviation (+ half an ulp on grad_x)."""
    N, Cc, H, W = 1, 2048, 1032, 1024
    Ho, Wo = H // 2, W // 2
    elems = Ho * Wo * 4 * Cc
    assert elems > 1 << 31 and (1 << 31) // (4 * Cc) // Wo == 512
    need = 4 * 2 * elems + 8 * H * W + (2 << 30)                                  # x, A, grad_A, grad_x in fp16; stats; the reference's slices
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < 1.1 * need:
        pytest.skip("the case needs %d bytes of device memory (x 1.1), %d are free" % (need, free))
    g = torch.Generator(device=DEV).manual_seed(5)
    xr = torch.randn(H * W, Cc, device=DEV, dtype=torch.float16, generator=g)    # channels-last rows
    gA = torch.randn(Ho * Wo, 4 * Cc, device=DEV, dtype=torch.float16, generator=g)
    w = (1.0 + 0.1 * torch.randn(Cc, device=DEV, generator=g))
    b = 0.1 * torch.randn(Cc, device=DEV, generator=g)
    A = torch.empty_like(gA)
    gx = torch.empty_like(xr)
    stats = torch.empty(H * W, 2, device=DEV)
    try:
        K.down_fwd(L, False, xr, 1, w, b, (N, H, W, Cc), 0, A, 1, stats)
        K.down_bwd(L, False, xr, 1, w, stats, gA, 1, (N, H, W, Cc), gx, None, None, None, 0)
        torch.cuda.synchronize()
        for lo, hi in ((0, 1), (510, 514), (515, 516)):
            xs = xr[2 * lo * W:2 * hi * W].reshape(1, 2 * (hi - lo), W, Cc).permute(0, 3, 1, 2)
            gs = gA[lo * Wo:hi * Wo]
            ref = R.patch_grads(xs.double(), w.double(), b.double(), gs.double())
            low = R.patch_grads(xs.float(), w, b, gs.float())
            got = {"A": A[lo * Wo:hi * Wo], "stats": stats[2 * lo * W:2 * hi * W],
                   "g_x": gx[2 * lo * W:2 * hi * W].reshape(1, 2 * (hi - lo), W, Cc).permute(0, 3, 1, 2)}
            for k in got:
                bound = 4 * R.rel_err(low[k], ref[k]) + (HALF_ULP[torch.float16] if k != "stats" else 0.0)
                err = R.rel_err(got[k], ref[k])
                print("2^31: rows %d..%d %-6s err %.3g bound %.3g" % (lo, hi, k, err, bound))
                assert err <= bound, (lo, k, err, bound)
            del ref, low, got
    finally:
        del xr, gA, A, gx, stats
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ autograd and API behaviour
def _count(tags, key):
    return sum(v for t, v in tags.items() if t.startswith(key))


@pytest.mark.parametrize("need", [(1, 1, 1, 1, 1), (1, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 0, 0, 1, 0), (0, 0, 0, 0, 1), (1, 0, 0, 1, 0),
                                  (0, 1, 1, 0, 1), (0, 0, 0, 1, 1)], ids=lambda n: "".join(map(str, n)))
def test_need_flags_change_the_launch_list(L, need):
    _, ins = fixture_inputs("c96")
    need = tuple(bool(k) for k in need)
    full = run_op(ins, torch.float32)
    got, tags = traced(L, lambda: run_op(ins, torch.float32, need=need))
    for n, k in zip(R.INPUTS, need):
        if k:
            assert torch.equal(got["g_" + n], full["g_" + n]), n
        else:
            assert got["g_" + n] is None, n
    assert torch.equal(got["y"], full["y"])
    ln = need[0] or need[1] or need[2]
    need_p = need[1] or need[2]
    assert _count(tags, "down_train fwd_cl") == 1 and _count(tags, "down_train rebuild_cl") == int(need[3]), tags
    assert _count(tags, "down_train bwd_cl") == int(ln) and _count(tags, "down_train reduce") == int(need_p), tags
    assert _count(tags, "pw_mlp ") == 2 * int(need[4]), tags                          # the column sum and its reduce
    if ln:
        assert ("gx=%d gwb=%d" % (need[0], need_p)) in [t for t in tags if t.startswith("down_train bwd")][0], tags
    assert all("a=f32" in t for t in tags if "_cl<" in t), tags


def test_tags_name_the_element_types(L):
    _, ins = fixture_inputs("c96")
    ins[0] = ins[0].half()
    with torch.autocast("cuda", dtype=torch.float16):
        _, tags = traced(L, lambda: run_op(ins))
    for kind in ("fwd", "rebuild", "bwd"):
        assert any(t.startswith("down_train %s_cl<f16,V=8,NV=3> G=4 a=f16" % kind) for t in tags), tags
    _, sins = fixture_inputs("stem_small")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        _, tags = traced(L, lambda: run_op(sins, stem=True))
    assert tags.get("down_train gather4<x=f32,a=bf16>") == 2 and tags.get("down_train scatter4<x=f32,a=bf16>") == 1, tags


def test_stem_without_an_image_gradient_launches_no_scatter(L):
    _, ins = fixture_inputs("stem_crop")
    full = run_op(ins, torch.float32, stem=True)
    got, tags = traced(L, lambda: run_op(ins, torch.float32, need=(False, True, True), stem=True))
    assert got["g_x"] is None and torch.equal(got["g_weight"], full["g_weight"]) and torch.equal(got["g_bias"], full["g_bias"])
    assert _count(tags, "down_train gather4") == 2 and _count(tags, "down_train scatter4") == 0, tags
    got, tags = traced(L, lambda: run_op(ins, torch.float32, need=(True, False, False), stem=True))
    assert torch.equal(got["g_x"], full["g_x"]) and _count(tags, "down_train gather4") == 1 and _count(tags, "down_train scatter4") == 1, tags


def test_autograd_keeps_x_the_vectors_the_weight_and_the_statistics(L):
    from unicorn_amd.ops import downsample_ln, stem_conv
    (N, C, H, W), Co = R.CASES["c100"]
    _, ins = fixture_inputs("c100")
    x, lw, lb, w, b = (t.to(DEV).requires_grad_(True) for t in ins[:5])
    xc = x.detach().contiguous(memory_format=CL).requires_grad_(True)
    y = downsample_ln(xc, lw, lb, w, b)
    saved = y.grad_fn.saved_tensors
    assert sorted(tuple(t.shape) for t in saved) == sorted([(N, C, H, W), (C,), (C,), (Co, C, 2, 2), (N * H * W, 2)])
    ptrs = {t.data_ptr() for t in saved}
    assert {xc.data_ptr(), lw.data_ptr(), lb.data_ptr(), w.data_ptr()} <= ptrs and b.data_ptr() not in ptrs and y.data_ptr() not in ptrs
    assert y.is_contiguous(memory_format=CL) and tuple(y.shape) == (N, Co, H // 2, W // 2)
    # other strides are converted once: the same values, x.grad channels-last
    y2 = downsample_ln(x, lw, lb, w, b)
    assert torch.equal(y2, y) and y2.grad_fn.saved_tensors[0].is_contiguous(memory_format=CL)
    xs = torch.from_numpy(R.load_case("stem_small")["x"]).to(DEV)
    ws, bs = (torch.from_numpy(R.load_case("stem_small")[n]).to(DEV).requires_grad_(True) for n in ("weight", "bias"))
    ys = stem_conv(xs, ws, bs)
    assert sorted(tuple(t.shape) for t in ys.grad_fn.saved_tensors) == sorted([tuple(xs.shape), tuple(ws.shape)])
    assert ys.is_contiguous(memory_format=CL)


def test_empty_batch_makes_no_library_call(L):
    from unicorn_amd.ops import downsample_ln, stem_conv
    x = torch.zeros(0, 8, 4, 4, device=DEV, requires_grad=True)
    ps = [t.to(DEV).requires_grad_(True) for t in (torch.ones(8), torch.zeros(8), torch.zeros(16, 8, 2, 2), torch.zeros(16))]
    xs = torch.zeros(0, 3, 8, 8, device=DEV, requires_grad=True)
    pss = [t.to(DEV).requires_grad_(True) for t in (torch.zeros(16, 3, 4, 4), torch.zeros(16))]

    def fn():
        y = downsample_ln(x, *ps)
        y.sum().backward()
        ys = stem_conv(xs, *pss)
        ys.sum().backward()
        return y, ys
    (y, ys), tags = traced(L, fn)
    assert not tags
    assert tuple(y.shape) == (0, 16, 2, 2) and tuple(ys.shape) == (0, 16, 2, 2) and tuple(x.grad.shape) == (0, 8, 4, 4)
    assert all(not p.grad.any() and p.grad.shape == p.shape for p in ps + pss)


# ------------------------------------------------------------------------------------------------ the drop-in
def _proto():
    torch.manual_seed(5)
    net = R.MiniBackbone(16)
    with torch.no_grad():
        for blk in (net.block1, net.block2):
            blk.dwconv.bias.normal_(0, 0.1), blk.norm.weight.normal_(1, 0.1), blk.norm.bias.normal_(0, 0.1)
    return net


def _step(net, x, t, autocast=None):
    net.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
        out = net(x)
    (out.float() * t).sum().backward() if out.dtype != torch.float64 else (out * t).sum().backward()
    res = {"out": out.detach()}
    res.update({n: p.grad for n, p in net.named_parameters()})
    return res


@pytest.fixture(scope="module")
def nets():
    from unicorn_amd import nn as unn
    proto = _proto()
    g = torch.Generator().manual_seed(8)
    x, t = torch.randn(2, 3, 36, 44, generator=g), torch.randn(2, 32, 4, 5, generator=g)
    plain64 = copy.deepcopy(proto).double().to(DEV).train()
    ref = _step(plain64, x.double().to(DEV), t.double().to(DEV))
    return unn, proto, x, t, ref


def test_drop_in_fp64(L, nets):
    unn, proto, x, t, ref = nets
    net = copy.deepcopy(proto).double().to(DEV).train()
    counts = unn.fuse_model_down(net)
    assert counts[-1] == 2
    (got, tags) = traced(L, lambda: _step(net, x.double().to(DEV), t.double().to(DEV)))
    assert _count(tags, "down_train fwd_cl") == 1 and _count(tags, "down_train gather4") == 2, tags
    for k in ref:
        err = R.rel_err(got[k], ref[k])
        assert err <= 1e-10, (k, err)
    net.eval()
    plain = copy.deepcopy(proto).double().to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(net(x.double().to(DEV)), plain(x.double().to(DEV)))


@pytest.mark.parametrize("autocast", [None, torch.float16], ids=["fp32", "fp16-autocast"])
def test_drop_in_is_as_close_to_fp64_as_the_unfused_net(L, nets, autocast):
    unn, proto, x, t, ref = nets
    plain = copy.deepcopy(proto).to(DEV).train()
    fused = copy.deepcopy(proto).to(DEV).train()
    assert unn.fuse_model_down(fused)[-1] == 2
    a, b = _step(plain, x.to(DEV), t.to(DEV), autocast), _step(fused, x.to(DEV), t.to(DEV), autocast)
    assert b["out"].dtype == a["out"].dtype
    for k in ref:
        ea, eb = R.rel_err(a[k], ref[k]), R.rel_err(b[k], ref[k])
        print("drop-in %-14s %-28s unfused %.3g fused %.3g" % (autocast, k, ea, eb))
        assert eb <= 4 * ea, (k, ea, eb)
