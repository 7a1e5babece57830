"""ops.sot_prop_loss / vos_prop_loss (uni_prop_labels, the correlation operator, uni_prop_dice_pyramid_fwd / _bwd) on the GPU: the fixtures
the reference's own compute_loss_sot / compute_loss_vos produced (tests/golden/prop_loss_*.npz) -- labels and match table bit for bit,
fp64 at 1e-12 of scale, fp32 within 4 x the reference's own fp32-vs-fp64 deviation --, empty slots and the no-match sample, gradcheck,
bitwise repeatability, NCHW against channels-last, one-sided gradients, missing upstream gradients, and the 100 x 160 x 128 geometry against
the restatement on the same GPU with a check that neither the forward nor backward() waits for the stream."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import prop_loss_ref as R  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from unicorn_amd import _lib, ops as o
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


@pytest.fixture(scope="module")
def cases():
    return {tag: R.load_case(tag) for tag in R.CASES}


def inputs(tag, c):
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    t = {k: torch.from_numpy(c[k]).to(DEV) for k in R.INPUTS}
    t["masks"] = torch.from_numpy(c["masks"]).to(DEV) if r else None
    return t


def op_fn(ops, kind, targets, img_size, masks=None, max_inst=None, keep=None):
    """the operator behind the result keys of the restatement (keep: dict that receives the label rows)"""
    def fn(e0, e1):
        if kind == "sot":
            loss, (p8, p16, p32) = ops.sot_prop_loss(e0, e1, targets, img_size)
            return {"corr_loss": loss, "p8": p8, "p16": p16, "p32": p32, "num_matched": torch.ones(e0.shape[0], dtype=torch.int32, device=e0.device)}
        loss, (p8, p16, p32), matched, num = ops.vos_prop_loss(e0, e1, targets, img_size, masks, max_inst)
        return {"corr_loss": loss, "p8": p8, "p16": p16, "p32": p32, "matched": matched, "num_matched": num}
    return fn


def run_op(ops, tag, t, dtype, need=(True, True), channels_last=False):
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    e0 = t["embed_0"].to(dtype).clone(memory_format=fmt).requires_grad_(need[0])
    e1 = t["embed_1"].to(dtype).clone(memory_format=fmt).requires_grad_(need[1])
    res = op_fn(ops, kind, t["targets"], (8 * H8, 8 * W8), t["masks"], max_inst)(e0, e1)
    R.total_of(kind, res, t["w8"], t["w16"], t["w32"]).backward()
    out = {k: v.detach() for k, v in res.items()}
    out["g_embed_0"], out["g_embed_1"] = e0.grad, e1.grad
    return out


def relerr(got, ref):
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all())
    return float((got - ref).abs().max() / ref.abs().max())


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tag", list(R.CASES))
def test_labels_and_match_table_equal_the_fixture_bit_for_bit(ops, cases, tag, dtype):
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    c, t = cases[tag], inputs(tag, cases[tag])
    matched, num, gt0, gt1 = ops.prop_labels(t["targets"], H8, W8, R.case_kc(tag), dtype, t["masks"], sot=kind == "sot")
    assert gt0.dtype == dtype and matched.dtype == torch.int32 and num.dtype == torch.int32
    assert torch.equal(matched.cpu(), torch.from_numpy(c["matched"])) and torch.equal(num.cpu(), torch.from_numpy(c["num_matched"]))
    for got, k in ((gt0, "gt0"), (gt1, "gt1")):
        assert torch.equal(got.double().cpu(), torch.from_numpy(c[k]).reshape(got.shape)), (tag, k)
    if kind == "vos":                                                               # the public function hands the same table out
        _, _, m2, n2 = ops.vos_prop_loss(t["embed_0"], t["embed_1"], t["targets"], (8 * H8, 8 * W8), t["masks"], max_inst)
        assert torch.equal(m2, matched) and torch.equal(n2, num)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fp64_operator_equals_the_fixture(ops, cases, tag):
    c = cases[tag]
    got = run_op(ops, tag, inputs(tag, c), torch.float64)
    for k in R.FLOAT_RESULTS:
        err = relerr(got[k], torch.from_numpy(c[k]))
        print("fp64 %-12s %-10s err %.3g (bound 1e-12)" % (tag, k, err))
        assert err <= 1e-12, (tag, k, err)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fp32_operator_within_four_times_the_reference_fp32_error(ops, cases, tag):
    c = cases[tag]
    got = run_op(ops, tag, inputs(tag, c), torch.float32)
    bad = []
    for k in R.FLOAT_RESULTS:
        err, bound = relerr(got[k], torch.from_numpy(c[k])), 4 * float(c[k + "_fp32_ref_err"])
        print("fp32 %-12s %-10s err %.3g  fp32_ref_err %.3g  ratio %.2f (bound 4)" % (tag, k, err, bound / 4, 4 * err / bound))
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_empty_slots_are_exactly_zero_and_a_sample_without_a_match_has_a_zero_gradient(ops, cases, dtype):
    t = inputs("vos_box", cases["vos_box"])
    a = run_op(ops, "vos_box", t, dtype)
    assert a["num_matched"].tolist() == [4, 0] and bool((a["matched"][0, 4:] == -1).all()) and bool((a["matched"][1] == -1).all())
    for k in ("corr_loss", "p8", "p16", "p32"):
        assert not a[k][0, 4:].any() and not a[k][1].any() and bool(a[k][0, :4].any()), k
    assert not a["g_embed_0"][1].any() and not a["g_embed_1"][1].any() and bool(a["g_embed_0"][0].any()) and bool(a["g_embed_1"][0].any())
    # upstream gradients on the empty slots change nothing: w8 .. w32 are non-zero there already; now sample 1 gets a match and sample 0 stays
    t2 = dict(t, targets=t["targets"].clone())
    t2["targets"][1, 1, 0, 5] = 2.0
    b = run_op(ops, "vos_box", t2, dtype)
    assert b["num_matched"].tolist() == [4, 1] and bool(b["g_embed_0"][1].any())
    for k in ("corr_loss", "p8", "p16", "p32"):
        assert torch.equal(bits(a[k][0]), bits(b[k][0])), k
    # the gradients of sample 0 are those of total / 5 instead of total / 4: the same bits up to that factor's rounding; a fixed upstream
    # gradient shows the bits themselves
    for tt in (t, t2):
        e0, e1 = tt["embed_0"].to(dtype).clone().requires_grad_(True), tt["embed_1"].to(dtype).clone().requires_grad_(True)
        loss, pri, _, _ = ops.vos_prop_loss(e0, e1, tt["targets"], (64, 96))
        (loss.sum() + sum((w.to(dtype) * p).sum() for w, p in zip((tt["w8"], tt["w16"], tt["w32"]), pri))).backward()
        tt["g"] = (e0.grad, e1.grad)
    assert torch.equal(bits(t["g"][0][0]), bits(t2["g"][0][0])) and torch.equal(bits(t["g"][1][0]), bits(t2["g"][1][0]))
    assert not t["g"][0][1].any() and not t["g"][1][1].any()


def test_gradcheck_fp64(ops):
    g = torch.Generator().manual_seed(5)
    e0, e1 = (torch.randn(1, 5, 5, 6, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True) for _ in range(2))
    t = torch.zeros(1, 2, 3, 6)
    t[0, 0, :, 5], t[0, 1, :, 5] = torch.tensor([4., 0., 7.]), torch.tensor([7., 4., 9.])                 # K = 2 matches
    t[0, 0, :, 1:5] = torch.tensor([[13.125, 9.125, 16.5, 12.5], [20.125, 20.125, 8.5, 8.5], [30.125, 22.125, 20.5, 24.5]])
    t[0, 1, :, 1:5] = torch.tensor([[28.125, 18.125, 22.5, 20.5], [15.125, 12.125, 18.5, 14.5], [40.125, 30.125, 8.5, 8.5]])
    assert R.rule_violations(t) == []
    t = t.to(DEV)

    def sot(a, b):
        loss, pri = ops.sot_prop_loss(a, b, t, (40, 48))
        return (loss,) + pri

    def vos(a, b):
        loss, pri, _, num = ops.vos_prop_loss(a, b, t, (40, 48))
        assert num.tolist() == [2]
        return (loss,) + pri
    for fn in (sot, vos):
        assert torch.autograd.gradcheck(fn, (e0, e1), eps=1e-6, atol=1e-8, rtol=1e-6, nondet_tol=0.0)


def test_two_runs_are_bitwise_equal_and_layouts_agree(ops, cases):
    for tag in ("sot_ragged", "vos_k9", "vos_mask_r4"):
        t = inputs(tag, cases[tag])
        a, b = run_op(ops, tag, t, torch.float32), run_op(ops, tag, t, torch.float32)
        for k in a:
            assert torch.equal(bits(a[k]) if a[k].is_floating_point() else a[k], bits(b[k]) if b[k].is_floating_point() else b[k]), (tag, k)
        cl = run_op(ops, tag, t, torch.float32, channels_last=True)
        for k in R.FLOAT_RESULTS:
            assert torch.equal(bits(a[k]), bits(cl[k])), (tag, k)


def test_only_one_embedding_requires_grad(ops, cases):
    for tag in ("sot_flat", "vos_cap"):
        t = inputs(tag, cases[tag])
        full = run_op(ops, tag, t, torch.float32)
        only0, only1 = run_op(ops, tag, t, torch.float32, need=(True, False)), run_op(ops, tag, t, torch.float32, need=(False, True))
        assert only0["g_embed_1"] is None and only1["g_embed_0"] is None
        assert torch.equal(bits(only0["g_embed_0"]), bits(full["g_embed_0"])) and torch.equal(bits(only1["g_embed_1"]), bits(full["g_embed_1"]))
        assert torch.equal(bits(only0["corr_loss"]), bits(full["corr_loss"]))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_a_missing_upstream_gradient_is_left_out(ops, cases, dtype):
    """each subset of (loss, p8, p16, p32) alone against the restatement's autograd in the same dtype on this GPU, at the bound of the dtype"""
    tag = "vos_cap"
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    t = inputs(tag, cases[tag])
    ws = {"p8": t["w8"].to(dtype), "p16": t["w16"].to(dtype), "p32": t["w32"].to(dtype)}
    for use in (("corr_loss",), ("p8",), ("p16",), ("p32",), ("p16", "p32"), ("corr_loss", "p32")):
        def grads(which, run_dtype):
            e0, e1 = t["embed_0"].to(run_dtype).clone().requires_grad_(True), t["embed_1"].to(run_dtype).clone().requires_grad_(True)
            res = op_fn(ops, kind, t["targets"], (8 * H8, 8 * W8), None, max_inst)(e0, e1) if which == "op" else \
                R.vos_loss(e0, e1, t["targets"], (8 * H8, 8 * W8), None, max_inst)
            sum((res[k].sum() if k == "corr_loss" else (ws[k].to(run_dtype) * res[k]).sum()) for k in use).backward()
            return e0.grad, e1.grad
        got, r64 = grads("op", dtype), grads("ref", torch.float64)
        r32 = grads("ref", torch.float32) if dtype == torch.float32 else None
        for n in range(2):
            tol = 1e-12 if dtype == torch.float64 else 4 * relerr(r32[n], r64[n])      # the restatement's own fp32 deviation on this GPU
            assert relerr(got[n], r64[n]) <= tol, (use, n, relerr(got[n], r64[n]), tol)


def test_headline_100x160x128_b2_k3_against_the_restatement_and_without_a_sync(ops):
    B, H8, W8, M = 2, 100, 160, 4
    g = torch.Generator().manual_seed(21)
    e0, e1 = (0.25 * torch.randn(B, 128, H8, W8, generator=g)).to(DEV), (0.25 * torch.randn(B, 128, H8, W8, generator=g)).to(DEV)
    t = torch.zeros(B, 2, M, 6)
    t[..., 1:5] = R._box_rows(g, B * 2 * M, 8 * H8, 8 * W8).view(B, 2, M, 4)
    t[:, 0, :, 5], t[:, 1, :, 5] = torch.tensor([3., 1, 0, 2]), torch.tensor([2., 3, 1, 0])              # three matches per sample
    assert R.rule_violations(t) == []
    t = t.to(DEV)
    Kc = 3
    w = [torch.randn(B, Kc, H8 // s, W8 // s, generator=g).to(DEV) for s in (1, 2, 4)]
    size = (8 * H8, 8 * W8)
    r64 = R.loss_and_grads("vos", e0.double(), e1.double(), t, size, *w, max_inst=Kc)
    r32 = R.loss_and_grads("vos", e0, e1, t, size, *w, max_inst=Kc)
    got = R.loss_and_grads("vos", e0, e1, t, size, *w, fn=op_fn(ops, "vos", t, size, None, Kc))
    assert got["num_matched"].tolist() == [3, 3] and torch.equal(got["matched"].cpu(), r64["matched"])
    bad = []
    for k in R.FLOAT_RESULTS:
        ref_err, err = relerr(r32[k], r64[k]), relerr(got[k], r64[k])
        print("headline %-10s err %.3g  restatement fp32 err %.3g  ratio %.2f (bound 4)" % (k, err, ref_err, err / ref_err))
        if not err <= 4 * ref_err:
            bad.append((k, err, ref_err))
    assert not bad, bad
    del r64, r32
    # No-sync check by a busy stream (the method of tests/test_mot_corr_gpu.py)
    a, b = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
    res = op_fn(ops, "vos", t, size, None, Kc)(a, b)
    R.total_of("vos", res, *w).backward()                                           # library, allocator and kernels warm
    a.grad = b.grad = None
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    torch.cuda._sleep(1000000)
    s1.record()
    s1.synchronize()
    cycles = int(200.0 / max(s0.elapsed_time(s1), 1e-3) * 1000000)

    def while_the_stream_is_busy(what, fn):
        behind_spin = torch.cuda.Event()
        torch.cuda._sleep(cycles)
        behind_spin.record()
        torch.cuda.set_sync_debug_mode("error")
        try:
            t0 = time.perf_counter()
            out = fn()
            host_ms = (time.perf_counter() - t0) * 1e3
        finally:
            torch.cuda.set_sync_debug_mode("default")
        pending = not behind_spin.query()
        torch.cuda.synchronize()
        print("%s returned after %.2f ms on the host; spin kernel of %d cycles still running: %s" % (what, host_ms, cycles, pending))
        assert pending, "%s waited for the stream (%.1f ms on the host)" % (what, host_ms)
        return out
    res = while_the_stream_is_busy("vos_prop_loss", lambda: op_fn(ops, "vos", t, size, None, Kc)(a, b))
    total = R.total_of("vos", res, *w)
    while_the_stream_is_busy("backward()", lambda: total.backward())
    assert torch.equal(bits(a.grad), bits(got["g_embed_0"])) and torch.equal(bits(b.grad), bits(got["g_embed_1"]))
    sres = while_the_stream_is_busy("sot_prop_loss", lambda: ops.sot_prop_loss(a, b, t, size))
    while_the_stream_is_busy("backward() of the SOT loss", lambda: (sres[0] + sres[1][2].sum()).backward())
