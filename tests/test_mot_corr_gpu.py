"""uni_mot_corr_loss_fwd / _bwd through ops.mot_corr_loss on the GPU: the fixtures the reference's own compute_loss_mot_corr produced
(tests/golden/mot_corr_*.npz) in fp64 at 1e-12 of scale and in fp32 within 4 x the reference's own fp32-vs-fp64 deviation, the NaN and
zero-gradient rule, gradcheck, bitwise repeatability, NCHW against channels-last maps, one-sided gradients, the 100 x 160 x 128 geometry
against the vectorised restatement on the same GPU, and a check that neither the forward nor backward() waits for the stream."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import mot_corr_ref as R  # noqa: E402

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


def inputs(c, dtype):
    return (torch.from_numpy(c["embed_0"]).to(DEV, dtype), torch.from_numpy(c["embed_1"]).to(DEV, dtype), torch.from_numpy(c["targets"]).to(DEV),
            torch.from_numpy(c["grad_loss"]).to(DEV, dtype))


def run_op(ops, e0, e1, targets, grad_loss, bidirect, grid_sample, need=(True, True), channels_last=False):
    """-> loss (B,), grad of embed_0, grad of embed_1 (None where not required)"""
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    a = e0.detach().clone(memory_format=fmt).requires_grad_(need[0])
    b = e1.detach().clone(memory_format=fmt).requires_grad_(need[1])
    loss = ops.mot_corr_loss(a, b, targets, R.S, bidirect, grid_sample)
    assert loss.shape == (e0.shape[0],) and loss.dtype == e0.dtype
    loss.backward(grad_loss)
    return loss.detach(), a.grad, b.grad


def relerr(got, ref):
    """max|got - ref| / max|ref| over the finite entries of ref; the NaN positions must be equal"""
    got, ref = got.detach().double().cpu(), ref.double().cpu()
    fin = torch.isfinite(ref)
    assert torch.equal(fin, torch.isfinite(got)), "NaN positions differ"
    return float((got - ref)[fin].abs().max() / ref[fin].abs().max())


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fp64_operator_equals_the_fixture(ops, cases, tag):
    c = cases[tag]
    got = dict(zip(R.RESULTS, run_op(ops, *inputs(c, torch.float64), *R.CASES[tag][5:7])))
    for k in R.RESULTS:
        err = relerr(got[k], torch.from_numpy(c[k]))
        print("fp64 %-8s %-10s err %.3g (bound 1e-12)" % (tag, k, err))
        assert err <= 1e-12, (tag, k, err)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_fp32_operator_within_four_times_the_reference_fp32_error(ops, cases, tag):
    c = cases[tag]
    got = dict(zip(R.RESULTS, run_op(ops, *inputs(c, torch.float32), *R.CASES[tag][5:7])))
    bad = []
    for k in R.RESULTS:
        err, bound = relerr(got[k], torch.from_numpy(c[k])), 4 * float(c[k + "_fp32_ref_err"])
        print("fp32 %-8s %-10s err %.3g  fp32_ref_err %.3g  ratio %.2f (bound 4)" % (tag, k, err, bound / 4, 4 * err / bound))
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_nan_loss_and_exactly_zero_gradient_without_a_matched_pair_or_an_instance(ops, cases, dtype):
    c = cases["nomatch"]
    e0, e1, t, g = inputs(c, dtype)
    loss, g0, g1 = run_op(ops, e0, e1, t, g, True, True)
    assert torch.isnan(loss).tolist() == [False, True, False]
    assert not g0[1].any() and not g1[1].any() and bool(g0[0].any()) and bool(g1[2].any())
    assert bool(torch.isfinite(g0).all()) and bool(torch.isfinite(g1).all())
    # a frame without an instance (the reference raises there): NaN and zero gradient for that sample, the others bit for bit as before
    t2 = t.clone()
    t2[1, 0, :, 5] = 0
    t3 = t.clone()
    t3[1, 1, :, 5] = 0
    for tt in (t2, t3):
        l2, h0, h1 = run_op(ops, e0, e1, tt, g, True, True)
        assert torch.isnan(l2).tolist() == [False, True, False] and not h0[1].any() and not h1[1].any()
        assert torch.equal(l2[[0, 2]], loss[[0, 2]]) and torch.equal(h0, g0) and torch.equal(h1, g1)
    # B == 0 and M == 0 return without a call
    assert ops.mot_corr_loss(e0[:0], e1[:0], t[:0]).shape == (0,)
    a = e0.clone().requires_grad_(True)
    l0 = ops.mot_corr_loss(a, e1, t[:, :, :0])
    assert bool(torch.isnan(l0).all()) and l0.shape == (3,)
    l0.backward(g)
    assert a.grad.shape == e0.shape and not a.grad.any()


def test_gradcheck_fp64(ops):
    g = torch.Generator().manual_seed(5)
    e0, e1 = (torch.randn(1, 5, 4, 6, generator=g, dtype=torch.float64).to(DEV).requires_grad_(True) for _ in range(2))
    t = torch.zeros(1, 2, 5, 6)
    t[0, 0, :3, 5] = torch.tensor([4., 2., 7.])
    t[0, 1, :4, 5] = torch.tensor([7., 9., 4., 2.])
    t[0, 0, :3, 1:3] = torch.tensor([[13.3, 9.1], [40.7, 22.9], [-3.0, 29.4]])     # one centre left of the map
    t[0, 1, :4, 1:3] = torch.tensor([[21.7, 5.3], [30.1, 17.7], [44.9, 30.3], [14.2, 9.6]])
    t = t.to(DEV)
    assert R.rule_violations(t.cpu(), 4, 6, True) == []
    for bidirect in (True, False):
        assert torch.autograd.gradcheck(lambda a, b: ops.mot_corr_loss(a, b, t, R.S, bidirect, True), (e0, e1), eps=1e-6, atol=1e-8, rtol=1e-6,
                                        nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda a, b: ops.mot_corr_loss(a, b, t, R.S, True, False), (e0, e1), eps=1e-6, atol=1e-8, rtol=1e-6,
                                    nondet_tol=0.0)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def test_two_runs_are_bitwise_equal_and_layouts_agree(ops, cases):
    for tag in ("crowd", "edge"):
        c = cases[tag]
        ins = inputs(c, torch.float32)
        a, b = run_op(ops, *ins, True, True), run_op(ops, *ins, True, True)
        for x, y in zip(a, b):
            assert torch.equal(bits(x), bits(y))
        # channels-last maps are read and their gradients written in place: only addresses change, every sum keeps its order
        cl = run_op(ops, *ins, True, True, channels_last=True)
        assert cl[1].is_contiguous(memory_format=torch.channels_last) and a[1].is_contiguous()
        for x, y in zip(a, cl):
            assert torch.equal(bits(x), bits(y))


def test_only_one_embedding_requires_grad(ops, cases):
    c = cases["plain"]
    ins = inputs(c, torch.float32)
    full = run_op(ops, *ins, True, True)
    only0, only1 = run_op(ops, *ins, True, True, need=(True, False)), run_op(ops, *ins, True, True, need=(False, True))
    assert only0[2] is None and only1[1] is None
    assert torch.equal(bits(only0[1]), bits(full[1])) and torch.equal(bits(only1[2]), bits(full[2]))
    assert torch.equal(bits(only0[0]), bits(full[0])) and torch.equal(bits(only1[0]), bits(full[0]))
    with torch.no_grad():
        assert torch.equal(bits(ops.mot_corr_loss(*ins[:3])), bits(full[0]))


def test_headline_100x160x128_b4_m100_against_the_restatement_and_without_a_sync(ops):
    B, C, H, W, M = 4, 128, 100, 160, 100
    e0, e1, t, g = (x.to(DEV) for x in R.draw("large", 11, (B, C, H, W, M)))
    assert R.rule_violations(t.cpu(), H, W, True) == []
    # the yardstick: the vectorised restatement in fp32 and in fp64 on this GPU; the operator is held to 4 x their deviation
    r64 = R.loss_and_grads(R.loss_vectorised, e0.double(), e1.double(), t, g.double(), True, True)
    r32 = R.loss_and_grads(R.loss_vectorised, e0, e1, t, g, True, True)
    got = dict(zip(R.RESULTS, run_op(ops, e0, e1, t, g, True, True)))
    bad = []
    for k in R.RESULTS:
        ref_err, err = relerr(r32[k], r64[k]), relerr(got[k], r64[k])
        print("headline %-10s err %.3g  restatement fp32 err %.3g  ratio %.2f (bound 4)" % (k, err, ref_err, err / ref_err))
        if not err <= 4 * ref_err:
            bad.append((k, err, ref_err))
    assert not bad, bad
    # No-sync check by a busy stream (the method of tests/test_simota_gpu.py): a spin kernel of ~0.2 s (calibrated first), an event behind
    # it, then the call.  The call must return while the event is still pending; set_sync_debug_mode("error") holds torch's operators too.
    a, b = e0.clone().requires_grad_(True), e1.clone().requires_grad_(True)
    ops.mot_corr_loss(a, b, t).backward(g)                                          # library, allocator and kernels warm
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
    loss = while_the_stream_is_busy("mot_corr_loss", lambda: ops.mot_corr_loss(a, b, t))
    while_the_stream_is_busy("backward()", lambda: loss.backward(g))
    assert torch.equal(bits(loss.detach()), bits(got["loss"])) and torch.equal(bits(a.grad), bits(got["g_embed_0"]))
    assert torch.equal(bits(b.grad), bits(got["g_embed_1"]))
