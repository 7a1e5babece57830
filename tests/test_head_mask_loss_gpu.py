"""uni_head_mask_loss_fwd / _bwd through ops.head_mask_loss on the GPU: every fixture that the reference's own get_losses produced
(tests/golden/head_mask_loss_*.npz) in fp64 within 1e-12 of scale and in fp32 within 4 x max(the reference's own fp32-vs-fp64 deviation,
one fp32 ulp); fed by head_det_loss's own assignment; against the loop of per-image condinst_dice_loss calls it replaces; gradcheck; bitwise
repeatability; one-sided gradients; a row pitch on dynamic_params; capacity equal to and below the instance count (the NaN rule); and the
headline geometry with a check that forward and backward return while the stream is busy and that no per-instance ground-truth map is
materialised."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import condinst_loss_ref as CR  # noqa: E402
import head_loss_ref as HR  # noqa: E402
import head_mask_loss_ref as R  # noqa: E402
import simota_ref as S  # noqa: E402

DEV = "cuda"
TAGS = sorted(R.CASES)
KINK = 5e-5            # tests/test_condinst_loss_gpu.py: above the a-priori fp32 error of the 10- and 8-term pre-activation sums


@pytest.fixture(scope="module")
def ops():
    from unicorn_amd import _lib, ops as o
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def hip_run(ops, mf, um, dp, lvl, masks, fg, matched, xs, ys, st, r, grad_out, dtype=None, need=(True, True, True), capacity=None,
            assignment=None, pitch=None):
    """ops.head_mask_loss with its backward -> the five quantities like R.loss_and_grads (a gradient not asked for: None)"""
    dtype = mf.dtype if dtype is None else dtype
    f = [t.to(device=DEV, dtype=dtype) for t in (mf, um, dp, masks, xs, ys, st)]
    if pitch is not None:                                                 # dynamic_params as a view of rows of `pitch` columns, NaN beside it
        wide = torch.full(dp.shape[:2] + (pitch,), float("nan"), device=DEV, dtype=dtype)
        wide[:, :, :169] = f[2]
        f[2] = wide.requires_grad_(need[2])[:, :, :169]
        leaf = wide
    else:
        leaf = f[2] = f[2].clone().requires_grad_(need[2])
    f[0], f[1] = f[0].clone().requires_grad_(need[0]), f[1].clone().requires_grad_(need[1])
    if assignment is None:
        fg_, mg_ = fg.to(DEV), matched.to(DEV)
        assignment = (fg_, mg_, torch.zeros(fg.shape, device=DEV), fg_.sum(dim=1))
    loss, per = ops.head_mask_loss(f[0], f[1], f[2], lvl.to(DEV), f[3], assignment, f[4][None], f[5][None], f[6][None], r, capacity=capacity)
    assert loss.shape == () and loss.dtype == dtype and per.shape == (mf.shape[0],) and per.dtype == dtype and not per.requires_grad
    if any(need):
        (loss * grad_out).backward()
    g_dp = leaf.grad
    if pitch is not None and g_dp is not None:
        assert not g_dp[:, :, 169:].any()
        g_dp = g_dp[:, :, :169]
    return {"loss_condinst": loss.detach(), "per_image": per, "g_mask_feats": f[0].grad, "g_up_masks": f[1].grad, "g_dynamic_params": g_dp}


def hold(got, want, bound_of, what):
    for k in R.QUANTITIES:
        e, b = R.rel_err(got[k], want[k]), bound_of(k)
        print("%s %-17s err %.3g  bound %.3g" % (what, k, e, b))
        assert e <= b, (what, k, e, b)


def zeros_where_the_reference_has_them(got, fg):
    fg = fg.to(got["g_dynamic_params"].device)
    assert not got["g_dynamic_params"][~fg].any()                                        # background rows: exact zeros
    for b in range(fg.shape[0]):
        if not bool(fg[b].any()):                                                         # an image without foreground: exact zeros
            assert float(got["per_image"][b]) == 0.0 and not got["g_mask_feats"][b].any() and not got["g_up_masks"][b].any()


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp64(ops, tag):
    c = R.load_case(tag)
    args = R.fixture_tensors(c, tag)
    got = hip_run(ops, *args, float(c["grad_out"]), torch.float64)
    hold(got, R.expected(c, tag), lambda k: 1e-12, tag)
    zeros_where_the_reference_has_them(got, args[5])


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp32(ops, tag):
    c = R.load_case(tag)
    args = R.fixture_tensors(c, tag)
    got = hip_run(ops, *args, float(c["grad_out"]), torch.float32)
    hold(got, R.expected(c, tag), lambda k: R.bound32(c[k + "_fp32_ref_err"]), tag)
    zeros_where_the_reference_has_them(got, args[5])
    if tag == "empty":
        assert float(got["loss_condinst"]) == 0.0 and not any(got[k].any() for k in R.QUANTITIES[1:])


def test_fed_by_head_det_loss_own_assignment(ops):
    c, h = R.load_case("batch"), HR.load_case("batch")
    H, W, C = (int(v) for v in h["shape"])
    args = R.fixture_tensors(c, "batch")
    xs, ys, st = (t.to(DEV) for t in S.anchors(H, W))
    _, own = ops.head_det_loss(torch.from_numpy(h["outputs"]).to(DEV), torch.from_numpy(h["origin_preds"]).to(DEV),
                               torch.from_numpy(h["labels"]).to(DEV), xs[None], ys[None], st[None], (H, W), C)
    assert torch.equal(own[0].cpu(), args[5]) and torch.equal(own[1].cpu()[args[5]], args[6][args[5]])
    for dtype in (torch.float32, torch.float64):
        a = hip_run(ops, *args, float(c["grad_out"]), dtype, assignment=own)
        b = hip_run(ops, *args, float(c["grad_out"]), dtype)
        assert all(torch.equal(bits(a[k]), bits(b[k])) for k in R.QUANTITIES)
    hold(a, R.expected(c, "batch"), lambda k: 1e-12, "batch, own assignment")


def per_image_loop(ops, mf, um, dp, lvl, masks, fg, matched, xs, ys, st, r, grad_out, dtype):
    """the path being replaced: :675-694 / :731-732 with ops.condinst_dice_loss on rows compacted by boolean index"""
    f = [t.to(device=DEV, dtype=dtype) for t in (mf, um, dp, masks, xs, ys, st)]
    mf_, um_, dp_ = (t.clone().requires_grad_(True) for t in f[:3])
    fg_, mg_, lvl_ = fg.to(DEV), matched.to(DEV), lvl.to(DEV)
    loss_masks, num_valid = [], 0
    for b in range(mf.shape[0]):
        if torch.sum(fg_[b]) > 0:
            p, loc, lv, gt = R.instances(b, dp_, lvl_, f[3], fg_, mg_, f[4], f[5], f[6])
            loss_masks.append(ops.condinst_dice_loss(mf_[b:b + 1], um_[b:b + 1], p, loc, lv, gt.unsqueeze(1), r).mean())
            num_valid += 1
        else:
            loss_masks.append(torch.sum(mf_[b:b + 1]) * 0.0 + torch.sum(dp_[b]) * 0.0)
    loss_masks = torch.stack(loss_masks)
    loss = torch.sum(loss_masks) / max(num_valid, 1)
    (loss * grad_out).backward()
    return {"loss_condinst": loss.detach(), "per_image": loss_masks.detach(), "g_mask_feats": mf_.grad,
            "g_up_masks": torch.zeros_like(um_) if um_.grad is None else um_.grad, "g_dynamic_params": dp_.grad}


@pytest.mark.parametrize("tag", ["batch", "edge"])
def test_equals_the_loop_of_per_image_condinst_dice_loss(ops, tag):
    c = R.load_case(tag)
    args = R.fixture_tensors(c, tag)
    want = R.expected(c, tag)
    for dtype, bound_of in ((torch.float64, lambda k: 1e-12), (torch.float32, lambda k: R.bound32(c[k + "_fp32_ref_err"]))):
        loop = per_image_loop(ops, *args, float(c["grad_out"]), dtype)
        got = hip_run(ops, *args, float(c["grad_out"]), dtype)
        hold(loop, want, bound_of, "%s loop %s" % (tag, dtype))
        hold(got, {k: loop[k].double() for k in R.QUANTITIES}, bound_of, "%s operator vs loop %s" % (tag, dtype))      # the same bar


def small_problem(seed, B=2, H8=4, W8=5, r=2, A=9, M=2, fg_rows=((1, 4, 7), (0, 8))):
    g = torch.Generator().manual_seed(seed)
    mf, um = torch.randn(B, 8, H8, W8, generator=g), torch.randn(B, 9 * r * r, H8, W8, generator=g)
    dp = 0.5 * torch.randn(B, A, 169, generator=g)
    lvl = torch.randint(0, 5, (B, A), generator=g).to(torch.int32)
    masks = (torch.rand(B, M, r * H8, r * W8, generator=g) < 0.4).float()
    fg = torch.zeros(B, A, dtype=torch.bool)
    for b, rows in enumerate(fg_rows):
        fg[b, list(rows)] = True
    matched = torch.where(fg, torch.randint(0, M, (B, A), generator=g), torch.full((B, A), -1))
    xs, ys = torch.randint(0, W8, (A,), generator=g).float(), torch.randint(0, H8, (A,), generator=g).float()
    st = torch.full((A,), 8.0)
    return mf, um, dp, lvl, masks, fg, matched, xs, ys, st, r


def test_gradcheck_fp64(ops):
    """a 4 x 5 coarse map, up_rate 2, B 2, A 6, 5 instances; no foreground pre-activation within 1e-3 of a ReLU kink (asserted, not filtered)"""
    mf, um, dp, lvl, masks, fg, matched, xs, ys, st, r = small_problem(32, A=6, fg_rows=((1, 4, 5), (0, 3)))      # seed 32: nearest kink at 2.2e-3
    assert int(fg.sum()) == 5
    d = [t.double() for t in (mf, um, dp, masks, xs, ys, st)]
    for b in range(2):
        p, loc, lv, _ = R.instances(b, d[2], lvl, d[3], fg, matched, d[4], d[5], d[6])
        _, p0, p1 = CR.pre_activations(d[0][b:b + 1], p, loc, lv)
        assert min(float(p0.abs().min()), float(p1.abs().min())) > 1e-3
    a, b_, c = (t.to(DEV).requires_grad_(True) for t in d[:3])
    asg = (fg.to(DEV), matched.to(DEV), torch.zeros(fg.shape, device=DEV), fg.sum(dim=1).to(DEV))
    rest = (lvl.to(DEV), d[3].to(DEV), asg, d[4].to(DEV), d[5].to(DEV), d[6].to(DEV), r)
    assert torch.autograd.gradcheck(lambda x, y, z: ops.head_mask_loss(x, y, z, *rest)[0], (a, b_, c), eps=1e-6, atol=1e-7, rtol=1e-5,
                                    nondet_tol=0.0)


def bits(t):
    return None if t is None else t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def ragged_problem():
    """B 3 with an empty image in the middle, 9 x 13 coarse (ragged tiles), up_rate 4, 21 + 0 + 19 instances: more than one sub-range and pass"""
    A = 60
    rows = (tuple(range(0, 42, 2)), (), tuple(range(3, 60, 3)))
    return small_problem(33, B=3, H8=9, W8=13, r=4, A=A, M=5, fg_rows=rows)


def test_two_runs_are_bitwise_equal_and_one_sided_gradients_equal_the_full_call(ops):
    args = ragged_problem()
    keys = R.QUANTITIES[2:]
    for dtype in (torch.float32, torch.float64):
        a = hip_run(ops, *args, R.GRAD_OUT, dtype)
        b = hip_run(ops, *args, R.GRAD_OUT, dtype)
        assert all(torch.equal(bits(a[k]), bits(b[k])) for k in R.QUANTITIES)
        for i, k in enumerate(keys):
            need = tuple(j == i for j in range(3))
            one = hip_run(ops, *args, R.GRAD_OUT, dtype, need=need)
            assert all(one[q] is None for q in keys if q != k) and torch.equal(bits(one[k]), bits(a[k])), (dtype, k)
            assert torch.equal(bits(one["loss_condinst"]), bits(a["loss_condinst"]))
    want = R.loss_and_grads(*[t.double() if t.is_floating_point() else t for t in args[:10]], args[10], R.GRAD_OUT)
    hold(a, want, lambda k: 1e-12, "ragged batch")


def test_row_pitch_of_196_gives_the_bits_of_the_contiguous_call(ops):
    args = ragged_problem()
    for dtype in (torch.float32, torch.float64):
        a = hip_run(ops, *args, R.GRAD_OUT, dtype)
        b = hip_run(ops, *args, R.GRAD_OUT, dtype, pitch=196)
        assert all(torch.equal(bits(a[k]), bits(b[k])) for k in R.QUANTITIES)


def test_capacity_equal_to_the_count_gives_the_same_bits_and_one_less_gives_nan_and_zero_gradients(ops):
    args = ragged_problem()
    n = int(args[5].sum())
    assert n == 40
    for dtype in (torch.float32, torch.float64):
        a = hip_run(ops, *args, R.GRAD_OUT, dtype)
        b = hip_run(ops, *args, R.GRAD_OUT, dtype, capacity=n)
        assert all(torch.equal(bits(a[k]), bits(b[k])) for k in R.QUANTITIES)
        over = hip_run(ops, *args, R.GRAD_OUT, dtype, capacity=n - 1)
        assert bool(torch.isnan(over["loss_condinst"])) and bool(torch.isnan(over["per_image"]).all())
        for k in R.QUANTITIES[2:]:
            assert over[k].shape == a[k].shape and not over[k].any() and not torch.isnan(over[k]).any(), k


def headline_inputs(B, H8, W8, r, M, per_image, seed):
    """Synthetic inputs at the headline geometry with a planted assignment (per_image anchors per image in ascending order, each matched to a
    random box) and no hidden unit of a foreground instance on a ReLU kink: the bias of a unit that has a pixel with |pre-activation| <=
    KINK is moved by steps of 2^-10 until none has, layer 0 first (the rule and the reasoning of tests/test_condinst_loss_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    xs, ys, st = S.anchors(8 * H8, 8 * W8, DEV)
    A = xs.shape[0]
    mf, um = torch.randn(B, 8, H8, W8, generator=g).to(DEV), torch.randn(B, 9 * r * r, H8, W8, generator=g).to(DEV)
    dp = (0.35 * torch.randn(B, A, 169, generator=g)).to(DEV)
    lvl = torch.randint(0, 5, (B, A), generator=g).to(torch.int32).to(DEV)
    masks = torch.zeros(B, M, r * H8, r * W8)
    for b in range(B):
        for m in range(M):
            y0, x0 = int(torch.randint(0, r * H8 // 2, (1,), generator=g)), int(torch.randint(0, r * W8 // 2, (1,), generator=g))
            masks[b, m, y0:y0 + 8 + int(torch.randint(0, r * H8 // 2, (1,), generator=g)),
                  x0:x0 + 8 + int(torch.randint(0, r * W8 // 2, (1,), generator=g))] = 1
    fg = torch.zeros(B, A, dtype=torch.bool)
    for b in range(B):
        fg[b, torch.randperm(A, generator=g)[:per_image]] = True
    matched = torch.where(fg, torch.randint(0, M, (B, A), generator=g), torch.full((B, A), -1))
    fg, matched, masks = fg.to(DEV), matched.to(DEV), masks.to(DEV)
    for b in range(B):
        rows = fg[b].nonzero()[:, 0]
        for layer, cols in ((0, slice(152, 160)), (1, slice(160, 168))):
            for _ in range(200):
                p, loc, lv, _ = R.instances(b, dp.double(), lvl, masks[:, :, :1, :1], fg, matched, xs.double(), ys.double(), st.double())
                pre = CR.pre_activations(mf[b:b + 1].double(), p, loc, lv)[1 + layer]
                bad = (pre.abs() <= KINK).any(dim=2)
                if not bool(bad.any()):
                    break
                dp[b, rows, cols] += bad.float() * 2.0 ** -10
            assert not bool(bad.any())
    return mf, um, dp, lvl, masks, fg, matched, xs, ys, st, r


def test_headline_800x1280_b2_r4_100_instances_per_image_without_a_sync_or_a_gather(ops):
    B, H8, W8, r, M, per_image = 2, 100, 160, 4, 10, 100
    args = headline_inputs(B, H8, W8, r, M, per_image, 17)
    mf, um, dp, lvl, masks, fg, matched, xs, ys, st, _ = args
    assert dp.shape == (B, 21000, 169) and int(fg.sum()) == B * per_image
    for b in range(B):                                    # fp32 and fp64 take the same ReLU branches, with a margin
        p, loc, lv, _ = R.instances(b, dp, lvl, masks[:, :, :1, :1], fg, matched, xs, ys, st)
        _, a0, a1 = CR.pre_activations(mf[b:b + 1].double(), p.double(), loc.double(), lv)
        _, b0, b1 = CR.pre_activations(mf[b:b + 1], p, loc, lv)
        assert min(float(a0.abs().min()), float(a1.abs().min())) > KINK and torch.equal(a0 > 0, b0 > 0) and torch.equal(a1 > 0, b1 > 0)
        assert max(float((a0 - b0).abs().max()), float((a1 - b1).abs().max())) < KINK / 2
        del a0, a1, b0, b1
    d64 = [t.double() if t.is_floating_point() else t for t in args[:10]]
    r64 = R.loss_and_grads(*d64, r, R.GRAD_OUT, chunk=10)
    r32 = R.loss_and_grads(*args[:10], r, R.GRAD_OUT, chunk=10)
    del d64
    asg = (fg, matched, torch.zeros(fg.shape, device=DEV), fg.sum(dim=1))

    def run():
        a, b_, c = (t.requires_grad_(True) for t in (mf, um, dp))
        a.grad = b_.grad = c.grad = None
        loss, per = ops.head_mask_loss(a, b_, c, lvl, masks, asg, xs[None], ys[None], st[None], r)       # default capacity B min(A, 10 M) = 200
        (loss * R.GRAD_OUT).backward()
        return {"loss_condinst": loss.detach(), "per_image": per, "g_mask_feats": a.grad, "g_up_masks": b_.grad, "g_dynamic_params": c.grad}
    hip_run(ops, *small_problem(21), R.GRAD_OUT)                                                          # library, allocator and kernels warm
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = run()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base              # the three dense gradients included
    one_map = B * per_image * r * H8 * r * W8 * 4
    print("headline: peak memory rise over forward + backward %.1f MB; one (N, rH8, rW8) fp32 map: %.1f MB" % (rise / 1e6, one_map / 1e6))
    got = {k: v.clone() for k, v in got.items()}
    hold(got, r64, lambda k: R.bound32(R.rel_err(r32[k], r64[k])), "headline")
    assert rise < one_map, "forward + backward allocated %.1f MB: a full-resolution per-instance tensor (%.1f MB) was materialised" % (
        rise / 1e6, one_map / 1e6)
    # No-sync check by a busy stream (the method of tests/test_head_loss_gpu.py): a calibrated spin kernel of ~0.2 s is queued, an event behind
    # it, then forward and backward.  Both must return while the event is still pending; set_sync_debug_mode("error") holds torch's own
    # operators as well.
    del got
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    torch.cuda._sleep(1000000)
    b.record()
    b.synchronize()
    cycles = int(200.0 / max(a.elapsed_time(b), 1e-3) * 1000000)
    behind_spin = torch.cuda.Event()
    torch.cuda._sleep(cycles)
    behind_spin.record()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t0 = time.perf_counter()
        again = run()
        host_ms = (time.perf_counter() - t0) * 1e3
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pending = not behind_spin.query()
    torch.cuda.synchronize()
    print("forward + backward returned after %.2f ms on the host; spin kernel of %d cycles still running: %s" % (host_ms, cycles, pending))
    assert pending, "head_mask_loss / backward waited for the stream (%.1f ms on the host)" % host_ms
    hold(again, r64, lambda k: R.bound32(R.rel_err(r32[k], r64[k])), "headline behind the spin kernel")
