"""uni_head_loss_fwd / _bwd through ops.HeadLossFunction and ops.head_det_loss on the GPU: every fixture that the reference's own get_losses
produced (tests/golden/head_loss_*.npz) in fp64 within 1e-12 of scale and in fp32 -- assignment included -- within 4 x max(the reference's
own fp32-vs-fp64 deviation, one fp32 ulp); planted cases (all four edges tie, one touching edge, C = 80, a ragged batch with an empty image,
a class beyond C) against the restatement (tests/head_loss_ref.py) on the same GPU in fp64; gradcheck; bitwise repeatability; one-sided
gradients; a row pitch on `outputs`; and the headline geometry with a check that forward and backward return while the stream is busy."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import head_loss_ref as R  # noqa: E402
import simota_ref as S  # noqa: E402

DEV = "cuda"
TAGS = sorted(R.CASES)


@pytest.fixture(scope="module")
def ops():
    from unicorn_amd import _lib, ops as o
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def num_gt_of(labels):
    return (labels.sum(dim=2) > 0).sum(dim=1).to(torch.int32)


def hip_run(ops, outputs, origin, labels, fg, matched, iou, xs, ys, st, grad_out, dtype, need=(True, True), num_gt=None, reg_weight=5.0):
    """HeadLossFunction with its backward on the planted assignment -> the seven quantities like R.run (a gradient not asked for: None)"""
    o = outputs.to(device=DEV, dtype=dtype).clone().requires_grad_(need[0])
    g = None if origin is None else origin.to(device=DEV, dtype=dtype).clone().requires_grad_(need[1])
    lab, iou_, xs_, ys_, st_ = (t.to(device=DEV, dtype=dtype) for t in (labels, iou, xs, ys, st))
    fg_ = fg.to(DEV)
    res = ops.HeadLossFunction.apply(o, g, lab, fg_.to(torch.uint8), matched.to(DEV).to(torch.int32), iou_, fg_.sum(1).to(torch.int32),
                                     num_gt_of(lab) if num_gt is None else num_gt, xs_, ys_, st_, reg_weight)
    assert res.shape == (5,) and res.dtype == dtype
    w = torch.tensor([float(v) for v in grad_out] + [0.0], device=DEV, dtype=dtype)
    (res * w).sum().backward()
    out = {k: res[i].detach() for i, k in enumerate(R.QUANTITIES[:5])}
    out["grad_outputs"], out["grad_origin"] = o.grad, None if g is None else g.grad
    return out


def fixture_inputs(c):
    H, W, C = (int(v) for v in c["shape"])
    origin = torch.from_numpy(c["origin_preds"]) if bool(c["use_l1"]) else None
    return (H, W, C), torch.from_numpy(c["outputs"]), origin, torch.from_numpy(c["labels"]), S.anchors(H, W)


def hold(got, want, bound_of, what):
    for k in R.QUANTITIES:
        if want.get(k) is None:
            assert got[k] is None, k
            continue
        e, b = R.rel_err(got[k], want[k]), bound_of(k)
        print("%s %-12s err %.3g  bound %.3g" % (what, k, e, b))
        assert e <= b, (what, k, e, b)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp64(ops, tag):
    c = R.load_case(tag)
    _, outputs, origin, labels, (xs, ys, st) = fixture_inputs(c)
    got = hip_run(ops, outputs, origin, labels, torch.from_numpy(c["fg_mask"]), torch.from_numpy(c["matched_gt_inds"]),
                  torch.from_numpy(c["matched_ious"]), xs, ys, st, c["grad_out"], torch.float64)
    hold(got, {k: c.get(k) for k in R.QUANTITIES}, lambda k: 1e-12, tag)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp32_through_head_det_loss_with_its_own_assignment(ops, tag):
    c = R.load_case(tag)
    (H, W, C), outputs, origin, labels, (xs, ys, st) = fixture_inputs(c)
    o = outputs.to(DEV).requires_grad_(True)
    g = None if origin is None else origin.to(DEV).requires_grad_(True)
    losses, (fg, matched, iou, num_fg) = ops.head_det_loss(o, g, labels.to(DEV), xs.to(DEV)[None], ys.to(DEV)[None], st.to(DEV)[None], (H, W), C)
    assert torch.equal(fg.cpu(), torch.from_numpy(c["fg_mask"])) and torch.equal(matched.cpu(), torch.from_numpy(c["matched_gt_inds"]))
    assert torch.equal(num_fg.cpu(), torch.from_numpy(c["num_fg_per_image"]))
    assert all(losses[k].shape == () and losses[k].is_cuda and losses[k].dtype == torch.float32 for k in R.QUANTITIES[:5] + ("total_loss",))
    assert torch.equal(losses["total_loss"], losses["iou_loss"] + losses["conf_loss"] + losses["cls_loss"] + losses["l1_loss"])
    assert not losses["num_fg"].requires_grad
    R.weighted(losses, [float(v) for v in c["grad_out"]]).backward()
    got = {k: losses[k].detach() for k in R.QUANTITIES[:5]}
    got["grad_outputs"], got["grad_origin"] = o.grad, None if g is None else g.grad
    hold(got, {k: c.get(k) for k in R.QUANTITIES}, lambda k: R.bound32(c[k + "_fp32_ref_err"]), tag)
    if tag == "empty":
        assert not o.grad[:, :, :4].any() and not o.grad[:, :, 5:].any() and not g.grad.any() and float(losses["num_fg"]) == 1.0
        assert bool(o.grad[:, :, 4].all())
    if tag == "batch_nol1":
        assert g is None and float(losses["l1_loss"]) == 0.0 and not losses["l1_loss"].requires_grad


def drawn(ops, H, W, C, Gs, seed, M=None):
    """a batch of synthetic images (simota_ref.draw) with the assignment the operator itself reaches: outputs, origin, labels (B, M, 5),
    fg, matched, iou and the anchors, fp32 on the CPU"""
    M = max(max(Gs), 1) if M is None else M
    outs, labels = [], torch.zeros(len(Gs), M, 5)
    for b, G in enumerate(Gs):
        bbox, obj, cls, gtb, gtc = S.draw(H, W, G, C, seed + b)
        outs.append(torch.cat([bbox, obj, cls], 1))
        labels[b, :G] = torch.cat([gtc[:, None], gtb], 1)
    outputs = torch.stack(outs)
    xs, ys, st = S.anchors(H, W)
    fg, matched, iou, _ = ops.simota_assign_batch(outputs.to(DEV), labels.to(DEV), xs.to(DEV), ys.to(DEV), st.to(DEV), (H, W), C)
    origin = torch.randn(outputs.shape[0], outputs.shape[1], 4, generator=torch.Generator().manual_seed(seed + 99))
    return outputs, origin, labels, fg.cpu(), matched.cpu(), iou.cpu(), (xs, ys, st)


def against_restatement(ops, outputs, origin, labels, fg, matched, iou, anchors, what, grad_out=R.GRAD_OUT):
    want = R.run(outputs, origin, labels, fg, matched, iou, *anchors, grad_out, torch.float64, device=DEV)
    got = hip_run(ops, outputs, origin, labels, fg, matched, iou, *anchors, grad_out, torch.float64)
    hold(got, want, lambda k: 1e-12, what)
    return got, want


def test_planted_prediction_equal_to_its_box_splits_the_gradient(ops):
    outputs, origin, labels, fg, matched, iou, anchors = drawn(ops, 32, 32, 3, (2,), 5)
    a = int(fg[0].nonzero()[0])
    labels[0, int(matched[0, a]), 1:5] = torch.tensor([10.0, 12.0, 8.0, 6.0])       # edges 6, 9, 14, 15: exact in every precision
    outputs[0, a, :4] = labels[0, int(matched[0, a]), 1:5]
    got, want = against_restatement(ops, outputs, origin, labels, fg, matched, iou, anchors, "four ties")
    # iou = 1 is the maximum: with the halves of torch's maximum / minimum the box gradient vanishes; an unsplit gradient (all of it to the
    # prediction, or none) would leave -+ 2 reg_weight g_iou / (n w) in the size columns
    scale = 2 * 5.0 * R.GRAD_OUT[0] / max(int(fg.sum()), 1) / 8.0
    assert float(got["grad_outputs"][0, a, :4].abs().max()) <= 1e-12 * scale and float(want["grad_outputs"][0, a, :4].abs().max()) <= 1e-12 * scale


def test_planted_prediction_touching_its_box_in_one_edge_has_no_box_gradient(ops):
    outputs, origin, labels, fg, matched, iou, anchors = drawn(ops, 32, 32, 3, (2,), 6)
    a = int(fg[0].nonzero()[0])
    labels[0, int(matched[0, a]), 1:5] = torch.tensor([12.0, 12.0, 8.0, 6.0])       # left edge 8
    outputs[0, a, :4] = torch.tensor([4.0, 12.0, 8.0, 6.0])                         # right edge 8: tl == br, en = 0
    got, _ = against_restatement(ops, outputs, origin, labels, fg, matched, iou, anchors, "touching edge")
    assert not got["grad_outputs"][0, a, :4].any()


def test_planted_c80_with_21_anchors(ops):
    outputs, origin, labels, fg, matched, iou, anchors = drawn(ops, 32, 32, 80, (1,), 7)
    assert outputs.shape[1] == 21
    fg, matched, iou = torch.zeros_like(fg), torch.full_like(matched, -1), torch.zeros_like(iou)
    for a, v in ((2, 0.8), (17, 0.25), (20, 0.0)):                                   # three foreground anchors, the last in the last lane used
        fg[0, a], matched[0, a], iou[0, a] = True, 0, v
    labels[0, 0, 0] = 70.0                                                           # a class in the second 64 of the wave's class loop
    against_restatement(ops, outputs, origin, labels, fg, matched, iou, anchors, "C = 80")


def test_planted_ragged_batch_with_an_empty_image(ops):
    outputs, origin, labels, fg, matched, iou, anchors = drawn(ops, 96, 160, 3, (5, 0, 7), 8)
    assert outputs.shape[:2] == (3, 315) and int(fg[0].sum()) > 0 and int(fg[1].sum()) == 0 and int(fg[2].sum()) > 0
    got, _ = against_restatement(ops, outputs, origin, labels, fg, matched, iou, anchors, "B = 3, A = 315")
    assert not got["grad_outputs"][1][:, :4].any() and not got["grad_outputs"][1][:, 5:].any() and not got["grad_origin"][1].any()
    against_restatement(ops, outputs, None, labels, fg, matched, iou, anchors, "B = 3, A = 315, no L1")


def test_planted_class_beyond_c_is_clamped(ops):
    C = 3
    outputs, origin, labels, fg, matched, iou, anchors = drawn(ops, 32, 32, C, (2,), 9)
    labels[0, :, 0] = C + 2
    got, _ = against_restatement(ops, outputs, origin, labels, fg, matched, iou, anchors, "class C + 2")
    labels[0, :, 0] = C - 1
    same = hip_run(ops, outputs, origin, labels, fg, matched, iou, *anchors, R.GRAD_OUT, torch.float64)
    assert all(torch.equal(got[k], same[k]) for k in R.QUANTITIES)


def test_gradcheck_fp64(ops):
    C = 3
    outputs, origin, labels, fg, matched, iou, (xs, ys, st) = drawn(ops, 32, 32, C, (2,), 11)
    assert outputs.shape[1] == 21 and int(fg.sum()) >= 2
    # no foreground anchor within 1e-3 of a kink (an edge tie, an empty intersection on the turn, a zero L1 residual): asserted, not filtered
    rows = R.matched_rows(labels.double(), fg, matched)
    pred = outputs.double()[:, :, :4].reshape(-1, 4)[fg.reshape(-1)]
    _, tl, br = R.iou_of(pred, rows[:, 1:5])
    edges = lambda b: torch.cat([b[:, :2] - b[:, 2:] / 2, b[:, :2] + b[:, 2:] / 2], 1)      # noqa: E731
    e = [t.double().reshape(1, -1).expand(1, 21)[fg] for t in (st, xs, ys)]
    resid = origin.double().reshape(-1, 4)[fg.reshape(-1)] - R.l1_target(rows[:, 1:5], *e)
    assert float((edges(pred) - edges(rows[:, 1:5])).abs().min()) > 1e-3 and float((br - tl).abs().min()) > 1e-3 and float(resid.abs().min()) > 1e-3
    o = outputs.double().to(DEV).requires_grad_(True)
    g = origin.double().to(DEV).requires_grad_(True)
    lab, iou_, xs_, ys_, st_ = (t.double().to(DEV) for t in (labels, iou, xs, ys, st))
    fg_ = fg.to(DEV)
    rest = (lab, fg_.to(torch.uint8), matched.to(DEV).to(torch.int32), iou_, fg_.sum(1).to(torch.int32), num_gt_of(lab), xs_, ys_, st_, 5.0)
    assert torch.autograd.gradcheck(lambda a, b: ops.HeadLossFunction.apply(a, b, *rest)[:4], (o, g), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


def bits(t):
    return None if t is None else t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def test_two_runs_are_bitwise_equal_and_one_sided_gradients_equal_the_two_sided(ops):
    outputs, origin, labels, fg, matched, iou, anchors = drawn(ops, 96, 160, 3, (5, 0, 7), 12)
    for dtype in (torch.float32, torch.float64):
        a = hip_run(ops, outputs, origin, labels, fg, matched, iou, *anchors, R.GRAD_OUT, dtype)
        b = hip_run(ops, outputs, origin, labels, fg, matched, iou, *anchors, R.GRAD_OUT, dtype)
        assert all(torch.equal(bits(a[k]), bits(b[k])) for k in R.QUANTITIES)
        only_o = hip_run(ops, outputs, origin, labels, fg, matched, iou, *anchors, R.GRAD_OUT, dtype, need=(True, False))
        only_g = hip_run(ops, outputs, origin, labels, fg, matched, iou, *anchors, R.GRAD_OUT, dtype, need=(False, True))
        assert only_o["grad_origin"] is None and torch.equal(bits(only_o["grad_outputs"]), bits(a["grad_outputs"]))
        assert only_g["grad_outputs"] is None and torch.equal(bits(only_g["grad_origin"]), bits(a["grad_origin"]))


def test_row_pitch_on_outputs_gives_the_same_bits(ops):
    C = 3
    outputs, origin, labels, fg, matched, iou, (xs, ys, st) = drawn(ops, 96, 160, C, (5, 0, 7), 13)
    B, A = outputs.shape[:2]
    wide = torch.full((B, A, 5 + C + 3), float("nan"), device=DEV)
    wide[:, :, :5 + C] = outputs.to(DEV)
    wide.requires_grad_(True)
    view = wide[:, :, :5 + C]
    assert view.stride() == ((5 + C + 3) * A, 5 + C + 3, 1)
    plain = outputs.to(DEV).requires_grad_(True)
    res = []
    for o in (view, plain):
        losses, _ = ops.head_det_loss(o, origin.to(DEV), labels.to(DEV), xs.to(DEV), ys.to(DEV), st.to(DEV), (96, 160), C)
        R.weighted(losses, R.GRAD_OUT).backward()
        res.append(losses)
    assert all(torch.equal(bits(res[0][k]), bits(res[1][k])) for k in R.QUANTITIES[:5])
    assert torch.equal(bits(wide.grad[:, :, :5 + C]), bits(plain.grad)) and not wide.grad[:, :, 5 + C:].any()


def test_headline_800x1280_b2_c80_g100_and_without_a_sync(ops):
    H, W, C, G = 800, 1280, 80, 100
    outs, labels = [], torch.zeros(2, G, 5)
    for b in range(2):
        bbox, obj, cls, gtb, gtc = S.draw(H, W, G, C, 40 + b, "mot")
        outs.append(torch.cat([bbox, obj, cls], 1))
        labels[b] = torch.cat([gtc[:, None], gtb], 1)
    outputs, labels = torch.stack(outs).to(DEV), labels.to(DEV)
    xs, ys, st = S.anchors(H, W, DEV)
    assert outputs.shape == (2, 21000, 85)
    origin = torch.randn(2, 21000, 4, generator=torch.Generator().manual_seed(3)).to(DEV)
    assignment = ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)
    fg, matched, iou, num_fg = assignment
    assert int(num_fg.sum()) >= 2 * G
    # the restatement on this GPU in both precisions: its own fp32-vs-fp64 deviation is the reference term of the bound
    r64 = R.run(outputs, origin, labels, fg, matched, iou, xs, ys, st, R.GRAD_OUT, torch.float64, device=DEV)
    r32 = R.run(outputs, origin, labels, fg, matched, iou, xs, ys, st, R.GRAD_OUT, torch.float32, device=DEV)
    o, g = outputs.clone().requires_grad_(True), origin.clone().requires_grad_(True)
    losses, _ = ops.head_det_loss(o, g, labels, xs, ys, st, (H, W), C)                # library, allocator and kernels warm
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    # No-sync check by a busy stream (the method of tests/test_simota_gpu.py): a calibrated spin kernel of ~0.2 s is queued, an event behind
    # it, then forward and backward.  Both must return while the event is still pending; set_sync_debug_mode("error") holds torch's own
    # operators as well.
    o.grad = g.grad = None
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
        losses, own = ops.head_det_loss(o, g, labels, xs, ys, st, (H, W), C)
        R.weighted(losses, R.GRAD_OUT).backward()
        host_ms = (time.perf_counter() - t0) * 1e3
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pending = not behind_spin.query()
    torch.cuda.synchronize()
    print("forward + backward returned after %.2f ms on the host; spin kernel of %d cycles still running: %s" % (host_ms, cycles, pending))
    assert pending, "head_det_loss / backward waited for the stream (%.1f ms on the host)" % host_ms
    assert all(torch.equal(x, y) for x, y in zip(own, assignment))
    got = {k: losses[k].detach() for k in R.QUANTITIES[:5]}
    got["grad_outputs"], got["grad_origin"] = o.grad, g.grad
    hold(got, r64, lambda k: R.bound32(R.rel_err(r32[k], r64[k])), "headline")
    # the assignment handed in gives the same bits as the one computed inside
    o2, g2 = outputs.clone().requires_grad_(True), origin.clone().requires_grad_(True)
    again, _ = ops.head_det_loss(o2, g2, labels, xs, ys, st, (H, W), C, assignment=assignment)
    R.weighted(again, R.GRAD_OUT).backward()
    assert all(torch.equal(bits(again[k]), bits(losses[k])) for k in R.QUANTITIES[:5]) and torch.equal(bits(o2.grad), bits(o.grad))
    assert torch.equal(bits(g2.grad), bits(g.grad))
