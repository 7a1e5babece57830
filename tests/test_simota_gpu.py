"""uni_simota_assign through ops.simota_assign / ops.simota_assign_batch on the GPU: exact equality with the fixtures the reference's own
get_assignments produced (tests/golden/simota_*.npz; decisions exact, the matched IoU within 4 x the stored fp32-vs-fp64 deviation), bitwise
repeatability, the invariants of an assignment, the headline geometry against the fp32 restatement on the same GPU -- after the fp64
restatement has shown that no decision of the draw sits inside the fixtures' margins -- with a check that the batched wrapper returns
while the stream is still busy, and the memory condition (no boxes x anchors x classes tensor)."""
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import simota_ref as R  # noqa: E402

DEV = "cuda"
HEADLINE = (800, 1280, 100, 1, 0)      # H, W, G, C, seed: chosen on the CPU so that the fp64 restatement shows no decision inside the margin


@pytest.fixture(scope="module")
def ops():
    from unicorn_amd import _lib, ops as o
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def dev(ts):
    return [t.to(DEV) for t in ts]


def single(ops, c, sfx, H, W, C):
    ins = dev(torch.from_numpy(c[n + sfx]) for n in R.INPUTS)
    xs, ys, st = R.anchors(H, W, DEV)
    return ops.simota_assign(*ins, xs[None], ys[None], st[None], (H, W), C)


def hold_to_fixture(got, c, sfx):
    classes, fg, ious, inds, num_fg = got
    assert isinstance(num_fg, int) and num_fg == int(c["num_fg" + sfx])
    assert fg.dtype == torch.bool and np.array_equal(fg.cpu().numpy(), c["fg_mask" + sfx])
    assert inds.dtype == torch.int64 and np.array_equal(inds.cpu().numpy(), c["matched_gt_inds" + sfx])
    assert np.array_equal(classes.cpu().numpy(), c["gt_matched_classes" + sfx])
    err = float(np.abs(ious.cpu().numpy().astype(np.float64) - c["pred_ious_this_matching" + sfx]).max())
    print("max |matched iou - fixture| %.3g, bound %.3g" % (err, 4 * float(c["margin_iou_dev" + sfx])))
    assert err <= 4 * float(c["margin_iou_dev" + sfx]), err


@pytest.mark.parametrize("tag", sorted(t for t in R.CASES if len(R.CASES[t][2]) == 1))
def test_fixture_exact(ops, tag):
    H, W, _, C, _ = R.CASES[tag]
    c = R.load_case(tag)
    hold_to_fixture(single(ops, c, "", H, W, C), c, "")


def test_batch_fixture_exact_and_equal_to_per_image_calls(ops):
    H, W, Gs, C, _ = R.CASES["batch"]
    c = R.load_case("batch")
    xs, ys, st = R.anchors(H, W, DEV)
    fg, inds, ious, num_fg = ops.simota_assign_batch(torch.from_numpy(c["outputs"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV), xs, ys[None],
                                                     st, (H, W), C)
    assert fg.dtype == torch.bool and inds.dtype == torch.int64 and ious.dtype == torch.float32 and num_fg.is_cuda
    assert fg.shape == inds.shape == ious.shape == (3, xs.shape[0]) and num_fg.shape == (3,)
    for b, G in enumerate(Gs):
        if G == 0:                                                  # an image without a box: everything background, everything written
            assert not fg[b].any() and bool((inds[b] == -1).all()) and not ious[b].any() and int(num_fg[b]) == 0
            continue
        sfx = "_%d" % b
        per_image = single(ops, c, sfx, H, W, C)
        hold_to_fixture(per_image, c, sfx)
        hold_to_fixture((torch.from_numpy(c["gt_classes" + sfx]).to(DEV)[inds[b][fg[b]]], fg[b], ious[b][fg[b]], inds[b][fg[b]], int(num_fg[b])), c, sfx)
        assert torch.equal(fg[b], per_image[1]) and torch.equal(inds[b][fg[b]], per_image[3]) and torch.equal(ious[b][fg[b]], per_image[2])
        assert bool((inds[b][~fg[b]] == -1).all()) and not ious[b][~fg[b]].any()
    empty = ops.simota_assign(*dev(torch.from_numpy(c[n + "_0"]) for n in R.INPUTS[:3]), torch.zeros(0, 4, device=DEV), torch.zeros(0, device=DEV),
                              xs, ys, st, (H, W), C)                # G == 0: empty results without a call
    assert empty[0].shape == (0,) and not empty[1].any() and empty[2].shape == (0,) and empty[3].shape == (0,) and empty[4] == 0


def test_two_runs_are_bitwise_equal(ops):
    H, W, _, C, _ = R.CASES["crowd"]
    c = R.load_case("crowd")
    a, b = single(ops, c, "", H, W, C), single(ops, c, "", H, W, C)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x.view(torch.uint8) if x.dtype == torch.bool else x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.uint8) if y.dtype == torch.bool else y.view(torch.int32) if y.dtype == torch.float32 else y)
    assert a[4] == b[4]
    H, W, _, C, _ = R.CASES["batch"]
    c = R.load_case("batch")
    args = (torch.from_numpy(c["outputs"]).to(DEV), torch.from_numpy(c["labels"]).to(DEV), *R.anchors(H, W, DEV), (H, W), C)
    for x, y in zip(ops.simota_assign_batch(*args), ops.simota_assign_batch(*args)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)


def test_invariants_256x416_g40(ops):
    H, W, G, C = 256, 416, 40, 3
    ins = dev(R.draw(H, W, G, C, 0, "mot"))
    xs, ys, st = R.anchors(H, W, DEV)
    labels = torch.cat([ins[4][:, None], ins[3]], 1)[None]
    fg, inds, ious, num_fg = ops.simota_assign_batch(torch.cat(ins[:3], 1)[None], labels, xs, ys, st, (H, W), C)
    fg, inds, ious = fg[0], inds[0], ious[0]
    # every fg anchor has exactly one box, inside [0, G); background has none
    assert int(num_fg[0]) == int(fg.sum()) > 0
    assert bool(((inds >= 0) == fg).all()) and bool((inds[fg] < G).all()) and bool((inds[~fg] == -1).all())
    # a matched IoU may be zero: a box with few candidates takes an anchor whose prediction does not overlap it (the reference does the same)
    assert bool((ious[fg] >= 0).all()) and bool((ious[fg] <= 1).all()) and not ious[~fg].any()
    r = R.assign(*ins, xs, ys, st, (H, W), C)
    assert bool((fg <= r["cand"]).all()), "a matched anchor that is no geometry candidate"
    # every box with an anchor inside box-and-centre owns an anchor, or lost each of its selections to a cheaper box
    owned = torch.zeros(G, dtype=torch.bool, device=DEV)
    owned[inds[fg]] = True
    cand_idx = r["cand"].nonzero()[:, 0]
    owner_of_cand = inds[cand_idx]
    for g in range(G):
        if not bool(r["both"][g].any()) or bool(owned[g]):
            continue
        sel = r["selected"][g].nonzero()[:, 0]
        assert sel.numel() >= 1
        for j in sel.tolist():
            o = int(owner_of_cand[j])
            assert o >= 0 and o != g and float(r["cost"][o, j]) <= float(r["cost"][g, j]), (g, j, o)
    own = ops.simota_assign(*ins, xs, ys, st, (H, W), C)
    assert torch.equal(own[1], fg) and torch.equal(own[3], inds[fg]) and own[4] == int(num_fg[0])


def test_headline_800x1280_g100_exact_and_without_a_sync(ops):
    H, W, G, C, seed = HEADLINE
    ins = dev(R.draw(H, W, G, C, seed, "mot"))
    xs, ys, st = R.anchors(H, W, DEV)
    assert xs.shape[0] == 21000
    # first, from the restatement alone: no decision of this draw sits inside the fixtures' margins
    m, r32, r64 = R.margins_of(*ins, xs, ys, st, (H, W), C)
    print({k: ("%.3g" % v if isinstance(v, float) else v) for k, v in m.items()})
    assert m["ok"] and m["min_gap_ratio"] > R.MARGIN and m["ksum_margin"] > R.MARGIN * 10 * m["iou_dev"] and m["min_abs_delta"] > R.MIN_DELTA, m
    assert torch.equal(r32["matching"], r64["matching"]) and int(r64["contested"].sum()) >= 1 and r32["num_fg"] >= G
    outputs, labels = torch.cat(ins[:3], 1)[None].contiguous(), torch.cat([ins[4][:, None], ins[3]], 1)[None].contiguous()
    ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)                  # library, allocator and kernels warm
    torch.cuda.synchronize()
    # No-sync check by a busy stream: a spin kernel of ~0.2 s (calibrated first, its clock rate is the device's business) is queued, an event
    # behind it, then the wrapper.  The wrapper must return while the event is still pending: a host synchronisation anywhere inside --
    # torch or the library -- would have waited for the spin kernel.  set_sync_debug_mode("error") holds torch's own operators as well.
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
        fg, inds, ious, num_fg = ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)
        host_ms = (time.perf_counter() - t0) * 1e3
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pending = not behind_spin.query()
    torch.cuda.synchronize()
    print("wrapper returned after %.2f ms on the host; spin kernel of %d cycles still running: %s" % (host_ms, cycles, pending))
    assert pending, "simota_assign_batch waited for the stream (%.1f ms on the host)" % host_ms
    # exact equality with the fp32 restatement on this GPU
    fg, inds, ious = fg[0], inds[0], ious[0]
    assert int(num_fg[0]) == r32["num_fg"]
    assert torch.equal(fg, r32["fg_mask"]) and torch.equal(inds[fg], r32["matched_gt_inds"])
    err = float((ious[fg].double() - r64["pred_ious_this_matching"]).abs().max())
    print("max |matched iou - fp64| %.3g, bound %.3g" % (err, 4 * m["iou_dev"]))
    assert err <= 4 * m["iou_dev"]
    own = ops.simota_assign(*ins, xs[None], ys[None], st[None], (H, W), C)
    assert own[4] == r32["num_fg"] and torch.equal(own[1], fg) and torch.equal(own[3], r32["matched_gt_inds"])
    assert torch.equal(own[0], r32["gt_matched_classes"]) and torch.equal(own[2], ious[fg])


def test_memory_800x1280_g64_c80(ops):
    H, W, G, C = 800, 1280, 64, 80
    ins = dev(R.draw(H, W, G, C, 0, "mot"))
    xs, ys, st = R.anchors(H, W, DEV)
    outputs, labels = torch.cat(ins[:3], 1)[None].contiguous(), torch.cat([ins[4][:, None], ins[3]], 1)[None].contiguous()
    gac = G * xs.shape[0] * C * 4                                   # one (G, A, C) fp32 tensor: 430 MB
    assert gac == 430080000
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.simota_assign_batch(outputs, labels, xs, ys, st, (H, W), C)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak allocation rise %.1f MB, limit %.1f MB" % (rise / 1e6, gac / 8 / 1e6))
    assert rise < gac // 8, rise
    assert int(out[3][0]) == int(out[0].sum()) > 0
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    own = ops.simota_assign(*ins, xs, ys, st, (H, W), C)             # the per-image form builds the (A, 5 + C) rows as well
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < gac // 8 and own[4] == int(out[3][0])
