"""uni_head_assemble_fwd / _bwd through ops.head_assemble / ops.HeadAssembleFunction on the GPU: every fixture that the reference's own lines
produced (tests/golden/head_assemble_*.npz), from NCHW and from channels-last maps -- columns 0, 1, 4 and up of outputs, origin_preds, the
shifts, strides, levels, dynamic_params and the gradients of obj, cls, ctrl and reg[0:2] BIT-equal to the fp32 fixture, the two exp columns
and the gradient of reg[2:4] within 4 x the recorded fp32-vs-fp64 deviation of the reference; the fp64 entries within 1e-12 and under
gradcheck; half maps bit-equal to the fp32 operator on the widened maps; gradient subsets, unused results, use_l1 False; the saved tensors;
bitwise repeatability; no host synchronisation; and the chain head_assemble -> head_det_loss -> head_mask_loss against the eager assembly."""
import os
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import head_assemble_ref as R  # noqa: E402
import head_mask_loss_ref as HM  # noqa: E402

DEV = "cuda"
TAGS = sorted(R.CASES)
CL = torch.channels_last
NCHW = torch.contiguous_format


@pytest.fixture(scope="module")
def ops():
    from unicorn_amd import _lib, ops as o
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return o


def hip_run(ops, p, dtype, fmt=NCHW, need=(True, True, True, True), use=("outputs", "origin_preds", "dynamic_params"), use_l1=True):
    """ops.head_assemble with its backward -> dict like R.run (a gradient not asked for or not reached: None); need: which roles require a
    gradient; use: which results enter the scalar that is differentiated"""
    maps = R.leaves(p, dtype, DEV, fmt)
    for ts, n in zip(maps, need):
        for t in ts or ():
            t.requires_grad_(n)
    reg, obj, cls, ctrl = maps
    res = ops.head_assemble(reg, obj, cls, p["strides"], ctrl, use_l1=use_l1)
    s = 0
    for i, k, g in ((0, "outputs", "g_outputs"), (1, "origin_preds", "g_origin"), (5, "dynamic_params", "g_params")):
        if k in use and res[i] is not None and res[i].requires_grad:
            s = s + (res[i] * p[g].to(device=DEV, dtype=res[i].dtype)).sum()
    if torch.is_tensor(s):
        s.backward()
    out = {k: (None if t is None else t.detach()) for k, t in zip(R.RESULTS, res)}
    out["_res"] = res
    for m, ts in zip(R.MAPS, maps):
        for k, t in enumerate(ts or ()):
            out["grad_%s_%d" % (m, k)] = t.grad
    return out


def grad_names(p, roles=R.MAPS):
    return ["grad_%s_%d" % (m, k) for m in roles if p[m] is not None for k in range(len(p["levels"]))]


def all_bits_equal(a, b, names):
    for k in names:
        assert (a[k] is None) == (b[k] is None), k
        assert a[k] is None or R.bits_equal(a[k], b[k]), k


@pytest.mark.parametrize("fmt", [NCHW, CL], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp32(ops, tag, fmt):
    c, p = R.load_case(tag), R.problem(tag)
    got = hip_run(ops, p, torch.float32, fmt)
    B, A, L = p["B"], p["A"], len(p["levels"])
    o, want = got["outputs"].cpu(), torch.from_numpy(c["outputs_fp32"])
    assert o.shape == (B, A, 5 + p["C"]) and o.dtype == torch.float32
    assert R.bits_equal(o[..., :2], want[..., :2]) and R.bits_equal(o[..., 4:], want[..., 4:])
    e, bound = R.rel_err(o[..., 2:4], c["outputs"][..., 2:4]), 4 * float(c["outputs_exp_fp32_ref_err"])
    print("%s outputs[2:4] err %.3g bound %.3g" % (tag, e, bound))
    assert e <= bound, (e, bound)
    for k in ("origin_preds", "x_shifts", "y_shifts", "expanded_strides"):
        assert R.bits_equal(got[k], c[k + "_fp32"]), k
    if p["P"]:
        assert R.bits_equal(got["dynamic_params"], c["dynamic_params_fp32"])
        assert got["fpn_levels"].dtype == torch.int32 and torch.equal(got["fpn_levels"].cpu().long(), torch.from_numpy(c["fpn_levels_fp32"]))
    else:
        assert got["dynamic_params"] is None and got["fpn_levels"] is None
    for k in grad_names(p, ("obj", "cls", "ctrl")):
        assert R.bits_equal(got[k], c[k + "_fp32"]), k
    for l in range(L):
        g, k = got["grad_reg_%d" % l].cpu(), "grad_reg_%d" % l
        assert g.is_contiguous(memory_format=fmt) or g.numel() <= 4
        assert R.bits_equal(g[:, :2], torch.from_numpy(c[k + "_fp32"])[:, :2]), k
        e, bound = R.rel_err(g[:, 2:], c[k][:, 2:]), 4 * float(c[k + "_exp_fp32_ref_err"])
        print("%s %s[2:4] err %.3g bound %.3g" % (tag, k, e, bound))
        assert e <= bound, (k, e, bound)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_fp64(ops, tag):
    c, p = R.load_case(tag), R.problem(tag)
    got = hip_run(ops, p, torch.float64)
    names, wide = R.stored_names(p)
    for k in names:
        e = R.rel_err(got[k], c[k])
        print("%s %-18s err %.3g" % (tag, k, e))
        assert got[k].dtype == torch.float64 and e <= 1e-12, (k, e)
    for k in wide:
        assert torch.equal(got[k].cpu().double(), torch.from_numpy(c[k + "_fp32"]).double()), k


def two_level():
    g = torch.Generator().manual_seed(77)
    levels = ((2, 3), (1, 2))
    return {"B": 2, "C": 2, "P": 3, "A": 8, "levels": levels, "strides": (8, 16),
            "reg": [torch.randn(2, 4, h, w, generator=g) for h, w in levels], "obj": [torch.randn(2, 1, h, w, generator=g) for h, w in levels],
            "cls": [torch.randn(2, 2, h, w, generator=g) for h, w in levels], "ctrl": [torch.randn(2, 3, h, w, generator=g) for h, w in levels]}


@pytest.mark.parametrize("which", ["one", "two_level"])
def test_gradcheck_fp64(ops, which):
    p = R.problem("one") if which == "one" else two_level()
    maps = R.leaves(p, torch.float64, DEV)
    L, flat = len(p["levels"]), [t for ts in maps if ts is not None for t in ts]

    def f(*ts):
        roles = [list(ts[r * L:(r + 1) * L]) for r in range(len(ts) // L)]
        res = ops.head_assemble(roles[0], roles[1], roles[2], p["strides"], roles[3] if len(roles) > 3 else None)
        return tuple(t for t in (res[0], res[1], res[5]) if t is not None)
    assert torch.autograd.gradcheck(f, flat, eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


@pytest.mark.parametrize("fmt", [NCHW, CL], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["small", "c80"])
def test_half_maps_equal_the_fp32_operator_on_the_widened_maps(ops, tag, half, fmt):
    p = dict(R.problem(tag))
    p["reg"][0][0, 2, 0, 0] = 11.5                                  # exp overflows fp16 above 11.09: the decode is in fp32
    wide = dict(p, **{m: (None if p[m] is None else [t.to(half).float() for t in p[m]]) for m in R.MAPS})
    got, want = hip_run(ops, p, half, fmt), hip_run(ops, wide, torch.float32, fmt)
    all_bits_equal(got, want, R.RESULTS)
    assert got["outputs"].dtype == torch.float32 and bool(torch.isfinite(got["outputs"]).all())
    for k in grad_names(p):
        assert got[k].dtype == half and got[k].is_contiguous(memory_format=fmt)
        assert R.bits_equal(got[k], want[k].to(half)), k              # rounded once


def test_gradient_subsets_unused_results_and_use_l1_false(ops):
    p = R.problem("small")
    full = hip_run(ops, p, torch.float32)
    only_cls = hip_run(ops, p, torch.float32, need=(False, False, True, False))
    assert all(only_cls[k] is None for k in grad_names(p, ("reg", "obj", "ctrl")))
    all_bits_equal(only_cls, full, grad_names(p, ("cls",)))
    only_reg = hip_run(ops, p, torch.float32, need=(True, False, False, False))
    assert all(only_reg[k] is None for k in grad_names(p, ("obj", "cls", "ctrl")))
    all_bits_equal(only_reg, full, grad_names(p, ("reg",)))
    # origin_preds unused: the gradient of reg is that of outputs alone; obj, cls, ctrl as before
    no_org = hip_run(ops, p, torch.float32, use=("outputs", "dynamic_params"))
    all_bits_equal(no_org, full, grad_names(p, ("obj", "cls", "ctrl")))
    zero_org = hip_run(ops, dict(p, g_origin=torch.zeros_like(p["g_origin"])), torch.float32)
    all_bits_equal(no_org, zero_org, grad_names(p, ("reg",)))
    # dynamic_params unused: no gradient reaches the controller maps, the others as before
    no_par = hip_run(ops, p, torch.float32, use=("outputs", "origin_preds"))
    assert all(no_par[k] is None for k in grad_names(p, ("ctrl",)))
    all_bits_equal(no_par, full, grad_names(p, ("reg", "obj", "cls")))
    # only origin_preds used: reg gets g_origin itself, obj and cls nothing
    only_org = hip_run(ops, p, torch.float32, use=("origin_preds",))
    assert all(only_org[k] is None for k in grad_names(p, ("obj", "cls", "ctrl")))
    off = 0
    for l, (h, w) in enumerate(p["levels"]):
        want = p["g_origin"][:, off:off + h * w].reshape(p["B"], h, w, 4).permute(0, 3, 1, 2)
        assert R.bits_equal(only_org["grad_reg_%d" % l], want.contiguous()), l
        off += h * w
    # use_l1 False: None, and the rest unchanged
    no_l1 = hip_run(ops, p, torch.float32, use_l1=False)
    assert no_l1["origin_preds"] is None
    all_bits_equal(no_l1, full, [k for k in R.RESULTS if k != "origin_preds"])
    all_bits_equal(no_l1, no_org, grad_names(p))
    # without controller maps
    no_ctrl = hip_run(ops, dict(p, ctrl=None, P=0), torch.float32)
    assert no_ctrl["dynamic_params"] is None and no_ctrl["fpn_levels"] is None
    all_bits_equal(no_ctrl, full, list(R.RESULTS[:5]) + grad_names(p, ("reg", "obj", "cls")))


def test_saved_tensors_are_the_reg_maps_only_and_the_shifts_carry_no_gradient(ops):
    p = R.problem("small")
    reg, obj, cls, ctrl = R.leaves(p, torch.float32, DEV)
    seen = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: seen.append(t) or t, lambda t: t):
        res = ops.head_assemble(reg, obj, cls, p["strides"], ctrl)
    assert len(seen) == len(reg) and all(s.data_ptr() == r.data_ptr() and s.shape == r.shape for s, r in zip(seen, reg))
    assert res[0].requires_grad and res[1].requires_grad and res[5].requires_grad
    assert not any(res[i].requires_grad for i in (2, 3, 4, 6))
    assert res[6].dtype == torch.int32 and all(res[i].shape == (1, p["A"]) for i in (2, 3, 4))


def test_two_runs_are_bitwise_equal(ops):
    for tag, dtype in (("small", torch.float32), ("c80", torch.float32), ("edge", torch.float64), ("small", torch.bfloat16)):
        p = R.problem(tag)
        a, b = hip_run(ops, p, dtype), hip_run(ops, p, dtype)
        all_bits_equal(a, b, list(R.RESULTS) + grad_names(p))


def test_other_strides_are_converted_once_and_mixed_layouts_read_in_place(ops):
    p = R.problem("small")
    full = hip_run(ops, p, torch.float32)
    reg, obj, cls, ctrl = R.leaves(p, torch.float32, DEV)
    with torch.no_grad():
        reg = [torch.cat([t, t], 3)[:, :, :, :t.shape[3]] for t in reg]                 # a view of a wider map: neither layout
        cls = [t.contiguous(memory_format=CL) for t in cls]
        ctrl[1] = ctrl[1].contiguous(memory_format=CL)
    assert not reg[0].is_contiguous() and not reg[0].is_contiguous(memory_format=CL)
    for t in reg + cls + ctrl:
        t.requires_grad_(True)
    res = ops.head_assemble(reg, obj, cls, p["strides"], ctrl)
    R.weighted(tuple(t if i in (0, 1, 5) else None for i, t in enumerate(res)), {k: p[k].to(DEV) for k in ("g_outputs", "g_origin", "g_params")},
               torch.float32, DEV).backward()
    for i, k in enumerate(R.RESULTS):
        assert R.bits_equal(res[i].detach(), full[k]), k
    for m, ts in (("reg", reg), ("obj", obj), ("cls", cls), ("ctrl", ctrl)):
        for l, t in enumerate(ts):
            assert R.bits_equal(t.grad, full["grad_%s_%d" % (m, l)]), (m, l)
    assert ctrl[1].grad.is_contiguous(memory_format=CL) and ctrl[0].grad.is_contiguous()


def headline(B, C, P, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    levels = ((100, 160), (50, 80), (25, 40))
    mk = lambda nc: [torch.randn(B, nc, h, w, generator=g).to(device=DEV, dtype=dtype).requires_grad_(True) for h, w in levels]      # noqa: E731
    return mk(4), mk(1), mk(C), mk(P), (8, 16, 32)


def test_headline_shape_without_a_sync(ops):
    reg, obj, cls, ctrl, strides = headline(2, 8, 169)

    def step():
        res = ops.head_assemble(reg, obj, cls, strides, ctrl)
        (res[0].sum() + res[1].sum() * 0.5 + res[5].sum() * 0.25).backward()
        return res
    res = step()                                                                     # library, allocator and kernels warm
    torch.cuda.synchronize()
    assert res[0].shape == (2, 21000, 13) and res[5].shape == (2, 21000, 169)
    # against the eager lines on this GPU (fp32 both: bit-equal outside the exp columns)
    with torch.no_grad():
        want = R.assemble(reg, obj, cls, strides, ctrl)
    for i in (1, 2, 3, 4, 5):
        assert R.bits_equal(res[i].detach(), want[i]), R.RESULTS[i]
    assert R.bits_equal(res[0].detach()[..., :2], want[0][..., :2]) and R.bits_equal(res[0].detach()[..., 4:], want[0][..., 4:])
    assert R.rel_err(res[0].detach()[..., 2:4], want[0][..., 2:4]) <= 4 * 2.0 ** -23
    assert torch.equal(res[6].cpu().long(), want[6])
    assert all(bool((t.grad == 0.25).all()) for t in ctrl) and all(bool((t.grad == 1.0).all()) for t in obj + cls)
    # No-sync check by a busy stream (the method of tests/test_head_loss_gpu.py)
    for t in reg + obj + cls + ctrl:
        t.grad = None
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
        step()
        host_ms = (time.perf_counter() - t0) * 1e3
    finally:
        torch.cuda.set_sync_debug_mode("default")
    pending = not behind_spin.query()
    torch.cuda.synchronize()
    print("forward + backward returned after %.2f ms on the host; spin kernel of %d cycles still running: %s" % (host_ms, cycles, pending))
    assert pending, "head_assemble / backward waited for the stream (%.1f ms on the host)" % host_ms


def test_end_to_end_with_the_loss_operators(ops):
    """head_assemble -> head_det_loss -> head_mask_loss -> backward on `small` (64 x 96 image) against the restated eager assembly feeding the
    same two loss operators; labels, masks, mask_feats and up_masks are images 0 and 2 of the head_mask_loss `batch` fixture (4 and 9 boxes)"""
    p = R.problem("small")
    c = HM.load_case("batch")
    (H, W), _, _, _, _ = HM.load_assignment("batch")
    assert (H, W) == (64, 96) and HM.CASES["batch"][1] == 4
    keep = [0, 2]
    labels = torch.from_numpy(np.load(os.path.join(R.GOLD, "head_loss_batch.npz"))["labels"])[keep].float().to(DEV)
    masks, mf, um = (torch.from_numpy(c[k])[keep].float().to(DEV) for k in ("masks", "mask_feats", "up_masks"))
    r, C = 4, p["C"]

    def chain(assemble, dtype, assignment=None):
        maps = R.leaves(p, dtype, DEV)
        outputs, origin, xs, ys, st, params, levels = assemble(*maps)
        if dtype == torch.float32:
            det, assignment = ops.head_det_loss(outputs, origin, labels, xs, ys, st, (H, W), C, assignment=assignment)
            det = det["total_loss"]
        else:                                                   # head_det_loss is fp32 only: the fp64 run takes the assignment of the fp32 one
            fg, matched, iou, num_fg = assignment
            lab = labels.double()
            det = ops.HeadLossFunction.apply(outputs, origin, lab, fg.to(torch.uint8), matched.to(torch.int32), iou.double(), num_fg.to(torch.int32),
                                             (lab.sum(2) > 0).sum(1).to(torch.int32), xs[0], ys[0], st[0], 5.0)[:4].sum()
        mask, _ = ops.head_mask_loss(mf.to(dtype), um.to(dtype), params, levels.to(DEV), masks.to(dtype), assignment, xs, ys, st, r)
        (det + 1.7 * mask).backward()
        out = {"det": det.detach(), "mask": mask.detach()}
        for m, ts in zip(R.MAPS, maps):
            for k, t in enumerate(ts):
                out["grad_%s_%d" % (m, k)] = t.grad
        return out, assignment

    hip, a_hip = chain(lambda reg, obj, cls, ctrl: ops.head_assemble(reg, obj, cls, p["strides"], ctrl), torch.float32)
    e32, a_e32 = chain(lambda reg, obj, cls, ctrl: R.assemble(reg, obj, cls, p["strides"], ctrl), torch.float32)
    e64, _ = chain(lambda reg, obj, cls, ctrl: R.assemble(reg, obj, cls, p["strides"], ctrl), torch.float64, a_e32)
    assert all(torch.equal(a_hip[i], a_e32[i]) for i in (0, 1, 3)), "the two assemblies reach different assignments"
    assert int(a_hip[3].sum()) > 0
    assert len(hip) == 2 + 12
    for k in hip:
        e, ref = R.rel_err(hip[k], e64[k]), R.rel_err(e32[k], e64[k])
        print("%-12s HIP vs fp64 %.3g   eager fp32 vs fp64 %.3g" % (k, e, ref))
        assert e <= 4 * ref, (k, e, ref)
