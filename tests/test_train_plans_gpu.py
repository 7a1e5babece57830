"""Every launch plan of the three ConvNeXt training operators (ops.layernorm_cf, ops.dwconv7_ln, ops.block_tail) is found, listed and run
against a reference (tests/train_plans.py holds the lists and says what a plan class is).

  1. sweep and closure   the forward alone at one pixel for every C = 4, 8, ..., 2048, traced: the plan classes the launchers pick are exactly
                         train_plans.EXPECTED, in both directions; {operator: {class: [C min, C max, count]}} goes to train_plan_census.json in
                         the suite's results directory (next to variant_census.json)
  2. parity per class    the smallest and the largest C of every class the sweep found (block_tail: every width of WIDTHS_BT), forward and
                         backward with all gradients wanted at train_plans.MAP / MAP_DW, traced -- the forward and the backward map kernels
                         must both report the class under test -- against the operator's own restatement in fp64: 1e-12 for the fp64 twin,
                         4 x the restatement's own fp32 deviation on the same inputs for fp32, plus half an ulp of the half type on the
                         half-typed gradient for fp16 / bf16 x (lncf) or y (block_tail), the restatement then on the rounded tensor.  Two
                         calls are bit-equal.  Failures are collected per class and reported once.  ops.downsample_ln runs the
                         channels-last kernel of lncf with another store address, so its kernels run alone (tests/down_calls.py, no
                         GEMM) at both ends of every channels-last class too, against down_train_ref.patch_grads: the traced tags, a
                         rebuilt A with the forward's bytes and exact zeros in g_x at the pixels an odd H or W drops.
  3. a block that loops at wide C: more groups / tiles / chunks than the 1024 blocks a launch may have (the existing many-pixel cases loop
     at C = 4 and 8 only), and dwln with four waves per strip on a map whose rows the weight pass splits.

No bound comes from a kernel.  A result whose fp32 yardstick is zero (block_tail's g_residual: grad_out itself) is held to the exact bits."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import block_tail_ref as RB  # noqa: E402
import down_calls as KD  # noqa: E402
import down_train_ref as RDN  # noqa: E402
import dwln_train_ref as RD  # noqa: E402
import guard  # noqa: E402
import lncf_ref as RL  # noqa: E402
import train_plans as P  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
CL, NCHW = torch.channels_last, torch.contiguous_format
FMT = {"cl": CL, "nchw": NCHW}
DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}          # one rounding to nearest, relative to the largest value
LNCF_COMBOS = [(lay, dt) for lay in ("cl", "nchw") for dt in ("f32", "f16", "bf16", "f64")]
DWLN_COMBOS = ["f32", "f64"]
BT_COMBOS = [(lay, dt) for lay in ("cl", "nchw") for dt in ("f64", "f32", "f16", "bf16")]


def _math(dt):
    """the dtype of the parameters and of the arithmetic next to an x / y of type dt"""
    return torch.float64 if dt == "f64" else torch.float32


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    yield _lib
    for cached in (lncf_case, down_case, bt_case, dwln_case):          # the wide cases hold their inputs and references on the device
        cached.cache_clear()


def traced(lib, fn):
    """fn() with the variant trace on -> (its result, {tag: launches})"""
    lib.uni_variant_trace(1)
    try:
        res = fn()
    finally:
        lib.uni_variant_trace(0)
    return res, vc.read_trace(lib)


def map_tags(tags, op, kind):
    """the plan classes of the map kernels `<op> <kind>...` in a trace, one entry per launch"""
    out = []
    for t, n in tags.items():
        if t.startswith("%s %s" % (op, kind)) and P.plan_class(t) is not None:
            out += [P.plan_class(t)] * n
    return out


# ================================================================================================================ 1. sweep and closure
@functools.lru_cache(maxsize=None)
def sweep(op, layout, dt):
    """{C: plan class} of the forward alone, one launch per C.  lncf reads x in place in either layout and (1, C, 1, 1) is both at once (the
    operator then takes it as channels-last), so the NCHW sweep runs (1, C, 1, 2): two pixels, NCHW-contiguous and not channels-last."""
    from unicorn_amd import _lib, ops
    lib = _lib.lib()
    g = torch.Generator().manual_seed(1)
    xbuf = torch.randn(2 * P.C_MAX, generator=g).to(DEV, DT[dt])
    vec = [torch.randn(49 * P.C_MAX, generator=g).to(DEV, _math(dt)) for _ in range(5)]
    kind = {"lncf": "lncf_train fwd_" + layout, "dwln": "dwln_train fwd"}[op]
    found = {}
    try:
        for C in P.SWEEP_C:
            if op == "lncf":
                x = xbuf[:2 * C].view(1, C, 1, 2) if layout == "nchw" else xbuf[:C].view(1, C, 1, 1)
                call = lambda: ops.layernorm_cf(x, vec[0][:C], vec[1][:C], RL.EPS)                                       # noqa: E731
            else:
                x = xbuf[:C].view(1, C, 1, 1)
                call = lambda: ops.dwconv7_ln(x, vec[0][:49 * C].view(C, 1, 7, 7), vec[1][:C], vec[2][:C], vec[3][:C], RD.EPS)      # noqa: E731
            lib.uni_variant_trace(1)
            call()
            tags = vc.read_trace(lib)
            assert len(tags) == 1 and sum(tags.values()) == 1, (op, layout, dt, C, tags)
            tag = next(iter(tags))
            assert tag.startswith(kind), (C, tag, kind)
            found[C] = P.plan_class(tag)
    finally:
        lib.uni_variant_trace(0)
    torch.cuda.synchronize()
    return found


def expected_of(op, layout, dt):
    head = "%s<%s," % (layout, dt) if op == "lncf" else "<%s," % dt
    return sorted(c for c in P.EXPECTED[op] if c.startswith(head))


def _closure(op, layout, dt):
    by_c = sweep(op, layout, dt)
    found, want = P.group(by_c), expected_of(op, layout, dt)
    extra, missing = sorted(set(found) - set(want)), sorted(set(want) - set(found))
    for cls, cs in found.items():
        print("%-28s C %4d .. %4d  (%d widths)" % (cls, cs[0], cs[-1], len(cs)))
    assert not extra and not missing, "launched but not listed: %s; listed but never launched: %s" % (
        {c: found[c][:3] for c in extra}, missing)
    # the restated arithmetic (which picks the widths of tests/test_train_plans_cpu.py) agrees with the launcher at every width
    off = {C: (cls, P.predicted(op, layout, dt, C)) for C, cls in by_c.items() if cls != P.predicted(op, layout, dt, C)}
    assert not off, "launcher and train_plans.predicted disagree: %s" % dict(sorted(off.items())[:8])


@pytest.mark.parametrize("layout,dt", LNCF_COMBOS, ids=["%s-%s" % c for c in LNCF_COMBOS])
def test_lncf_sweep_finds_exactly_the_listed_classes(L, layout, dt):
    _closure("lncf", layout, dt)


@pytest.mark.parametrize("dt", DWLN_COMBOS)
def test_dwln_sweep_finds_exactly_the_listed_classes(L, dt):
    _closure("dwln", "", dt)


def test_the_census_lists_every_class_with_its_range(L):
    """all sweeps together are EXPECTED, nothing more and nothing less, and the census file holds every class with its C range"""
    census, launches = {"lncf": {}, "dwln": {}}, 0
    for op, combos in (("lncf", LNCF_COMBOS), ("dwln", [("", dt) for dt in DWLN_COMBOS])):
        for layout, dt in combos:
            found = sweep(op, layout, dt)
            launches += len(found)
            for cls, cs in P.group(found).items():
                assert cls not in census[op], "one class from two sweeps: %s" % cls
                census[op][cls] = [cs[0], cs[-1], len(cs)]
    for op in census:
        assert sorted(census[op]) == sorted(P.EXPECTED[op]), (op, sorted(set(census[op]) ^ set(P.EXPECTED[op])))
        for cls in P.FIRST_RUN[op]:
            assert cls in census[op], cls
    assert launches == (len(LNCF_COMBOS) + len(DWLN_COMBOS)) * len(P.SWEEP_C)
    print("%d sweep launches, %d + %d classes" % (launches, len(census["lncf"]), len(census["dwln"])))
    out = guard.results_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "train_plan_census.json"), "w") as f:
        json.dump(dict(census, sweep_launches=launches, first_run={k: sorted(v) for k, v in P.FIRST_RUN.items()}), f, indent=1, sort_keys=True)


# ================================================================================================================ 2. parity per class
def _half_of(dt):
    return DT[dt] if dt in HALF_ULP else None


def _report(bad):
    """every failed case by name, in full (the representation of a long dict in an assertion is shortened)"""
    return "%d case(s) failed: %s\n%s" % (len(bad), ", ".join(bad), "\n".join("  %s: %s" % kv for kv in bad.items()))


def _judge(bad, key, got, again, ref, dev, dt, half_results):
    """collects into bad[key] every result outside its bound (half_results: those a half dt rounds once more) and every result that differs
    between the two calls"""
    for n in ref:
        err = RL.rel_err(got[n], ref[n])
        bound = 1e-12 if dt == "f64" else 4 * dev[n] + (HALF_ULP[dt] if dt in HALF_ULP and n in half_results else 0.0)
        print("%-36s %-10s err %.3e  bound %.3e" % (key, n, err, bound))
        if not (got[n].shape == ref[n].shape and err <= bound):
            bad.setdefault(key, {})[n] = (err, bound)
        if not torch.equal(got[n], again[n]):
            bad.setdefault(key, {})[n + " (second call)"] = "differs"


# ---------------------------------------------------------------------------------------------------------------- lncf
@functools.lru_cache(maxsize=None)
def lncf_case(shape, half=None, on_device=False):
    """draws (x rounded to `half` first), the restatement in fp64 and its own fp32 deviation: computed once per case, shared, never modified"""
    ins = list(RL.draw("plain", sum(shape), shape))
    if half is not None:
        ins[0] = ins[0].to(half).float()
    if on_device:
        ins = [t.to(DEV) for t in ins]
    ref = RL.value_and_grads(*ins, dtype=torch.float64)
    f32 = RL.value_and_grads(*ins, dtype=torch.float32)
    return ins, ref, {n: RL.rel_err(f32[n], ref[n]) for n in RL.RESULTS}


def lncf_run(ins, dt, layout):
    from unicorn_amd.ops import layernorm_cf
    m = _math(dt)
    x = ins[0].detach().to(DEV, DT[dt], copy=True).contiguous(memory_format=FMT[layout]).requires_grad_(True)
    w, b = (t.detach().to(DEV, m, copy=True).requires_grad_(True) for t in ins[1:3])
    g = ins[3].to(DEV, m).contiguous(memory_format=FMT[layout])
    y = layernorm_cf(x, w, b, RL.EPS)
    y.backward(g)
    torch.cuda.synchronize()
    assert y.dtype == m and x.grad.dtype == DT[dt] and y.is_contiguous(memory_format=FMT[layout]) and x.grad.is_contiguous(memory_format=FMT[layout])
    return {"y": y.detach(), "g_x": x.grad, "g_weight": w.grad, "g_bias": b.grad}


def lncf_check(lib, bad, shape, dt, layout, cls, on_device=False):
    key = "%s C=%d" % (cls, shape[1])
    ins, ref, dev = lncf_case(shape, _half_of(dt), on_device)
    got, tags = traced(lib, lambda: lncf_run(ins, dt, layout))
    again = lncf_run(ins, dt, layout)
    fwd, bwd = map_tags(tags, "lncf_train", "fwd"), map_tags(tags, "lncf_train", "bwd")
    if not (fwd == [cls] and bwd == [cls] and sum(tags.values()) == 3):         # forward, backward, reduce
        bad.setdefault(key, {})["trace"] = tags
    _judge(bad, key, got, again, ref, dev, dt, ("g_x",))


@pytest.mark.parametrize("layout,dt", LNCF_COMBOS, ids=["%s-%s" % c for c in LNCF_COMBOS])
def test_lncf_parity_at_both_ends_of_every_class(L, layout, dt):
    classes = P.group(sweep("lncf", layout, dt))
    assert classes
    bad = {}
    for cls, cs in classes.items():
        for C in P.ends(cs):
            lncf_check(L.lib(), bad, (P.MAP[0], C) + P.MAP[1:], dt, layout, cls)
    assert not bad, _report(bad)


# ---------------------------------------------------------------------------------------------------------------- down_train
# ops.downsample_ln walks its input as lncf's channels-last plan says (csrc/ln_cl.h is the kernel of both), so its classes are those the
# lncf sweep finds; its fixtures (tests/down_train_ref.py) reach NV <= 3 only.  The kernels alone through the C-ABI, no GEMM.
@functools.lru_cache(maxsize=None)
def down_case(C, half=None):
    """x (MAP with C channels) and grad_A (M, 4 C), both rounded to `half` first (A has the element type of x here), the LayerNorm parameters,
    the patch restatement in fp64 and its own fp32 deviation: computed once per case, shared, never modified"""
    shape = (P.MAP[0], C) + P.MAP[1:]
    x, w, b = RDN.draw("plain", sum(shape), shape, 4)[:3]
    gA = torch.randn(P.MAP[0] * (P.MAP[1] // 2) * (P.MAP[2] // 2), 4 * C, generator=torch.Generator().manual_seed(C))
    if half is not None:
        x, gA = x.to(half).float(), gA.to(half).float()
    ref = RDN.patch_grads(x, w, b, gA, dtype=torch.float64)
    f32 = RDN.patch_grads(x, w, b, gA, dtype=torch.float32)
    return (x, w, b, gA), ref, {n: RL.rel_err(f32[n], ref[n]) for n in ref}


def down_run(L, ins, dt):
    x, w, b, gA = ins
    return KD.run_down(L, x.to(DEV, DT[dt]), w.to(DEV, _math(dt)), b.to(DEV, _math(dt)), gA.to(DEV, DT[dt]), DT[dt])


def down_check(L, bad, C, dt, cls):
    key = "%s C=%d" % (cls, C)
    ins, ref, dev = down_case(C, _half_of(dt))
    got, tags = traced(L.lib(), lambda: down_run(L, ins, dt))
    again = down_run(L, ins, dt)
    want = {"down_train fwd_%s a=%s" % (cls, dt): 1, "down_train rebuild_%s a=%s" % (cls, dt): 1,
            "down_train bwd_%s a=%s gx=1 gwb=1" % (cls, dt): 1, "down_train reduce<%s>" % ("f64" if dt == "f64" else "f32"): 1}
    if tags != want:
        bad.setdefault(key, {})["trace"] = tags
    if not torch.equal(got["A"].view(torch.uint8), got["A2"].view(torch.uint8)):
        bad.setdefault(key, {})["A2"] = "the rebuilt A differs from the forward's"
    Ho, Wo = P.MAP[1] // 2, P.MAP[2] // 2                   # H = 3 and W = 7 drop the last row and the last column
    if got["g_x"][:, :, 2 * Ho:, :].any() or got["g_x"][:, :, :, 2 * Wo:].any():
        bad.setdefault(key, {})["g_x"] = "not zero at a dropped pixel"
    _judge(bad, key, got, again, ref, dev, dt, ("A", "g_x"))


@pytest.mark.parametrize("dt", ["f32", "f16", "bf16", "f64"])
def test_down_parity_at_both_ends_of_every_class(L, dt):
    """bounds as for lncf above, from the restatement alone: 1e-12 for fp64, else 4 x the deviation of the fp32 patch_grads from its fp64 run
    on the same inputs, plus half an ulp of the half type on A and on g_x, which are then rounded once more"""
    classes = P.group(sweep("lncf", "cl", dt))
    assert classes
    bad = {}
    for cls, cs in classes.items():
        for C in P.ends(cs):
            down_check(L, bad, C, dt, cls)
    assert not bad, _report(bad)


# ---------------------------------------------------------------------------------------------------------------- dwln
@functools.lru_cache(maxsize=None)
def dwln_case(shape):
    """as tests/test_dwln_train_gpu.py large_case: the restatement on the CPU in fp64 and its own deviation in fp32"""
    ins = RD.draw("plain", sum(shape), shape)
    ref = RD.value_and_grads(*(t.double() for t in ins))
    f32 = RD.value_and_grads(*ins)
    return ins, ref, {n: RD.rel_err(f32[n], ref[n]) for n in RD.RESULTS}


def dwln_run(ins, dt):
    from unicorn_amd.ops import dwconv7_ln
    m = DT[dt]
    leaves = [ins[0].to(DEV, m).contiguous(memory_format=CL)] + [t.to(DEV, m) for t in ins[1:5]]
    for t in leaves:
        t.requires_grad_(True)
    y = dwconv7_ln(*leaves, eps=RD.EPS)
    y.backward(ins[5].to(DEV, m))
    torch.cuda.synchronize()
    assert y.dtype == m and y.is_contiguous()
    return dict(zip(RD.RESULTS, [y.detach()] + [t.grad for t in leaves]))


def dwln_check(lib, bad, shape, dt, cls):
    key = "%s C=%d" % (cls, shape[1])
    ins, ref, dev = dwln_case(shape)
    got, tags = traced(lib, lambda: dwln_run(ins, dt))
    again = dwln_run(ins, dt)
    kernels = [map_tags(tags, "dwln_train", k) for k in ("fwd", "bwd_a", "bwd_dx")]
    if not (kernels == [[cls]] * 3 and sum(tags.values()) == 5):               # + the weight pass and the reduce
        bad.setdefault(key, {})["trace"] = tags
    _judge(bad, key, got, again, ref, dev, dt, ())


@pytest.mark.parametrize("dt", DWLN_COMBOS)
def test_dwln_parity_at_both_ends_of_every_class(L, dt):
    classes = P.group(sweep("dwln", "", dt))
    assert classes
    bad = {}
    for cls, cs in classes.items():
        for C in P.ends(cs):
            dwln_check(L.lib(), bad, (P.MAP_DW[0], C) + P.MAP_DW[1:], dt, cls)
    assert not bad, _report(bad)


# ---------------------------------------------------------------------------------------------------------------- block_tail
@functools.lru_cache(maxsize=None)
def bt_case(shape, half=None, on_device=False):
    """gamma and a per-sample factor with the middle sample of three dropped; y rounded to `half` first"""
    ins = list(RB.draw("plain", sum(shape), shape, scale=P.SCALE_BT))
    if half is not None:
        ins[0] = ins[0].to(half).float()
    if on_device:
        ins = [t.to(DEV) for t in ins]
    ref = RB.value_and_grads(*ins, dtype=torch.float64)
    f32 = RB.value_and_grads(*ins, dtype=torch.float32)
    return ins, ref, {n: RB.rel_err(f32[n], ref[n]) for n in RB.RESULTS}


def bt_run(ins, dt, layout):
    from unicorn_amd.ops import block_tail
    m = _math(dt)
    y = ins[0].detach().to(DEV, DT[dt], copy=True).requires_grad_(True)
    res = ins[1].detach().to(DEV, m, copy=True).contiguous(memory_format=FMT[layout]).requires_grad_(True)
    gamma = ins[2].detach().to(DEV, m, copy=True).requires_grad_(True)
    g = ins[4].to(DEV, m).contiguous(memory_format=FMT[layout])
    out = block_tail(y, res, gamma, ins[3].to(DEV, m))
    out.backward(g)
    torch.cuda.synchronize()
    assert out.dtype == m and out.is_contiguous(memory_format=CL) and y.grad.dtype == DT[dt] and y.grad.is_contiguous()
    return {"out": out.detach(), "g_residual": res.grad, "g_y": y.grad, "g_gamma": gamma.grad}


def bt_check(lib, bad, shape, dt, layout, on_device=False):
    cls = P.bt_class(layout, dt, shape[1])
    key = "%s C=%d" % (cls, shape[1])
    ins, ref, dev = bt_case(shape, _half_of(dt), on_device)
    got, tags = traced(lib, lambda: bt_run(ins, dt, layout))
    again = bt_run(ins, dt, layout)
    fwd, bwd = map_tags(tags, "block_tail", "fwd"), map_tags(tags, "block_tail", "bwd")
    if not (fwd == [cls] and bwd == [cls] and sum(tags.values()) == 3):         # forward, backward, reduce
        bad.setdefault(key, {})["trace"] = tags
    _judge(bad, key, got, again, ref, dev, dt, ("g_y",))


@pytest.mark.parametrize("layout,dt", BT_COMBOS, ids=["%s-%s" % c for c in BT_COMBOS])
def test_block_tail_parity_at_every_listed_width(L, layout, dt):
    bad = {}
    for C in P.WIDTHS_BT:
        bt_check(L.lib(), bad, (3, C) + P.MAP[1:], dt, layout)
    assert not bad, _report(bad)


# ================================================================================================================ 3. a block that loops, at wide C
# TRAIN_ROWS = 1024 blocks at most (csrc/train_ops.h).  The restatement and its fp32 deviation are computed on the device, as the many-pixel
# cases of tests/test_lncf_train_gpu.py and tests/test_block_tail_gpu.py do; dwln's on the CPU, as tests/test_dwln_train_gpu.py does.
@pytest.mark.parametrize("shape,layout,dt,cls", [
    # 4225 pixels, 4 per block (G = 64): 1057 groups, the last of one pixel
    ((1, 768, 65, 65), "cl", "f32", "cl<f32,V=4,NV=3> G=64"),
    ((1, 768, 65, 65), "cl", "f64", "cl<f64,V=4,NV=3> G=64"),
    # fp16 x has 8 channels per lane: G = 32, 8 pixels per block, 529 groups at this map (one step per block) ...
    ((1, 768, 65, 65), "cl", "f16", "cl<f16,V=8,NV=3> G=32"),
    # ... and 8281 pixels make 1036 groups: its blocks loop too
    ((1, 768, 91, 91), "cl", "f16", "cl<f16,V=8,NV=3> G=32"),
    # 65792 pixels: 1028 tiles of 64; C = 260 gives the eight waves slices of 33 and 32 channels, walked in chunks of 8 with a tail of 1 or 0
    ((1, 260, 257, 256), "nchw", "f32", "nchw<f32,stream=8>"),
    ((1, 260, 257, 256), "nchw", "f64", "nchw<f64,stream=8>"),
], ids=["cl768-f32", "cl768-f64", "cl768-f16", "cl768-f16-loop", "nchw260-f32", "nchw260-f64"])
def test_lncf_blocks_that_loop_at_wide_c(L, shape, layout, dt, cls):
    bad = {}
    lncf_check(L.lib(), bad, shape, dt, layout, cls, on_device=True)
    assert not bad, _report(bad)


@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_block_tail_blocks_that_loop_at_wide_c(L, dt):
    """(3, 768, 53, 53): PP = 2, chunks of 8 pixels, 352 per image and 1056 in all: blocks 0 .. 31 take a second chunk, which lies in the last
    image while their first lies in the first; the middle image is dropped"""
    bad = {}
    bt_check(L.lib(), bad, (3, 768, 53, 53), dt, "cl", on_device=True)
    assert not bad, _report(bad)


@pytest.mark.parametrize("dt,cls", [("f32", "<f32,PXT=8> wps=4 NS=2"), ("f64", "<f64,PXT=2> wps=4 NS=2")], ids=["f32", "f64"])
def test_dwln_many_strips_at_wide_c(L, dt, cls):
    """(1, 1024, 40, 130): four waves per strip, two strips per block.  fp32: 17 strips per row (the last of 2 pixels), 680 in 340 blocks; fp64:
    65 strips per row, 2600 in 1300 groups, more than the 1024 blocks of pass A, so its blocks take a second group.  W > 128: the weight pass
    splits a row into two strips of 65"""
    bad = {}
    dwln_check(L.lib(), bad, (1, 1024, 40, 130), dt, cls)
    assert not bad, _report(bad)
