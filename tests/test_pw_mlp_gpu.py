"""The recomputing pwconv1-GELU-pwconv2 operator on the GPU (ops.pw_mlp, csrc/pw_mlp.hip, unicorn_amd.nn.fuse_pw_mlp / fuse_backbone_mlp): the
fixtures written from the reference's own Block in fp64 (1e-12) and fp32 (4 x the larger of the reference's own fp32 deviation and that of the
eager lines on the same device), fp16 / bf16 autocast against the eager autocast lines, the kernels alone through the C-ABI, the widest and the
longest shapes, a width whose last column tile has idle vector slots, finite extremes of the GELU, the need flags with the variant trace, what autograd keeps and how many bytes that is, an empty
batch, and a stand-in mini-backbone fused with fuse_backbone_mlp against the unfused one.  No bound comes from the code under test."""
import copy
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import block_tail_ref as RB  # noqa: E402
import pw_mlp_ref as R  # noqa: E402
import train_plans as TP  # noqa: E402
from pw_mlp_calls import act_calls, traced as _traced  # noqa: E402

DEV = "cuda"
KEEPS = ["hidden", "input"]
GRADS = ("g_t", "g_w1", "g_b1", "g_w2", "g_b2")
ULP = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def _leaves(ins, dtype, need):
    return [x.detach().to(DEV, dtype, copy=True).requires_grad_(k) for x, k in zip(ins[:5], need)]


def run_op(ins, dtype, keep="hidden", need=(True,) * 5, autocast=None):
    """ops.pw_mlp + backward on the device -> {y, g_t, g_w1, g_b1, g_w2, g_b2} (None where not needed)"""
    from unicorn_amd.ops import pw_mlp
    lv = _leaves(ins, dtype, need)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        y = pw_mlp(*lv, keep=keep)
    assert y.dtype == (autocast or dtype) and tuple(y.shape) == tuple(ins[0].shape[:-1]) + (ins[3].shape[0],)
    if any(need):
        y.backward(ins[5].to(DEV, y.dtype))
    torch.cuda.synchronize()
    return dict(zip(("y",) + GRADS, [y.detach()] + [x.grad for x in lv]))


def run_eager(ins, dtype, autocast=None):
    """the three eager lines on the device"""
    lv = _leaves(ins, dtype, (True,) * 5)
    with torch.autocast("cuda", dtype=autocast or torch.float16, enabled=autocast is not None):
        y = F.linear(F.gelu(F.linear(lv[0], lv[1], lv[2])), lv[3], lv[4])
    y.backward(ins[5].to(DEV, y.dtype))
    torch.cuda.synchronize()
    return dict(zip(("y",) + GRADS, [y.detach()] + [x.grad for x in lv]))


def fixture_inputs(c):
    return [torch.from_numpy(c[n]) for n in R.INPUTS]


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp64_matches_the_fixture(L, tag, keep):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float64, keep)
    bad = {}
    for n in R.RESULTS:
        err = R.rel_err(got[n], torch.from_numpy(c[n]))
        print("%s %s fp64 %-5s err %.3e" % (tag, keep, n, err))
        if not (got[n].shape == c[n].shape and err <= 1e-12):
            bad[n] = err
    assert not bad, bad


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp32_within_four_times_the_reference_side_fp32_deviation(L, tag, keep):
    """per result, 4 x the larger of the fixture's fp32 yardstick (the reference Block's lines in fp32 on the CPU) and the deviation of the eager
    fp32 lines on this device from the fixture: the GEMMs are the vendor's on both sides"""
    c = R.load_case(tag)
    ins = fixture_inputs(c)
    got, eager = run_op(ins, torch.float32, keep), run_eager(ins, torch.float32)
    bad = {}
    for n in R.RESULTS:
        ref = torch.from_numpy(c[n])
        yard_cpu, yard_dev = float(c[n + "_fp32_ref_err"]), R.rel_err(eager[n], ref)
        err, bound = R.rel_err(got[n], ref), 4 * max(yard_cpu, yard_dev)
        print("%s %s fp32 %-5s err %.3e  yardsticks: fixture %.3e, eager on the device %.3e" % (tag, keep, n, err, yard_cpu, yard_dev))
        assert got[n].dtype == torch.float32
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c24", "h100", "c48"])
def test_half_autocast_against_the_eager_autocast_lines(L, tag, half, keep):
    """fp32 tensors under torch.autocast: each run is compared with the fixture (fp64) and the operator may be at most 4 x as far from it as the
    eager autocast lines on the same device are, per result; y and every gradient have eager's dtypes.  c24 and c48 take 8 hidden units per
    lane, h100 (Hd % 8 == 4) four."""
    c = R.load_case(tag)
    ins = fixture_inputs(c)
    got, eager = run_op(ins, torch.float32, keep, autocast=half), run_eager(ins, torch.float32, autocast=half)
    assert got["y"].dtype == eager["y"].dtype == half
    bad = {}
    for n in R.RESULTS:
        ref = torch.from_numpy(c[n])
        err, bound = R.rel_err(got[n], ref), 4 * R.rel_err(eager[n], ref)
        print("%s %s %s %-5s err %.3e  bound %.3e" % (tag, keep, half, n, err, bound))
        assert got[n].dtype == eager[n].dtype, n
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ the kernels alone, through the C-ABI
@functools.lru_cache(maxsize=None)
def hidden_case(tag):
    """h and grad_a of the case in fp64 on the CPU (the restatement on the fixture's inputs); computed once, shared, never modified"""
    c = R.load_case(tag)
    full = R.value_and_grads(*fixture_inputs(c), dtype=torch.float64)
    Hd = full["h"].shape[-1]
    return c, full["h"].reshape(-1, Hd), full["grad_a"].reshape(-1, Hd)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=["fp32", "fp64", "fp16", "bf16"])
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_kernels_alone(L, tag, dtype):
    """h and grad_a in, a, grad_h and grad_b1 out, against the restatement in fp64 on the ROUNDED inputs: no GEMM on either side.  fp64: 1e-12.
    fp32: 4 x the larger of the fixture's yardstick and the deviation of eager F.gelu + autograd in fp32 on this device.  fp16 / bf16: one
    rounding of the element type on top for a and grad_h (half an ulp of the largest value); grad_b1 sums unrounded values and gets none.  The
    in-place forms and a second call give the same bits."""
    c, h64, ga64 = hidden_case(tag)
    h, ga = h64.to(DEV, dtype), ga64.to(DEV, dtype)
    ref = R.act_maps(h.double(), ga.double())
    got = act_calls(L, h, ga)
    # the eager yardstick: F.gelu and its autograd backward in fp32 on the device, on the fp32-rounded inputs
    he = h64.to(DEV, torch.float32).requires_grad_(True)
    ae = F.gelu(he)
    ae.backward(ga64.to(DEV, torch.float32))
    ref32 = R.act_maps(he.detach().double(), ga64.to(DEV, torch.float32).double())
    eager = {"a": R.rel_err(ae, ref32["a"]), "grad_h": R.rel_err(he.grad, ref32["grad_h"]), "g_b1": R.rel_err(he.grad.sum(0), ref32["g_b1"])}
    bad = {}
    for n, key in (("a_fwd", "a"), ("a", "a"), ("grad_h", "grad_h"), ("g_b1", "g_b1")):
        err = R.rel_err(got[n], ref[key])
        if dtype == torch.float64:
            bound = 1e-12
        else:
            bound = 4 * max(float(c[key + "_fp32_ref_err"]), eager[key]) + (ULP.get(dtype, 0.0) if key != "g_b1" else 0.0)
        print("%s %s %-6s err %.3e  bound %.3e (fixture %.3e, eager on the device %.3e)" % (tag, dtype, n, err, bound,
                                                                                          float(c[key + "_fp32_ref_err"]), eager[key]))
        if not err <= bound:
            bad[n] = (err, bound)
    assert got["a"].dtype == got["grad_h"].dtype == dtype and got["g_b1"].dtype == (torch.float64 if dtype == torch.float64 else torch.float32)
    assert not bad, bad
    assert torch.equal(got["a_fwd"], got["a"])
    again, inpl = act_calls(L, h, ga), act_calls(L, h, ga, inplace=True)
    for n in ("a_fwd", "a", "grad_h", "g_b1"):
        assert torch.equal(got[n], again[n]), n
        assert torch.equal(got[n], inpl[n]), n


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16], ids=["fp32", "fp64", "fp16"])
def test_finite_extremes(L, dtype):
    """h in {0, +-1e-3, +-6, +-30}: finite a and grad_h, gelu'(30) == 1, gelu'(-30) == 0, a(-30) == 0, a(0) == 0, gelu'(0) == 0.5.  In fp64
    gelu'(-30) = Phi(-30) - 30 phi(30) = -4.4e-195 is a representable number (exp(-450) does not underflow there), so the exact zero is
    demanded of the fp32 arithmetic only and the fp64 form is held to the restatement."""
    h = torch.tensor([[0.0, 1e-3, -1e-3, 6.0], [-6.0, 30.0, -30.0, 0.0]], device=DEV, dtype=dtype)
    got = act_calls(L, h, torch.ones_like(h))
    a, d = got["a"], got["grad_h"]                                   # grad_a = 1: grad_h = gelu'(h)
    assert torch.isfinite(a).all() and torch.isfinite(d).all() and torch.isfinite(got["g_b1"]).all()
    assert d[1, 1] == 1 and a[1, 2] == 0 and a[0, 0] == 0 and a[1, 3] == 0 and d[0, 0] == 0.5 and a[1, 1] == 30
    assert (-1e-190 < d[1, 2] <= 0) if dtype == torch.float64 else d[1, 2] == 0
    ref = R.act_maps(h.double(), torch.ones_like(h).double())
    tol = 1e-12 if dtype == torch.float64 else 4e-7 + ULP.get(dtype, 0.0)      # a few fp32 roundings; the fixtures' yardsticks are 1 - 3e-7
    assert R.rel_err(a, ref["a"]) <= tol and R.rel_err(d, ref["grad_h"]) <= tol


# ------------------------------------------------------------------------------------------------ wide and long shapes
WIDE = {"hd8192": ((3,), 2048, 8192, 2048),          # the limit
        "hd6144": ((6,), 1536, 6144, 1536),          # the widest stage
        "long": ((1, 300, 300), 4, 16, 4)}           # 90000 rows: L = 4, 64 rows per group, 1407 groups on 256 rows of partials -> blocks loop


@functools.lru_cache(maxsize=None)
def wide_case(tag):
    """inputs, the eager lines in fp64 on the device and their own fp32 deviation (computed once, shared, never modified)"""
    ins = R.draw(tag, 77, WIDE[tag])
    ref = run_eager(ins, torch.float64)
    f32 = run_eager(ins, torch.float32)
    return ins, ref, {n: R.rel_err(f32[n], ref[n]) for n in R.RESULTS}


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("tag", sorted(WIDE))
def test_wide_and_long_shapes_against_the_eager_lines(L, tag, keep):
    """fp32 against eager fp64 on the same device, bound 4 x eager fp32's own deviation; `long` covers the column sum of grad_y with Co = 4 as
    well (g_b2).  Two calls are bit-equal."""
    ins, ref, dev = wide_case(tag)
    got, again = run_op(ins, torch.float32, keep), run_op(ins, torch.float32, keep)
    bad = {}
    for n in R.RESULTS:
        err, bound = R.rel_err(got[n], ref[n]), 4 * dev[n]
        print("%s %s %-5s fp32 err %.3e bound %.3e" % (tag, keep, n, err, bound))
        if not err <= bound:
            bad[n] = (err, bound)
        assert torch.equal(got[n], again[n]), n
    assert not bad, bad


def test_long_column_sums_alone(L):
    """the two sums of 90000 rows through the C-ABI against fp64 sums of the same values, bound 4 x the deviation of torch's fp32 sum"""
    g = torch.Generator().manual_seed(5)
    h, ga, gy = (torch.randn(90000, n, generator=g).to(DEV) for n in (16, 16, 4))
    got = act_calls(L, h, ga, gy=gy, want=("gb1",))
    ref = R.act_maps(h.double(), ga.double())
    e1, b1 = R.rel_err(got["g_b1"], ref["g_b1"]), 4 * R.rel_err((ga * R.gelu_grad(h)).sum(0), ref["g_b1"])
    e2, b2 = R.rel_err(got["g_b2"], gy.double().sum(0)), 4 * R.rel_err(gy.sum(0), gy.double().sum(0))
    print("g_b1 err %.3e bound %.3e   g_b2 err %.3e bound %.3e" % (e1, b1, e2, b2))
    assert e1 <= b1 and e2 <= b2


# ------------------------------------------------------------------------------------------------ idle vector slots behind the first column tile
RAGGED = ((2, 3, 7), 20, 136, 68)          # Hd = 136: 17 vectors of 8 on three tiles of L = 8 in a half type; Co = 68: the same with vectors of 4
PRECISIONS = {"fp32": (torch.float32, None), "fp64": (torch.float64, None), "fp16": (torch.float32, torch.float16), "bf16": (torch.float32, torch.bfloat16)}


@functools.lru_cache(maxsize=None)
def ragged_case():
    """inputs and the eager lines in fp64 on the device (computed once, shared, never modified)"""
    ins = R.draw("ragged", 78, RAGGED)
    return ins, run_eager(ins, torch.float64)


def test_the_ragged_widths_have_idle_slots_behind_the_first_tile():
    (_, _, Hd, Co) = RAGGED
    for dt, N in (("f16", Hd), ("bf16", Hd), ("f32", Co), ("f64", Co), ("f16", Co)):
        e = TP.plan_extra("pw_mlp", "", dt, N)
        assert e["gx"] > 1 and e["idle"] > 0, (dt, N, e)


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("prec", sorted(PRECISIONS))
def test_ragged_widths_against_the_eager_lines(L, prec, keep):
    """ops.pw_mlp where the last column tile has idle vector slots, against the eager lines in fp64 on the same device: 1e-12 for fp64, else
    4 x the deviation of the eager lines in the same precision (fp32, or fp32 tensors under fp16 / bf16 autocast), per result"""
    dtype, autocast = PRECISIONS[prec]
    ins, ref = ragged_case()
    got, tags = _traced(L, lambda: run_op(ins, dtype, keep, autocast=autocast))
    dt = {"fp32": "f32", "fp64": "f64", "fp16": "f16", "bf16": "bf16"}[prec]
    assert tags.get("pw_mlp act_fwd" + _cls(dt, RAGGED[2])) == 1 and tags.get("pw_mlp colsum" + _cls(dt, RAGGED[3])) == 1, tags
    eager = None if prec == "fp64" else run_eager(ins, dtype, autocast=autocast)
    bad = {}
    for n in R.RESULTS:
        err = R.rel_err(got[n], ref[n])
        bound = 1e-12 if eager is None else 4 * R.rel_err(eager[n], ref[n])
        print("ragged %s %s %-5s err %.3e  bound %.3e" % (prec, keep, n, err, bound))
        assert eager is None or got[n].dtype == eager[n].dtype, n
        if not (got[n].shape == ref[n].shape and err <= bound):
            bad[n] = (err, bound)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ need flags, saved tensors, memory, M = 0
NEEDS = {"all": ((True,) * 5, 3), "t": ((True, False, False, False, False), 1), "w2": ((False, False, False, True, False), 1),
         "b2": ((False, False, False, False, True), 2), "b1": ((False, False, True, False, False), 2),
         "w1+b1": ((False, True, True, False, False), 2), "none": ((False,) * 5, 0)}


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("which", sorted(NEEDS))
def test_need_flags(L, which, keep):
    """only what autograd asks for is computed: the other gradients are None, the wanted ones keep their bits, and the launches are counted by
    their `pw_mlp ` tags: one forward; backward 3 with everything (map, column sum, reduce), 1 for t alone (no sums, no reduce), 1 for w2 alone
    (a only), 2 for b2 alone (column sum + reduce)"""
    need, launches = NEEDS[which]
    ins = fixture_inputs(R.load_case("c24"))
    full = run_op(ins, torch.float32, keep)
    got, tags = _traced(L, lambda: run_op(ins, torch.float32, keep, need=need))
    assert torch.equal(got["y"], full["y"])
    for n, k in zip(GRADS, need):
        if k:
            assert torch.equal(got[n], full[n]), n
        else:
            assert got[n] is None, n
    count = lambda key: sum(v for t, v in tags.items() if t == "pw_mlp " + key)          # noqa: E731
    (_, Cc, Hd, Co) = R.CASES["c24"]
    hid, out = _cls("f32", Hd), _cls("f32", Co)                      # '<f32,V=4> L=8' at both widths of c24
    assert count("act_fwd" + hid) == 1 and sum(tags.values()) == 1 + launches, tags
    nt, nw1, nb1, nw2, nb2 = need
    if nt or nw1 or nb1 or nw2:
        flags = "a=%d gh=%d gb=%d" % (nw2, nt or nw1, nb1)
        assert count("act_bwd%s %s" % (hid, flags)) == 1, tags
    else:
        assert not [t for t in tags if t.startswith("pw_mlp act_bwd")], tags
    assert count("colsum" + out) == int(nb2) and count("reduce<f32>") == int(nb1 or nb2), tags


def _cls(dt, N):
    """the plan class `<dt,V=..> L=..` of width N with the L the host code lists (train_plan_check --list), not a retyped one"""
    V = 8 if dt in ("f16", "bf16") and N % 8 == 0 else 4
    return "<%s,V=%d> L=%d" % (dt, V, TP.plan_extra("pw_mlp", "", dt, N)["L"])


def test_the_variant_tags_name_dtype_and_width(L):
    """the map kernels over the hidden units carry the class of Hd, the column sum of grad_y that of Co"""
    want = {("c24", torch.float16): ("f16", 8, 8), ("h100", torch.float16): ("f16", 4, 4), ("c48", torch.bfloat16): ("bf16", 8, 8)}
    for (tag, half), (dt, v_hid, v_out) in want.items():
        (_, Cc, Hd, Co) = R.CASES[tag]
        hid, out = _cls(dt, Hd), _cls(dt, Co)
        assert hid.startswith("<%s,V=%d> L=" % (dt, v_hid)) and out.startswith("<%s,V=%d> L=" % (dt, v_out))
        ins = fixture_inputs(R.load_case(tag))
        _, tags = _traced(L, lambda: run_op(ins, torch.float32, autocast=half))
        assert tags == {"pw_mlp act_fwd" + hid: 1, "pw_mlp act_bwd%s a=1 gh=1 gb=1" % hid: 1, "pw_mlp colsum" + out: 1, "pw_mlp reduce<f32>": 1}, (tag, tags)
    (_, Cc, Hd, Co) = R.CASES["small"]
    _, tags = _traced(L, lambda: run_op(fixture_inputs(R.load_case("small")), torch.float64))
    assert tags == {"pw_mlp act_bwd%s a=1 gh=1 gb=1" % _cls("f64", Hd): 1, "pw_mlp act_fwd" + _cls("f64", Hd): 1, "pw_mlp colsum" + _cls("f64", Co): 1,
                    "pw_mlp reduce<f64>": 1}, tags
    assert _cls("f64", Hd) == "<f64,V=4> L=4" and _cls("f64", Co) == "<f64,V=4> L=1" and _cls("f16", 96) == "<f16,V=8> L=16"       # the format, once


@pytest.mark.parametrize("autocast", [None, torch.float16], ids=["fp32", "fp16-autocast"])
def test_what_autograd_keeps(L, autocast):
    from unicorn_amd.ops import pw_mlp
    (nhw, Cc, Hd, Co) = R.CASES["c24"]
    M = nhw[0] * nhw[1] * nhw[2]
    cd = autocast or torch.float32
    for keep in KEEPS:
        t, w1, b1, w2, b2 = _leaves(fixture_inputs(R.load_case("c24")), torch.float32, (True,) * 5)
        with torch.autocast("cuda", dtype=torch.float16, enabled=autocast is not None):
            y = pw_mlp(t, w1, b1, w2, b2, keep=keep)
            h = F.linear(t, w1, b1).detach()
        saved = y.grad_fn.saved_tensors
        ptrs = {s.data_ptr() for s in saved}
        big = [s for s in saved if s.numel() == M * Hd]
        assert w1.data_ptr() in ptrs and w2.data_ptr() in ptrs and b2.data_ptr() not in ptrs and y.data_ptr() not in ptrs
        kept_t = [s for s in saved if tuple(s.shape) == (M, Cc)]
        assert len(kept_t) == 1 and kept_t[0].dtype == cd and (autocast is not None or kept_t[0].data_ptr() == t.data_ptr())
        if keep == "hidden":
            assert sorted(tuple(s.shape) for s in saved) == sorted([(M, Cc), (Hd, Cc), (Co, Hd), (M, Hd)])
            assert len(big) == 1 and big[0].dtype == cd and torch.equal(big[0], h.reshape(M, Hd))       # h with eager's bits, not gelu(h)
            assert b1.data_ptr() not in ptrs
        else:
            assert sorted(tuple(s.shape) for s in saved) == sorted([(M, Cc), (Hd, Cc), (Hd,), (Co, Hd)])
            assert not big and b1.data_ptr() in ptrs
        y.backward(torch.ones_like(y))
        if keep == "hidden":
            assert torch.equal(big[0], h.reshape(M, Hd)), "h is a saved tensor and is never written"


def test_bytes_held_between_forward_and_backward(L):
    """A condition from the shapes, not a measurement: k = 3 operators in a row, M = 4096, C = 32, Hd = 128, fp32 (every map a multiple of
    512 bytes).  The eager lines keep h and gelu(h) per operator, keep="hidden" h alone, keep="input" neither."""
    from unicorn_amd.ops import pw_mlp
    k, M, Cc, Hd = 3, 4096, 32, 128
    g = torch.Generator().manual_seed(0)
    params = [[x.to(DEV).requires_grad_(True) for x in R.draw("net", 10 + i, ((M,), Cc, Hd, Cc))[1:5]] for i in range(k)]
    x = torch.randn(M, Cc, generator=g).to(DEV)

    def held(step):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        y = x
        for p in params:
            y = step(y, *p)
        torch.cuda.synchronize()
        now = torch.cuda.memory_allocated() - base
        y.sum().backward()
        for p in params:
            for q in p:
                q.grad = None
        return now

    eager = held(lambda t, w1, b1, w2, b2: F.linear(F.gelu(F.linear(t, w1, b1)), w2, b2))
    hidden = held(lambda t, w1, b1, w2, b2: pw_mlp(t, w1, b1, w2, b2, keep="hidden"))
    inp = held(lambda t, w1, b1, w2, b2: pw_mlp(t, w1, b1, w2, b2, keep="input"))
    one = k * M * Hd * 4
    print("bytes held: eager %d, hidden %d, input %d; one hidden map per operator = %d" % (eager, hidden, inp, one))
    assert eager - hidden >= 0.95 * one and eager - inp >= 0.95 * 2 * one


def test_empty_batch(L):
    from unicorn_amd.ops import pw_mlp
    t, w1, b1, w2, b2 = _leaves(R.draw("e", 1, ((0, 3, 3), 8, 32, 12))[:5], torch.float32, (True,) * 5)

    def go():
        y = pw_mlp(t, w1, b1, w2, b2)
        y.sum().backward()
        return y

    y, tags = _traced(L, go)
    assert not tags
    assert tuple(y.shape) == (0, 3, 3, 12) and tuple(t.grad.shape) == (0, 3, 3, 8)
    for p in (w1, b1, w2, b2):
        assert p.grad.shape == p.shape and not p.grad.any()


# ------------------------------------------------------------------------------------------------ the drop-in on a stand-in mini-backbone
def _proto():
    torch.manual_seed(5)
    net = R.MiniBackbone(16)
    with torch.no_grad():
        for blk in (net.block1, net.block2):
            blk.dwconv.bias.normal_(0, 0.1), blk.norm.weight.normal_(1, 0.1), blk.norm.bias.normal_(0, 0.1)
    return net


def _run_net(proto, x, t, dtype, keep, autocast=False, train=True):
    """one forward (+ backward in training mode) of a copy of `proto`, fused with fuse_backbone_mlp(keep) unless keep is None"""
    from unicorn_amd.nn import fuse_backbone_mlp
    net = copy.deepcopy(proto).to(DEV, dtype).train(train)
    if keep:
        assert fuse_backbone_mlp(net, keep) == (2, 2, 3, 2)
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
    return proto, x, t, _run_net(proto, x, t, torch.float64, None)


@pytest.mark.parametrize("keep", KEEPS)
def test_fused_backbone_against_the_unfused_one_fp64(L, keep):
    proto, x, t, exact = _net_case()
    (fused, tags) = _traced(L, lambda: _run_net(proto, x, t, torch.float64, keep))
    assert sum(v for k, v in tags.items() if k.startswith("pw_mlp act_fwd")) == 2, tags       # both blocks ran the operator
    assert sorted(fused) == sorted(exact)
    for n in exact:
        err = R.rel_err(fused[n], exact[n])
        print("%-24s %s fused vs unfused %.3e" % (n, keep, err))
        assert err <= 1e-10, (n, err)


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("autocast", [False, True], ids=["fp32", "fp16-autocast"])
def test_fused_backbone_against_the_unfused_one_fp32(L, autocast, keep):
    """each run is compared with the unfused fp64 run, and the fused one may be at most 4 x as far from it as the unfused one is, per quantity"""
    proto, x, t, exact = _net_case()
    plain = _run_net(proto, x, t, torch.float32, None, autocast=autocast)
    fused = _run_net(proto, x, t, torch.float32, keep, autocast=autocast)
    bad = {}
    for n in exact:
        err, bound = R.rel_err(fused[n], exact[n]), 4 * R.rel_err(plain[n], exact[n])
        print("%-24s %s fused %.3e  bound %.3e" % (n, keep, err, bound))
        assert fused[n].dtype == plain[n].dtype, n
        if not err <= bound:
            bad[n] = (err, bound)
    assert not bad, bad


def test_fused_backbone_in_eval_mode_is_the_unfused_one(L):
    proto, x, t, _ = _net_case()
    fused, plain = _run_net(proto, x, t, torch.float32, "hidden", train=False), _run_net(proto, x, t, torch.float32, None, train=False)
    assert torch.equal(fused["out"], plain["out"])


@pytest.mark.parametrize("keep", KEEPS)
def test_seeded_drop_path_drops_the_same_samples(L, keep):
    from unicorn_amd.nn import fuse_backbone_mlp
    torch.manual_seed(5)
    proto = RB.StandInBlock(16, drop_path=0.5)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(4, 16, 6, 7, generator=g)
    torch.manual_seed(3)
    mask = torch.empty((4, 1, 1, 1), dtype=torch.float32, device=DEV).bernoulli_(0.5).flatten().tolist()
    assert 0.0 in mask and 1.0 in mask, mask
    outs = []
    for fuse in (False, True):
        net = copy.deepcopy(proto).to(DEV).train()
        if fuse:
            assert fuse_backbone_mlp(net, keep) == (1, 1, 0, 1)
        torch.manual_seed(3)
        outs.append(net(x.to(DEV)).detach().cpu())
    dropped = [[bool(torch.equal(o[n], x[n])) for n in range(4)] for o in outs]
    assert dropped[0] == dropped[1] == [m == 0.0 for m in mask]
