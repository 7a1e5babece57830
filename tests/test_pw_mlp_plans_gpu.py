"""Every launch plan of pw_mlp's map kernel (csrc/pw_mlp.hip, pw_plan in csrc/train_plan.h) is found, listed and run against a reference, through
the C-ABI alone (uni_pw_mlp_act_fwd / _bwd and their _f64 twins; no GEMM on either side).  tests/train_plans.py holds the list
(EXPECTED_PW: a class is `<dtype,V=..> L=..`), the three widths of a class and the two row counts.

  1. sweep and closure   act_fwd at one row for every N = 4, 8, ..., 8192, traced, per element type: each launch leaves one tag, its class is
                         the one `train_plan_check --list` gives at that N, and the classes found are exactly the listed ones, in both
                         directions; {class: [N min, N max, count]} goes to pw_mlp_plan_census.json in the suite's results directory
  2. parity per class    three shapes per class -- its smallest and its largest N at M_short rows (two groups, the second partial), and at
                         M_loop rows (more groups than rows of partials: the blocks loop) the smallest N whose last column tile has idle
                         vector slots behind a first tile -- each with act_fwd, act_bwd with a, grad_h and grad_b1, and the column sums of a
                         grad_y of the same width, so the colsum launch and the second job of the reduce run the class as well; the act_fwd,
                         act_bwd and colsum tags must each name the class under test.  Reference: the restatement (pw_mlp_ref.act_maps) and
                         plain column sums in fp64 on the rounded inputs.  fp64: 1e-12.  fp32: 4 x the larger of the restatement's own fp32
                         deviation on the CPU and that of eager F.gelu + autograd / torch.sum in fp32 on the device, both on the same inputs.
                         fp16 / bf16: that plus half an ulp on a and grad_h (one rounding to the element type); the sums are fp32 and get
                         none.  Where a yardstick is zero -- the column sums of a few fp16 / bf16 values of grad_y are exact in fp32 on the
                         CPU and on the device alike -- the sum is a number of fp32 and the kernel, which adds in double, is held to it
                         exactly.  A second call and the in-place forms give the bits of the first.
  3. exact rows          the same shapes with h = 30 and small integers for grad_a and grad_y: a == h, grad_h == grad_a and both sums are
                         integers below 2^24 in every arithmetic, held to the last bit

No bound comes from a kernel.  Failures are collected per class and reported once; no case is skipped."""
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import pw_mlp_ref as R  # noqa: E402
import train_plans as P  # noqa: E402
import variant_cases as vc  # noqa: E402
from pw_mlp_calls import DEV, H_DTYPE, P as ptr, act_calls, traced  # noqa: E402

DT = {"f32": torch.float32, "f64": torch.float64, "f16": torch.float16, "bf16": torch.bfloat16}
HALF_ULP = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}          # one rounding to nearest, relative to the largest value
MAPS = ("a_fwd", "a", "grad_h")
KEY = {"a_fwd": "a", "a": "a", "grad_h": "grad_h", "g_b1": "g_b1", "g_b2": "g_b2"}


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def _report(bad):
    return "%d case(s) failed: %s\n%s" % (len(bad), ", ".join(bad), "\n".join("  %s: %s" % kv for kv in bad.items()))


# ================================================================================================================ 1. sweep and closure
@functools.lru_cache(maxsize=None)
def sweep(dt):
    """{N: plan class} of act_fwd on one row, one launch per N"""
    from unicorn_amd import _lib
    lib = _lib.lib()
    f64 = dt == "f64"
    fwd = getattr(lib, "uni_pw_mlp_act_fwd" + ("_f64" if f64 else ""))
    h = torch.randn(P.N_MAX, generator=torch.Generator().manual_seed(1)).to(DEV, DT[dt])
    a = torch.empty_like(h)
    s = _lib.stream_ptr()
    found = {}
    try:
        for N in P.SWEEP_N:
            lib.uni_variant_trace(1)
            _lib.check(fwd(ptr(h), H_DTYPE[DT[dt]], 1, N, ptr(a), s), "uni_pw_mlp_act_fwd")
            tags = vc.read_trace(lib)
            assert len(tags) == 1 and sum(tags.values()) == 1, (dt, N, tags)
            kind, cls = P.pw_tag(next(iter(tags)))
            assert kind == "act_fwd", (dt, N, tags)
            found[N] = cls
    finally:
        lib.uni_variant_trace(0)
    torch.cuda.synchronize()
    return found


@pytest.mark.parametrize("dt", P.PW_DTYPES)
def test_sweep_finds_exactly_the_listed_classes(L, dt):
    by_n = sweep(dt)
    assert sorted(by_n) == list(P.SWEEP_N)
    found = P.group(by_n)
    want = [c for c in P.EXPECTED_PW if c.startswith("<%s," % dt)]
    for cls, ns in found.items():
        print("%-20s N %4d .. %4d  (%d widths)" % (cls, ns[0], ns[-1], len(ns)))
    extra, missing = sorted(set(found) - set(want)), sorted(set(want) - set(found))
    assert not extra and not missing, "launched but not listed: %s; listed but never launched: %s" % ({c: found[c][:3] for c in extra}, missing)
    off = {N: (cls, P.predicted("pw_mlp", "", dt, N)) for N, cls in by_n.items() if cls != P.predicted("pw_mlp", "", dt, N)}
    assert not off, "launcher and `train_plan_check --list` disagree: %s" % dict(sorted(off.items())[:8])


def test_the_census_lists_every_class_with_its_range(L):
    census, launches = {}, 0
    for dt in P.PW_DTYPES:
        found = sweep(dt)
        launches += len(found)
        for cls, ns in P.group(found).items():
            assert cls not in census, "one class from two sweeps: %s" % cls
            census[cls] = [ns[0], ns[-1], len(ns)]
    assert sorted(census) == sorted(P.EXPECTED_PW), sorted(set(census) ^ set(P.EXPECTED_PW))
    assert launches == len(P.PW_DTYPES) * len(P.SWEEP_N) and sum(v[2] for v in census.values()) == launches
    print("%d sweep launches, %d classes" % (launches, len(census)))
    out = guard.results_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "pw_mlp_plan_census.json"), "w") as f:
        json.dump({"pw_mlp": census, "sweep_launches": launches, "first_run": P.pw_first_run()}, f, indent=1, sort_keys=True)


# ================================================================================================================ 2. parity per class
def _trace_ok(tags, cls):
    """forward, backward map, column sum and reduce: four launches, the three map kernels in the class under test"""
    kinds = sorted(P.pw_tag(t) for t in tags if P.pw_tag(t) is not None)
    return kinds == [("act_bwd", cls), ("act_fwd", cls), ("colsum", cls)] and sum(tags.values()) == 4 and \
        "pw_mlp act_bwd%s a=1 gh=1 gb=1" % cls in tags and any(t.startswith("pw_mlp reduce<") for t in tags)


@functools.lru_cache(maxsize=None)
def parity_case(dt, M, N):
    """-> device inputs of type dt, the fp64 reference on those rounded inputs, and the fp32 yardstick per result: the larger of the restatement's
    own fp32 deviation on the CPU and that of the eager fp32 lines on the device.  Computed once per case, shared, never modified."""
    h, ga, gy = (t.to(DT[dt]) for t in R.draw_maps(M, N, N))
    ref = R.act_maps(h.double(), ga.double())
    ref["g_b2"] = gy.double().sum(0)
    yard = None
    if dt != "f64":
        f32 = R.act_maps(h.float(), ga.float())
        f32["g_b2"] = gy.float().sum(0)
        he = h.to(DEV, torch.float32).requires_grad_(True)
        ae = F.gelu(he)
        ae.backward(ga.to(DEV, torch.float32))
        eager = {"a": ae.detach(), "grad_h": he.grad, "g_b1": he.grad.sum(0), "g_b2": gy.to(DEV, torch.float32).sum(0)}
        yard = {n: (R.rel_err(f32[n], ref[n]), R.rel_err(eager[n], ref[n])) for n in ref}
    return (h.to(DEV), ga.to(DEV), gy.to(DEV)), ref, yard


def parity_check(L, bad, dt, cls, M, N):
    key = "%s M=%d N=%d" % (cls, M, N)
    (h, ga, gy), ref, yard = parity_case(dt, M, N)
    got, tags = traced(L, lambda: act_calls(L, h, ga, gy=gy))
    if not _trace_ok(tags, cls):
        bad.setdefault(key, {})["trace"] = tags
    again, inpl = act_calls(L, h, ga, gy=gy), act_calls(L, h, ga, gy=gy, inplace=True)
    sdt = torch.float64 if dt == "f64" else torch.float32
    for n in MAPS + ("g_b1", "g_b2"):
        k = KEY[n]
        err = R.rel_err(got[n], ref[k])
        bound = 1e-12 if dt == "f64" else 4 * max(yard[k]) + (HALF_ULP.get(dt, 0.0) if n in MAPS else 0.0)
        print("%-36s %-6s err %.3e  bound %.3e%s" % (key, n, err, bound, "" if yard is None else "  (restatement %.3e, eager %.3e)" % yard[k]))
        if not (got[n].shape == ref[k].shape and got[n].dtype == (DT[dt] if n in MAPS else sdt) and err <= bound):
            bad.setdefault(key, {})[n] = (err, bound)
        if not torch.equal(got[n], again[n]):
            bad.setdefault(key, {})[n + " (second call)"] = "differs"
        if not torch.equal(got[n], inpl[n]):
            bad.setdefault(key, {})[n + " (in place)"] = "differs"
    if not torch.equal(got["a_fwd"], got["a"]):
        bad.setdefault(key, {})["a of the backward"] = "differs from the forward's"


@pytest.mark.parametrize("dt", P.PW_DTYPES)
def test_parity_at_three_shapes_of_every_class(L, dt):
    shapes = P.pw_shapes(dt)
    assert {c for c, _, _ in shapes} == set(P.group(sweep(dt)))          # the classes the device launches, each of them
    bad = {}
    for cls, M, N in shapes:
        parity_check(L, bad, dt, cls, M, N)
    parity_case.cache_clear()                                            # the inputs are on the device
    assert not bad, _report(bad)


# ================================================================================================================ 3. exact rows and columns
@pytest.mark.parametrize("dt", P.PW_DTYPES)
def test_exact_rows_and_columns_at_three_shapes_of_every_class(L, dt):
    bad = {}
    for cls, M, N in P.pw_shapes(dt):
        key = "%s M=%d N=%d" % (cls, M, N)
        h, ga, gy, s1, s2 = R.exact_maps(M, N, N, DT[dt], DEV)
        got, tags = traced(L, lambda: act_calls(L, h, ga, gy=gy))
        if not _trace_ok(tags, cls):
            bad.setdefault(key, {})["trace"] = tags
        sdt = torch.float64 if dt == "f64" else torch.float32
        for n, want in (("a_fwd", h), ("a", h), ("grad_h", ga), ("g_b1", s1.to(sdt)), ("g_b2", s2.to(sdt))):
            if not (got[n].dtype == want.dtype and torch.equal(got[n], want)):
                wrong = (got[n] != want).nonzero()
                bad.setdefault(key, {})[n] = "%d elements differ, the first at %s" % (len(wrong), wrong[0].tolist())
    assert not bad, _report(bad)
