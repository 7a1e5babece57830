"""The four ConvNeXt training operators through the C-ABI at maps whose element offsets pass 2^31 (pw_mlp: 2^32 as well), and the column sums
of pw_mlp at training row counts.  tests/train_scale.py holds the shapes, the memory arithmetic, the inputs, the chunked fp64 references and
the checking functions; tests/test_train_scale_cpu.py checks those without a device.

  A. one case per operator, layout and kernel family (train_scale.PW_A, BT_A, LN_A, DW_A), each with at least 2^24 elements behind the
     boundary and ragged in every tiled axis.  Every output is filled with NaN before the call; values are held to the operator's existing
     rule (4 x the fp32 yardstick measured in the same pass, half an ulp more on a half map; parameter gradients against chunk-accumulated
     fp64 sums), a second call gives the bits of the first, pw_mlp's in-place forms give the bits of the out-of-place ones, and pw_mlp and
     block_tail run once more on small integers, held to the last bit.  dwln_train is judged in three bands of image rows (the first, the
     last, those around offset 2^31) against dwln_train_ref in fp64, its parameter gradients against a whole-map fp64 accumulation of shifted
     multiply-adds; its second grad_x is compared by a position-weighted digest of the bits, there being no room for a second map.
  B. grad_b1 / grad_b2 where a lane adds 1025 rows serially (train_scale.PW_B), zero-mean and mean-1 draws judged apart, fp32 and fp16.

The _f64 forms are not run at this size: they double the memory and share every index expression with the fp32 forms through the templates.
Maps past 2^32 elements are run for pw_mlp only.  Each case states its memory need, skips only where the device has less than 1.1 x that
free (saying both numbers), frees its buffers in a `finally`, and leaves a record (shape, elements, peak bytes, wall time, err / bound per
result, terms per lane) in train_scale.json in the suite's results directory.  No bound is a number picked in advance."""
import ctypes as C
import json
import os
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard  # noqa: E402
import train_plans as P  # noqa: E402
import train_scale as S  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
_RECORDS = {}


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    yield _lib
    out = guard.results_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "train_scale.json"), "w") as f:
        json.dump(_RECORDS, f, indent=1, sort_keys=True)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


class Run:
    """one case: the memory gate before, the record and the release after"""

    def __init__(self, key, shape, elems, need, terms=None):
        self.key, self.shape, self.elems, self.need, self.terms = key, shape, elems, need, terms
        self.results, self.tags = {}, {}

    def __enter__(self):
        assert self.need <= S.CAP, "%s needs %d bytes, more than the cap of %d" % (self.key, self.need, S.CAP)
        torch.cuda.empty_cache()
        free = torch.cuda.mem_get_info()[0]
        if free < 1.1 * self.need:
            pytest.skip("%s needs %d bytes of device memory (x 1.1), %d are free" % (self.key, self.need, free))
        torch.cuda.reset_peak_memory_stats()
        self.t0 = time.time()
        return self

    def take(self, name, rep):
        """print a Report, keep its figures, -> its failures"""
        for line in rep.lines():
            print("%-28s %-14s %s" % (self.key, name, line))
        self.results[name] = {k: {"err_before": v[0], "err_behind": v[1], "bound": v[2]} for k, v in rep.items()}
        self.results[name].update({"exact " + k: (v or "equal") for k, v in rep.wrong.items()})
        if rep.notes:
            self.results[name]["notes"] = rep.notes
        return ["%s %s" % (name, f) for f in rep.failures()]

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated()
        _RECORDS[self.key] = {"shape": self.shape, "elements": self.elems, "need_bytes": self.need, "peak_bytes": peak,
                              "wall_s": round(time.time() - self.t0, 2), "terms_per_lane": self.terms, "results": self.results,
                              "tags": sorted(self.tags)}
        print("%-28s %s  %.3e elements  peak %.2f GiB of %.2f stated  %.1f s" % (self.key, self.shape, self.elems, peak / 2 ** 30,
                                                                              self.need / 2 ** 30, time.time() - self.t0))
        torch.cuda.empty_cache()
        if exc[0] is None:
            assert peak <= self.need, "%s took %d bytes at its peak, %d were stated" % (self.key, peak, self.need)
        return False


def traced(L, fn, prefix):
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        fn()
    finally:
        lib.uni_variant_trace(0)
    return {t: v for t, v in vc.read_trace(lib).items() if t.startswith(prefix)}


# ================================================================================================================ pw_mlp
def pw_fwd(L, case, h, a):
    L.check(L.lib().uni_pw_mlp_act_fwd(ptr(h), S.CODE[case.dt], case.M, case.Hd, ptr(a), L.stream_ptr()), "uni_pw_mlp_act_fwd")


def pw_bwd(L, case, h, ga, a, gh, gb1, gy, gb2, ws):
    L.check(L.lib().uni_pw_mlp_act_bwd(ptr(h), S.CODE[case.dt], ptr(ga), case.M, case.Hd, ptr(a), ptr(gh), ptr(gb1), ptr(gy), case.Co, ptr(gb2),
                                       ptr(ws), ws.numel() if ws is not None else 0, L.stream_ptr()), "uni_pw_mlp_act_bwd")


def pw_workspace(L, case):
    need = L.lib().uni_pw_mlp_workspace_bytes(case.M, case.Hd, case.Co)
    assert need == 4 * 256 * (case.Hd + case.Co)
    return torch.empty(need, dtype=torch.uint8, device=DEV)


def pw_family_ok(tags, dt, Hd, Co):
    """the forward, the backward map and the column sum each ran the class the host plan gives for this width"""
    kinds = {P.pw_tag(t) for t in tags} - {None}
    return kinds == {("act_fwd", P.predicted("pw_mlp", "", dt, Hd)), ("act_bwd", P.predicted("pw_mlp", "", dt, Hd)),
                     ("colsum", P.predicted("pw_mlp", "", dt, Co))}


def pw_outputs(L, case, forms, bad, run):
    """-> (a, grad_h, g_b1, g_b2, grad_y) after every call of the case and every bit comparison between them; `out` in forms: the out-of-place
    calls are the ones judged and the in-place ones must give their bits; else the in-place calls, twice"""
    M, Hd, Co = case.M, case.Hd, case.Co
    ws = pw_workspace(L, case)
    H, G = (case.fill(n, torch.empty(M, Hd, dtype=case.dtype, device=DEV)) for n in ("h", "ga"))
    Y = case.fill("gy", torch.empty(M, Co, dtype=case.dtype, device=DEV))
    sums = lambda: (nan(Hd), nan(Co))                                              # noqa: E731
    if "out" in forms:
        A, D = nan(M, Hd, dtype=case.dtype), nan(M, Hd, dtype=case.dtype)
        g1, g2 = sums()

        run.tags.update(traced(L, lambda: pw_bwd(L, case, H, G, A, D, g1, Y, g2, ws), "pw_mlp "))
        h1, h2 = sums()
        pw_bwd(L, case, H, G, H, G, h1, Y, h2, ws)                                 # in place: the second call as well
        torch.cuda.synchronize()
        for n, x, y in (("a", H, A), ("grad_h", G, D), ("g_b1", h1, g1), ("g_b2", h2, g2)):
            if not S.same_bits(x, y):
                bad.append("%s in place differs from out of place" % n)
        case.fill("h", H)
        G.fill_(float("nan"))
        run.tags.update(traced(L, lambda: pw_fwd(L, case, H, G), "pw_mlp "))         # forward, out of place
        pw_fwd(L, case, H, H)                                                      # and in place
        torch.cuda.synchronize()
        for n, x in (("out of place", G), ("in place", H)):
            if not S.same_bits(x, A):
                bad.append("a of the forward (%s) differs from the backward's" % n)
        del H
        return A, D, g1, g2, Y, (G if case.dt == "f32" else None)
    g1, g2 = sums()
    run.tags.update(traced(L, lambda: pw_bwd(L, case, H, G, H, G, g1, Y, g2, ws), "pw_mlp "))
    A, D = H.clone(), G.clone()
    case.fill("h", H), case.fill("ga", G)
    h1, h2 = sums()
    pw_bwd(L, case, H, G, H, G, h1, Y, h2, ws)
    torch.cuda.synchronize()
    for n, x, y in (("a", H, A), ("grad_h", G, D), ("g_b1", h1, g1), ("g_b2", h2, g2)):
        if not S.same_bits(x, y):
            bad.append("%s differs in the second call" % n)
    del D
    case.fill("h", A)
    run.tags.update(traced(L, lambda: pw_fwd(L, case, A, A), "pw_mlp "))
    torch.cuda.synchronize()
    if not S.same_bits(A, H):
        bad.append("a of the forward (in place) differs from the backward's")
    del A
    return H, G, g1, g2, Y, None


@pytest.mark.parametrize("tag", sorted(S.PW_A))
def test_pw_mlp_past_the_boundary(L, tag):
    dt, M, Hd, Co, boundary, forms = S.PW_A[tag]
    assert M * Hd >= boundary + S.BEHIND and boundary // Hd < M
    bad = []
    with Run("pw_mlp A " + tag, "M=%d Hd=%d Co=%d %s %s" % (M, Hd, Co, dt, "+".join(forms)), M * Hd, S.pw_need(tag)) as run:
        try:
            case = S.PwCase(dt, M, Hd, Co)
            a, gh, g1, g2, gy, scratch = pw_outputs(L, case, forms, bad, run)
            if scratch is None:
                torch.cuda.empty_cache()
            bad += run.take("values", S.pw_check(case, {"a": a, "grad_h": gh, "g_b1": g1, "g_b2": g2}, boundary, scratch=scratch, gy=gy))
            if not pw_family_ok(run.tags, dt, Hd, Co):
                bad.append("trace: %s" % sorted(run.tags))
            del a, gh, gy, scratch
            torch.cuda.empty_cache()
            # small integers: the last bit.  Base 0 where 3 M would pass 2^24
            exact = S.PwCase(dt, M, Hd, Co, exact=1 if 3 * M < 2 ** 24 else 0)
            a, gh, g1, g2, gy, scratch = pw_outputs(L, exact, forms, bad, run)
            bad += run.take("integers", S.pw_check_exact(exact, {"a": a, "grad_h": gh, "g_b1": g1, "g_b2": g2}))
        finally:
            a = gh = gy = scratch = g1 = g2 = None
            torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mean", S.PW_B_MEANS, ids=["mean0", "mean1"])
@pytest.mark.parametrize("tag", sorted(S.PW_B))
def test_pw_mlp_sums_of_training_length(L, tag, mean):
    """grad_b1 (the unrounded grad_h) and grad_b2 where a lane adds 1025 terms serially, against chunk-accumulated fp64 sums; the bound is 4 x the
    error of torch's fp32 sum(0) of the same device values"""
    dt, M, N, lanes, terms = S.PW_B[tag]
    bad = []
    with Run("pw_mlp B %s mean=%g" % (tag, mean), "M=%d Hd=Co=%d %s" % (M, N, dt), M * N, S.pw_b_need(tag), terms) as run:
        try:
            case = S.PwCase(dt, M, N, N, mean=mean, seed=53)
            ws = pw_workspace(L, case)
            H, G, Y = (case.fill(n, torch.empty(M, N, dtype=case.dtype, device=DEV)) for n in ("h", "ga", "gy"))
            g1, g2, h1, h2 = nan(N), nan(N), nan(N), nan(N)
            run.tags.update(traced(L, lambda: pw_bwd(L, case, H, G, None, None, g1, Y, g2, ws), "pw_mlp "))
            pw_bwd(L, case, H, G, None, None, h1, Y, h2, ws)
            torch.cuda.synchronize()
            if not (torch.equal(g1, h1) and torch.equal(g2, h2)):
                bad.append("the second call differs")
            cls = P.predicted("pw_mlp", "", dt, N)
            if {P.pw_tag(t) for t in run.tags} - {None} != {("act_bwd", cls), ("colsum", cls)} or P.pw_lanes(cls) != lanes:
                bad.append("trace: %s" % sorted(run.tags))
            del H, G
            bad += run.take("sums", S.pw_check(case, {"g_b1": g1, "g_b2": g2}, gy=Y))
        finally:
            H = G = Y = None
            torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


# ================================================================================================================ block_tail
def bt_calls(L, case, y, x, gamma, scale, out, gy, gg, ws):
    B, Cc, H, W = case.shape
    lib, s = L.lib(), L.stream_ptr()
    if out is not None:
        L.check(lib.uni_block_tail_fwd(ptr(y), S.CODE[case.dt], ptr(x), case.nchw, ptr(gamma), ptr(scale), B, H, W, Cc, ptr(out), s), "uni_block_tail_fwd")
    if gy is not None or gg is not None:
        L.check(lib.uni_block_tail_bwd(ptr(y), S.CODE[case.dt], ptr(x), case.nchw, ptr(gamma), ptr(scale), B, H, W, Cc, ptr(gy), ptr(gg), ptr(ws),
                                       ws.numel(), s), "uni_block_tail_bwd")
    torch.cuda.synchronize()


def bt_run(L, case, boundary, bad, run, name):
    B, Cc, H, W = case.shape
    M = case.M
    need = L.lib().uni_block_tail_workspace_bytes(B, H, W, Cc)
    assert need == 4 * 1024 * Cc
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    gamma, scale = case.gamma.to(DEV), case.scale.to(DEV)
    y = case.fill(case.y, torch.empty(M, Cc, dtype=case.dtype, device=DEV), 0)
    x = case.fill(case.x, torch.empty(M * Cc, dtype=torch.float32, device=DEV), case.nchw)
    out, out2 = nan(M, Cc), nan(M, Cc)
    run.tags.update(traced(L, lambda: bt_calls(L, case, y, x, gamma, scale, out, None, None, ws), "block_tail "))
    bt_calls(L, case, y, x, gamma, scale, out2, None, None, ws)
    if not S.same_bits(out, out2):
        bad.append("%s: out differs in the second call" % name)
    del out2
    gy, gy2 = nan(M, Cc, dtype=case.dtype), nan(M, Cc, dtype=case.dtype)
    gg, gg2 = nan(Cc), nan(Cc)
    run.tags.update(traced(L, lambda: bt_calls(L, case, y, x, gamma, scale, None, gy, gg, ws), "block_tail "))
    bt_calls(L, case, y, x, gamma, scale, None, gy2, gg2, ws)
    if not (S.same_bits(gy, gy2) and torch.equal(gg, gg2)):
        bad.append("%s: grad_y or grad_gamma differs in the second call" % name)
    del gy2, y, x
    scratch = None if case.exact else torch.empty(M, Cc, dtype=torch.float32, device=DEV)      # the products of the g_gamma yardstick
    bad += run.take(name, S.bt_check(case, {"out": out, "g_y": gy, "g_gamma": gg}, boundary, scratch=scratch))


@pytest.mark.parametrize("tag", sorted(S.BT_A))
def test_block_tail_past_2_31(L, tag):
    dt, nchw, shape = S.BT_A[tag]
    bad = []
    with Run("block_tail A " + tag, "B=%d C=%d H=%d W=%d y=%s" % (shape + (dt,)), S.elements(shape), S.bt_need(tag)) as run:
        try:
            bt_run(L, S.BtCase(dt, nchw, shape), S.B31, bad, run, "values")
            torch.cuda.empty_cache()
            bt_run(L, S.BtCase(dt, nchw, shape, exact=True), S.B31, bad, run, "integers")
            cls = P.bt_class("nchw" if nchw else "cl", dt, shape[1])
            want = {"block_tail fwd_%s gy=0 gg=0" % cls, "block_tail bwd_%s gy=1 gg=1" % cls, "block_tail reduce<f32>"}
            if set(run.tags) != want:
                bad.append("trace: %s, expected %s" % (sorted(run.tags), sorted(want)))
        finally:
            torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


# ================================================================================================================ lncf_train
@pytest.mark.parametrize("tag", sorted(S.LN_A))
def test_lncf_train_past_2_31(L, tag):
    dt, nchw, shape, cls = S.LN_A[tag]
    B, Cc, H, W = shape
    bad = []
    with Run("lncf_train A " + tag, "B=%d C=%d H=%d W=%d x=%s" % (shape + (dt,)), S.elements(shape), S.ln_need(tag)) as run:
        try:
            case = S.LnCase(dt, nchw, shape)
            lib, s, M, E = L.lib(), L.stream_ptr(), case.M, case.M * Cc
            need = lib.uni_lncf_train_workspace_bytes(B, H, W, Cc)
            assert need == 4 * 1024 * 2 * Cc
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            w, b = case.weight.to(DEV), case.bias.to(DEV)
            x = case.fill(case.x, torch.empty(E, dtype=case.dtype, device=DEV), nchw)

            def fwd(y_, st_):
                L.check(lib.uni_lncf_train_fwd(ptr(x), S.CODE[dt], nchw, ptr(w), ptr(b), S.RL.EPS, B, H, W, Cc, ptr(y_), ptr(st_), s), "uni_lncf_train_fwd")
                torch.cuda.synchronize()

            def bwd(gx_, gw_, gb_):
                L.check(lib.uni_lncf_train_bwd(ptr(x), S.CODE[dt], nchw, ptr(w), ptr(st), ptr(g), B, H, W, Cc, ptr(gx_), ptr(gw_), ptr(gb_), ptr(ws), need, s),
                        "uni_lncf_train_bwd")
                torch.cuda.synchronize()

            y, y2, st, st2 = nan(E), nan(E), nan(M, 2), nan(M, 2)
            run.tags.update(traced(L, lambda: fwd(y, st), "lncf_train "))
            fwd(y2, st2)
            if not (S.same_bits(y, y2) and S.same_bits(st, st2)):
                bad.append("y or stats differs in the second call")
            del st2
            g = case.fill(case.gy, y2, nchw)                                      # the second y becomes grad_y
            gx, gx2 = nan(E, dtype=case.dtype), nan(E, dtype=case.dtype)
            gw, gb, gw2, gb2 = nan(Cc), nan(Cc), nan(Cc), nan(Cc)
            run.tags.update(traced(L, lambda: bwd(gx, gw, gb), "lncf_train "))
            bwd(gx2, gw2, gb2)
            if not (S.same_bits(gx, gx2) and torch.equal(gw, gw2) and torch.equal(gb, gb2)):
                bad.append("a gradient differs in the second call")
            del gx2
            x = None                                                               # the check draws x again, chunk by chunk
            torch.cuda.empty_cache()
            scratch = torch.empty(E, dtype=torch.float32, device=DEV)
            bad += run.take("values", S.ln_check(case, {"y": y, "stats": st, "g_x": gx, "g_weight": gw, "g_bias": gb}, S.B31, scratch=scratch, gy=g))
            want = {"lncf_train fwd_%s gx=0 gwb=0" % cls, "lncf_train bwd_%s gx=1 gwb=1" % cls, "lncf_train reduce<f32>"}
            if set(run.tags) != want or P.predicted("lncf", "nchw" if nchw else "cl", dt, Cc) != cls:
                bad.append("trace: %s, expected %s" % (sorted(run.tags), sorted(want)))
        finally:
            x = y = y2 = g = gx = gx2 = st = scratch = None
            torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


# ================================================================================================================ dwln_train
def test_dwln_train_past_2_31(L):
    shape = S.DW_A
    B, Cc, H, W = shape
    M, E = B * H * W, S.elements(shape)
    bad = []
    with Run("dwln_train A", "B=%d C=%d H=%d W=%d f32" % shape, E, S.dw_need()) as run:
        try:
            case = S.DwCase(shape)
            lib, s = L.lib(), L.stream_ptr()
            need = lib.uni_dwln_train_workspace_bytes(B, H, W, Cc)
            assert need == S.dw_workspace(shape)
            wt, bias, gam, bet = (t.to(DEV) for t in (case.w49(), case.bias, case.ln_weight, case.ln_bias))
            x = case.fill(case.x, torch.empty(E, dtype=torch.float32, device=DEV))

            def fwd(y_, st_):
                L.check(lib.uni_dwln_train_fwd(ptr(x), ptr(wt), ptr(bias), ptr(gam), ptr(bet), S.RD.EPS, B, H, W, Cc, ptr(y_), ptr(st_), s), "uni_dwln_train_fwd")
                torch.cuda.synchronize()

            def bwd(gx_, gw_, gb_, gg_, gbe_):
                L.check(lib.uni_dwln_train_bwd(ptr(x), ptr(wt), ptr(bias), ptr(gam), ptr(st), ptr(g), B, H, W, Cc, ptr(gx_), ptr(gw_), ptr(gb_), ptr(gg_),
                                               ptr(gbe_), ptr(ws), need, s), "uni_dwln_train_bwd")
                torch.cuda.synchronize()

            y, y2, st, st2 = nan(E), nan(E), nan(M, 2), nan(M, 2)
            run.tags.update(traced(L, lambda: fwd(y, st), "dwln_train "))
            fwd(y2, st2)
            if not (S.same_bits(y, y2) and S.same_bits(st, st2)):
                bad.append("y or stats differs in the second call")
            del st2
            bad += run.take("forward", S.dw_band_check(case, x, None, {"y": y, "stats": st}))
            del y
            g = case.fill(case.gy, y2)                                            # the second y becomes grad_y
            ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            # grad_x alone
            gx = nan(E)
            run.tags.update(traced(L, lambda: bwd(gx, None, None, None, None), "dwln_train "))
            first = S.digest(gx)
            bad += run.take("grad_x", S.dw_band_check(case, x, g, {"grad_x": gx}))
            gx.fill_(float("nan"))
            bwd(gx, None, None, None, None)
            if S.digest(gx) != first:
                bad.append("grad_x differs in the second call")
            del gx
            # the two parameter pairs alone
            outs = [nan(49, Cc), nan(Cc), nan(Cc), nan(Cc)]
            again = [nan(49, Cc), nan(Cc), nan(Cc), nan(Cc)]
            run.tags.update(traced(L, lambda: bwd(None, *outs), "dwln_train "))
            bwd(None, *again)
            if not all(torch.equal(a, b) for a, b in zip(outs, again)):
                bad.append("a parameter gradient differs in the second call")
            del ws
            st = None
            torch.cuda.empty_cache()
            bad += run.take("parameters", S.dw_param_check(case, x, g, dict(zip(("grad_weight", "grad_bias", "grad_ln_weight", "grad_ln_bias"), outs))))
            want = {"dwln_train fwd" + S.DW_CLASS, "dwln_train bwd_a%s du=1 gb=0" % S.DW_CLASS, "dwln_train bwd_a%s du=1 gb=1" % S.DW_CLASS,
                    "dwln_train bwd_dx" + S.DW_CLASS, "dwln_train bwd_dw<f32> slen=128", "dwln_train reduce<f32> dw=1 gb=1"}
            if set(run.tags) != want:
                bad.append("trace: %s, expected %s" % (sorted(run.tags), sorted(want)))
        finally:
            x = y = y2 = g = gx = ws = st = None
            torch.cuda.empty_cache()
    assert not bad, "\n".join(bad)


# ================================================================================================================ every family, behind 2^31
def test_every_kernel_family_ran_behind_2_31(L):
    """from the records of the cases above (they run first: pytest keeps the order of the file): every family has a case of at least
    2^31 + 2^24 elements whose trace names it"""
    tags = {t for r in _RECORDS.values() if r["elements"] >= S.B31 + S.BEHIND for t in r["tags"]}
    families = ("pw_mlp act_fwd<f32,V=4>", "pw_mlp act_bwd<f32,V=4>", "pw_mlp colsum<f32,V=4>", "pw_mlp act_fwd<f16,V=8>", "pw_mlp act_bwd<f16,V=8>",
                "block_tail fwd_cl<", "block_tail bwd_cl<", "block_tail fwd_nchw<", "block_tail bwd_nchw<",
                "lncf_train fwd_cl<", "lncf_train bwd_cl<", "lncf_train fwd_nchw<f16,regs=16>", "lncf_train bwd_nchw<f16,regs=16>",
                "lncf_train fwd_nchw<f16,regs=32>", "lncf_train bwd_nchw<f16,regs=32>", "lncf_train fwd_nchw<f16,stream=8>",
                "lncf_train bwd_nchw<f16,stream=8>", "dwln_train fwd<", "dwln_train bwd_a<", "dwln_train bwd_dx<", "dwln_train bwd_dw<")
    missing = [f for f in families if not any(t.startswith(f) for t in tags)]
    assert not missing, "no case of 2^31 + 2^24 elements ran: %s (ran: %s)" % (missing, sorted(tags))
