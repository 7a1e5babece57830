"""Guard-band runs of uni_gn_act_train_fwd / _bwd (fp32 and fp64, both memory layouts, fp16 x), the method of
tests/test_lncf_train_bounds_gpu.py: every buffer is a tests/guard.py allocation [front guard | payload | back guard].  x, weight, bias,
stats and grad_y are NaN-poisoned beyond their last element, so a read outside a map reaches an output; y, stats, grad_x, grad_weight and
grad_bias are filled with 0xA5 and must come back completely written; the workspace is exactly what uni_gn_act_train_workspace_bytes returns
(twice that for fp64).  Guards must come back untouched and every output BIT-EQUAL to the plain call on exact-size tensors.  Shapes: the
fixtures `c96` (cpg = 6, 63 pixels per image, channel rows that are not 16-byte aligned), `c100` (C no multiple of 8 or 16), `hw130`, `c1536`
(the widest neck width on a map smaller than a unit) and `cpg1`, held to the fixture values as well, and a single pixel of 192 channels (the
forward keeps one plane of partial statistics in y there)."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import gn_act_ref as R  # noqa: E402
import guard as G  # noqa: E402

DEV = "cuda"
X_DTYPE = {torch.float32: 0, torch.float64: 0, torch.float16: 1, torch.bfloat16: 2}
ACT = {"none": 0, "relu": 1, "silu": 3}
PIXEL = ((1, 192, 1, 1), 16, "silu", 1e-3)


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_gn_act_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def guarded_runs(L, tag, dtype, nchw, x_dtype=None):
    """plain call, guarded call, the two partial backward calls; -> (shape, case parameters, fixture or None, inputs, plain outputs)"""
    if tag == "pixel":
        (shape, Gn, act, eps), c = PIXEL, None
        ins = R.draw("plain", 9, shape)
    else:
        (shape, Gn, act, eps), c = R.CASES[tag], R.load_case(tag)
        ins = [torch.from_numpy(c[n]) for n in R.INPUTS]
    B, Cc, H, W = shape
    M = B * H * W
    f64 = dtype == torch.float64
    sfx = "_f64" if f64 else ""
    x_dtype = x_dtype or dtype
    xd, a = X_DTYPE[x_dtype], ACT[act]
    lib = L.lib()
    fwd, bwd = getattr(lib, "uni_gn_act_train_fwd" + sfx), getattr(lib, "uni_gn_act_train_bwd" + sfx)
    need = lib.uni_gn_act_train_workspace_bytes(B, H, W, Cc, Gn) * (2 if f64 else 1)
    rpi = -(-H * W // 16)                         # units of 16 pixels at these sizes, a row of partials each
    assert need == 4 * ((B * rpi * 2 * Cc + 63) // 64 * 64 + B * Gn * 2) * (2 if f64 else 1)
    rows, cols = (B * Cc, H * W) if nchw else (M, Cc)

    def lay(t):                                   # (B, C, H, W) -> rows of the layout under test
        return t.reshape(rows, cols).contiguous() if nchw else t.permute(0, 2, 3, 1).reshape(rows, cols).contiguous()

    x = lay(ins[0]).to(DEV, x_dtype)
    g = lay(ins[3]).to(DEV, dtype)
    w, b = ins[1].to(DEV, dtype), ins[2].to(DEV, dtype)

    def run(x_, w_, b_, g_, y_, st_, gx_, gw_, gb_, ws_):
        L.check(fwd(P(x_), xd, nchw, P(w_), P(b_), eps, a, B, H, W, Cc, Gn, P(y_), P(st_), L.stream_ptr()), "uni_gn_act_train_fwd" + sfx)
        L.check(bwd(P(x_), xd, nchw, P(w_), P(b_), P(st_), P(g_), a, B, H, W, Cc, Gn, P(gx_), P(gw_), P(gb_), P(ws_), need, L.stream_ptr()),
                "uni_gn_act_train_bwd" + sfx)
        torch.cuda.synchronize()

    e = lambda dt, *s: torch.empty(*s, device=DEV, dtype=dt)       # noqa: E731
    plain = dict(y=e(dtype, rows, cols), stats=e(dtype, B * Gn, 2), g_x=e(x_dtype, rows, cols), g_weight=e(dtype, Cc), g_bias=e(dtype, Cc))
    run(x, w, b, g, *plain.values(), torch.empty(need, dtype=torch.uint8, device=DEV))

    gb_ = lambda t: G.guard_bytes(t.shape[-1], t.element_size())   # noqa: E731
    gi = [G.guard_in(n, t, guard=gb_(t)) for n, t in (("x", x), ("weight", w), ("bias", b), ("grad_y", g))]
    go = [G.guard_out(n, t.reshape(-1, t.shape[-1]).shape[0], t.shape[-1], t.dtype, DEV, guard=gb_(t)) for n, t in plain.items()]
    gw = G.guard_ws("workspace", need, DEV)
    run(*gi, *go, gw)
    G.check_all(*(gi + go + [gw]))
    for gd, t in zip(go, plain.values()):
        gd.check_equal(t)
    G.record("uni_gn_act_train_fwd/_bwd" + sfx, "nchw=%d x=%s act=%s G=%d" % (nchw, x_dtype, act, Gn), "B=%d C=%d H=%d W=%d" % (B, Cc, H, W), {},
             gi + go + [gw], workspace_bytes=need)
    # the statistics the backward reads: an input now, poisoned beyond its end
    st = G.guard_in("stats", plain["stats"], guard=gb_(plain["stats"]))
    # grad_x alone: grad_weight and grad_bias are not touched (NULL), grad_x has the same bits
    lone = G.guard_out("grad_x alone", rows, cols, x_dtype, DEV, guard=gb_(x))
    gw1 = G.guard_ws("workspace (grad_x alone)", need, DEV)
    L.check(bwd(P(gi[0]), xd, nchw, P(gi[1]), P(gi[2]), P(st), P(gi[3]), a, B, H, W, Cc, Gn, P(lone), None, None, P(gw1), need, L.stream_ptr()),
            "uni_gn_act_train_bwd" + sfx)
    # grad_weight + grad_bias alone: grad_x is not touched (NULL), the pair has the same bits
    lone_w = G.guard_out("grad_weight alone", 1, Cc, dtype, DEV, guard=gb_(w))
    lone_b = G.guard_out("grad_bias alone", 1, Cc, dtype, DEV, guard=gb_(w))
    gw2 = G.guard_ws("workspace (pair alone)", need, DEV)
    L.check(bwd(P(gi[0]), xd, nchw, P(gi[1]), P(gi[2]), P(st), P(gi[3]), a, B, H, W, Cc, Gn, None, P(lone_w), P(lone_b), P(gw2), need, L.stream_ptr()),
            "uni_gn_act_train_bwd" + sfx)
    torch.cuda.synchronize()
    G.check_all(lone, lone_w, lone_b, gw1, gw2, st, *gi)
    lone.check_equal(plain["g_x"])
    lone_w.check_equal(plain["g_weight"])
    lone_b.check_equal(plain["g_bias"])
    # nothing asked for: no launch, a given workspace stays as it was
    gw3 = G.guard_ws("workspace (nothing asked for)", need, DEV)
    snap = gw3.base.clone()
    L.check(bwd(P(gi[0]), xd, nchw, P(gi[1]), P(gi[2]), P(st), P(gi[3]), a, B, H, W, Cc, Gn, None, None, None, P(gw3), need, L.stream_ptr()),
            "uni_gn_act_train_bwd" + sfx)
    torch.cuda.synchronize()
    assert torch.equal(gw3.base, snap)
    return shape, (Gn, act, eps), c, ins, plain


def unlay(t, shape, nchw):
    B, Cc, H, W = shape
    return t.reshape(B, Cc, H, W) if nchw else t.reshape(B, H, W, Cc).permute(0, 3, 1, 2)


def results(plain, shape, nchw):
    return dict(y=unlay(plain["y"], shape, nchw), g_x=unlay(plain["g_x"], shape, nchw), g_weight=plain["g_weight"], g_bias=plain["g_bias"])


@pytest.mark.parametrize("nchw", [0, 1], ids=["cl", "nchw"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("tag", ["c96", "c100", "hw130", "c1536", "cpg1", "pixel"])
def test_gn_act_train_stays_inside_its_buffers(L, tag, dtype, nchw):
    shape, _, c, _, plain = guarded_runs(L, tag, dtype, nchw)
    if c is not None:                                 # the values: the fixture
        got = results(plain, shape, nchw)
        for k in got:
            err = R.rel_err(got[k], torch.from_numpy(c[k]))
            assert err <= (1e-12 if dtype == torch.float64 else 4 * float(c[k + "_fp32_ref_err"])), (k, err)


@pytest.mark.parametrize("nchw", [0, 1], ids=["cl", "nchw"])
@pytest.mark.parametrize("tag", ["c96", "c100", "hw130", "c1536", "cpg1", "pixel"])
def test_fp16_x_stays_inside_its_buffers(L, tag, nchw):
    """x and grad_x in fp16 (x_dtype 1): rows of 2 C bytes; widths with C % 8 == 0 take 8 channels per lane in the channels-last kernel, c100
    four.  Values: the restatement in fp64 on the rounded x, the fp32 bound of the fixture, one rounding of fp16 on grad_x."""
    shape, (Gn, act, eps), c, ins, plain = guarded_runs(L, tag, torch.float32, nchw, x_dtype=torch.float16)
    if c is None:
        return
    ins = list(ins)
    ins[0] = ins[0].half().float()
    ref = R.value_and_grads(*ins, Gn, act, eps, dtype=torch.float64)
    got = results(plain, shape, nchw)
    for k in got:
        err = R.rel_err(got[k], ref[k])
        assert err <= 4 * float(c[k + "_fp32_ref_err"]) + (2.0 ** -11 if k == "g_x" else 0.0), (k, err)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(1 << 16, device=DEV)
    ok = dict(B=1, H=4, W=4, C=8, G=2, xd=0, act=3)
    s = L.stream_ptr()
    for change, what in (({"C": 6}, "outside"), ({"C": 2052, "G": 4}, "outside"), ({"B": 0}, "outside"), ({"H": 0}, "outside"), ({"xd": 3}, "x_dtype"),
                         ({"B": 1 << 11, "H": 1 << 10, "W": 1 << 10}, "outside"), ({"G": 0}, "outside"), ({"G": 3}, "outside"), ({"G": 16}, "outside"),
                         ({"act": 2}, "act"), ({"act": -1}, "act")):
        a = dict(ok, **change)
        for nchw in (0, 1):
            rc = lib.uni_gn_act_train_fwd(P(x), a["xd"], nchw, P(x), P(x), 1e-5, a["act"], a["B"], a["H"], a["W"], a["C"], a["G"], P(x), P(x), s)
            assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
            rc = lib.uni_gn_act_train_bwd(P(x), a["xd"], nchw, P(x), P(x), P(x), P(x), a["act"], a["B"], a["H"], a["W"], a["C"], a["G"], P(x), P(x), P(x),
                                          P(x), 1 << 18, s)
            assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    rc = lib.uni_gn_act_train_fwd_f64(P(x), 1, 0, P(x), P(x), 1e-5, 3, 1, 4, 4, 8, 2, P(x), P(x), s)
    assert rc != 0 and "x_dtype" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd_f64(P(x), 1, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), P(x), P(x), P(x), 1 << 18, s)
    assert rc != 0 and "x_dtype" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_fwd(P(x), 0, 0, P(x), P(x), 0.0, 3, 1, 4, 4, 8, 2, P(x), P(x), s)
    assert rc != 0 and "eps" in lib.uni_last_error().decode()
    wsb = lib.uni_gn_act_train_workspace_bytes
    rc = lib.uni_gn_act_train_bwd(P(x), 0, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), P(x), P(x), P(x), 16, s)          # short
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd(P(x), 0, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), P(x), P(x), None, 1 << 20, s)      # NULL
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd(P(x), 0, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), None, None, None, 0, s)            # grad_x alone needs it too
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd_f64(P(x), 0, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), P(x), P(x), P(x), wsb(1, 4, 4, 8, 2), s)   # fp64: twice that
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd(P(x), 0, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), P(x), None, P(x), 1 << 18, s)      # half a pair
    assert rc != 0 and "pair" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_fwd(None, 0, 0, P(x), P(x), 1e-5, 3, 1, 4, 4, 8, 2, P(x), P(x), s)
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd(P(x), 0, 0, P(x), None, P(x), P(x), 3, 1, 4, 4, 8, 2, P(x), P(x), P(x), P(x), 1 << 18, s)
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    off = C.c_void_p(x.data_ptr() + 4)
    rc = lib.uni_gn_act_train_fwd(off, 0, 0, P(x), P(x), 1e-5, 3, 1, 4, 4, 8, 2, P(x), P(x), s)
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_fwd(P(x), 0, 1, P(x), P(x), 1e-5, 3, 1, 4, 4, 8, 2, off, P(x), s)
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    rc = lib.uni_gn_act_train_bwd(P(x), 0, 0, P(x), P(x), P(x), P(x), 3, 1, 4, 4, 8, 2, off, P(x), P(x), P(x), 1 << 18, s)
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
