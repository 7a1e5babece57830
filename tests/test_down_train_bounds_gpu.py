"""Guard-band runs of uni_down_train_fwd / _bwd and uni_patch4_gather / _scatter (fp32 and fp64, half x with a half patch matrix), the method
of tests/test_lncf_train_bounds_gpu.py: every buffer is a tests/guard.py allocation [front guard | payload | back guard].  Inputs are
NaN-poisoned beyond their last element, so a read outside a map reaches an output; outputs are filled with 0xA5 and must come back
completely written; the workspace is exactly what uni_down_train_workspace_bytes returns (twice that for fp64).  Guards must come back
untouched and every output BIT-EQUAL to the plain call on exact-size tensors.  Shapes: the fixtures `odd` (a dropped row and column), `c96` (a
pixel group that straddles two images), `c100` (C no multiple of 8), `c768` (a map smaller than a group), a single 2 x 2 map of 192 channels,
and `stem_crop` (margins of 1 and 2) for the stem patches."""
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import down_calls as K  # noqa: E402
import down_train_ref as R  # noqa: E402
import guard as G  # noqa: E402

DEV = "cuda"
FORMS = [(torch.float32, torch.float32, torch.float32), (torch.float64, torch.float64, torch.float64), (torch.float32, torch.float16, torch.float16),
         (torch.float32, torch.bfloat16, torch.bfloat16)]
FORM_IDS = ["fp32", "fp64", "fp16", "bf16"]


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_down_train_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def gb_(t):
    return G.guard_bytes(t.shape[-1], t.element_size())


@pytest.mark.parametrize("dtype,x_dtype,a_dtype", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("tag", ["odd", "c96", "c100", "c768", "map2x2"])
def test_down_train_stays_inside_its_buffers(L, tag, dtype, x_dtype, a_dtype):
    if tag == "map2x2":
        shape = (1, 192, 2, 2)
        ins = R.draw("plain", 9, shape, 4)
    else:
        shape = R.CASES[tag][0]
        c = R.load_case(tag)
        ins = [torch.from_numpy(c[n]) for n in R.INPUTS]
    N, Cc, H, W = shape
    f64 = dtype == torch.float64
    dims = (N, H, W, Cc)
    M, px = N * (H // 2) * (W // 2), N * H * W
    xd, ad = K.DT[x_dtype], K.DT[a_dtype]
    need = K.ws_bytes(L, f64, dims)
    assert need == 4 * 1024 * 2 * Cc * (2 if f64 else 1)
    x = K.cl_rows(ins[0]).to(DEV, x_dtype)
    w, b = ins[1].to(DEV, dtype), ins[2].to(DEV, dtype)
    gA = torch.randn(M, 4 * Cc, generator=torch.Generator().manual_seed(3)).to(DEV, a_dtype)

    def run(x_, w_, b_, g_, A_, A2_, st_, gx_, gw_, gb2_, ws_):
        K.down_fwd(L, f64, x_, xd, w_, b_, dims, 0, A_, ad, st_)
        K.down_fwd(L, f64, x_, xd, w_, b_, dims, 1, A2_, ad, st_)
        K.down_bwd(L, f64, x_, xd, w_, st_, g_, ad, dims, gx_, gw_, gb2_, ws_, need)
        torch.cuda.synchronize()

    e = lambda dt, *s: torch.empty(*s, device=DEV, dtype=dt)       # noqa: E731
    plain = dict(A=e(a_dtype, M, 4 * Cc), A2=e(a_dtype, M, 4 * Cc), stats=e(dtype, px, 2), g_x=e(x_dtype, px, Cc), g_ln_weight=e(dtype, Cc),
                 g_ln_bias=e(dtype, Cc))
    run(x, w, b, gA, *plain.values(), torch.empty(need, dtype=torch.uint8, device=DEV))
    assert torch.equal(plain["A"].view(torch.uint8), plain["A2"].view(torch.uint8))
    gi = [G.guard_in(n, t, guard=gb_(t)) for n, t in (("x", x), ("ln_weight", w), ("ln_bias", b), ("grad_A", gA))]
    go = [G.guard_out(n, t.reshape(-1, t.shape[-1]).shape[0], t.shape[-1], t.dtype, DEV, guard=gb_(t)) for n, t in plain.items()]
    gw = G.guard_ws("workspace", need, DEV)
    run(*gi, *go, gw)
    G.check_all(*(gi + go + [gw]))
    for gd, t in zip(go, plain.values()):
        gd.check_equal(t)
    G.record("uni_down_train_fwd/_bwd" + K.sfx(f64), "x=%s a=%s" % (x_dtype, a_dtype), "B=%d C=%d H=%d W=%d" % (N, Cc, H, W), {}, gi + go + [gw],
             workspace_bytes=need)
    # the statistics the rebuild and the backward read: an input now, poisoned beyond its end
    st = G.guard_in("stats", plain["stats"], guard=gb_(plain["stats"]))
    re = G.guard_out("A rebuilt", M, 4 * Cc, a_dtype, DEV, guard=gb_(gA))
    K.down_fwd(L, f64, gi[0], xd, gi[1], gi[2], dims, 1, re, ad, st)
    # grad_x alone: the pair and the workspace are not touched (all NULL); the pair alone: grad_x is not touched
    lone = G.guard_out("grad_x alone", px, Cc, x_dtype, DEV, guard=gb_(x))
    K.down_bwd(L, f64, gi[0], xd, gi[1], st, gi[3], ad, dims, lone, None, None, None, 0)
    lone_w = G.guard_out("grad_ln_weight alone", 1, Cc, dtype, DEV, guard=gb_(w))
    lone_b = G.guard_out("grad_ln_bias alone", 1, Cc, dtype, DEV, guard=gb_(w))
    gw2 = G.guard_ws("workspace (pair alone)", need, DEV)
    K.down_bwd(L, f64, gi[0], xd, gi[1], st, gi[3], ad, dims, None, lone_w, lone_b, gw2, need)
    torch.cuda.synchronize()
    G.check_all(re, lone, lone_w, lone_b, gw2, st, *gi)
    re.check_equal(plain["A"])
    lone.check_equal(plain["g_x"])
    lone_w.check_equal(plain["g_ln_weight"])
    lone_b.check_equal(plain["g_ln_bias"])
    if tag != "map2x2":                               # the values: the patch restatement in fp64 on the same (rounded) inputs
        xs = K.from_cl_rows(x, shape)
        ref = R.patch_grads(xs.double(), w.double(), b.double(), gA.double())
        low = R.patch_grads(xs.float(), w.float(), b.float(), gA.float())
        got = dict(plain, g_x=K.from_cl_rows(plain["g_x"], shape))
        for k in ref:
            ulp = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}.get(a_dtype if k == "A" else x_dtype if k == "g_x" else None, 0.0)
            yard = float(c[{"A": "y", "stats": "y"}.get(k, k) + "_fp32_ref_err"])
            err = R.rel_err(got[k], ref[k])
            assert err <= (1e-12 if f64 else 4 * max(yard, R.rel_err(low[k], ref[k])) + ulp), (k, err)


@pytest.mark.parametrize("dtype,x_dtype,a_dtype", FORMS, ids=FORM_IDS)
def test_stem_patches_stay_inside_their_buffers(L, dtype, x_dtype, a_dtype):
    (N, Cin, H, W), _ = R.STEM_CASES["stem_crop"]
    f64 = dtype == torch.float64
    dims = (N, Cin, H, W)
    M = N * (H // 4) * (W // 4)
    xd, ad = K.DT[x_dtype], K.DT[a_dtype]
    x = torch.from_numpy(R.load_case("stem_crop")["x"]).to(DEV, x_dtype).reshape(N * Cin * H, W)
    gA = torch.randn(M, 16 * Cin, generator=torch.Generator().manual_seed(4)).to(DEV, a_dtype)
    A, gx = torch.empty_like(gA), torch.empty_like(x)
    K.gather(L, f64, x, xd, dims, A, ad)
    K.scatter(L, f64, gA, ad, dims, gx, xd)
    torch.cuda.synchronize()
    gi = [G.guard_in("x", x, guard=gb_(x)), G.guard_in("grad_A", gA, guard=gb_(gA))]
    go = [G.guard_out("A", M, 16 * Cin, a_dtype, DEV, guard=gb_(gA)), G.guard_out("grad_x", N * Cin * H, W, x_dtype, DEV, guard=gb_(x))]
    K.gather(L, f64, gi[0], xd, dims, go[0], ad)
    K.scatter(L, f64, gi[1], ad, dims, go[1], xd)
    torch.cuda.synchronize()
    G.check_all(*(gi + go))
    go[0].check_equal(A)
    go[1].check_equal(gx)
    G.record("uni_patch4_gather/_scatter" + K.sfx(f64), "x=%s a=%s" % (x_dtype, a_dtype), "B=%d Cin=%d H=%d W=%d" % dims, {}, gi + go)
    assert torch.equal(A, R.to_patches(x.reshape(N, Cin, H, W), 4).to(a_dtype))
    want = torch.zeros(N, Cin, H, W, device=DEV, dtype=x_dtype)
    g4 = gA.reshape(N, H // 4, W // 4, Cin, 4, 4).permute(0, 3, 1, 4, 2, 5).reshape(N, Cin, 8, 12)
    want[:, :, :8, :12] = g4.to(x_dtype)
    assert torch.equal(gx.reshape(N, Cin, H, W), want)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    P = K.P
    x = torch.zeros(1 << 16, device=DEV)
    s = L.stream_ptr()
    ok = dict(B=1, H=4, W=4, C=8, xd=0, ad=0)
    for change, what in (({"C": 6}, "outside"), ({"C": 2052}, "outside"), ({"B": 0}, "outside"), ({"H": 1}, "outside"), ({"W": 1}, "outside"),
                         ({"xd": 3}, "x_dtype"), ({"ad": 3}, "a_dtype"), ({"B": 1 << 11, "H": 1 << 10, "W": 1 << 10}, "outside")):
        a = dict(ok, **change)
        rc = lib.uni_down_train_fwd(P(x), a["xd"], P(x), P(x), 1e-6, a["B"], a["H"], a["W"], a["C"], 0, P(x), a["ad"], P(x), s)
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
        rc = lib.uni_down_train_bwd(P(x), a["xd"], P(x), P(x), P(x), a["ad"], a["B"], a["H"], a["W"], a["C"], P(x), P(x), P(x), P(x), 1 << 18, s)
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    for xd, ad, what in ((1, 0, "x_dtype"), (0, 2, "a_dtype")):
        rc = lib.uni_down_train_fwd_f64(P(x), xd, P(x), P(x), 1e-6, 1, 4, 4, 8, 0, P(x), ad, P(x), s)
        assert rc != 0 and what in lib.uni_last_error().decode()
        rc = lib.uni_patch4_gather_f64(P(x), xd, 1, 3, 8, 8, P(x), ad, s)
        assert rc != 0 and what in lib.uni_last_error().decode()
    rc = lib.uni_down_train_fwd(P(x), 0, P(x), P(x), 0.0, 1, 4, 4, 8, 0, P(x), 0, P(x), s)
    assert rc != 0 and "eps" in lib.uni_last_error().decode()
    wsb = lib.uni_down_train_workspace_bytes
    assert wsb(1, 4, 4, 8) == 4 * 1024 * 2 * 8 == lib.uni_lncf_train_workspace_bytes(1, 4, 4, 8)
    for bad in ((1, 4, 4, 6), (1, 4, 4, 2052), (0, 4, 4, 8), (1, 1, 4, 8), (1, 4, 1, 8), (1 << 11, 1 << 10, 1 << 10, 8)):
        assert wsb(*bad) == 0, bad
    rc = lib.uni_down_train_bwd(P(x), 0, P(x), P(x), P(x), 0, 1, 4, 4, 8, P(x), P(x), P(x), P(x), 16, s)             # short
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_down_train_bwd_f64(P(x), 0, P(x), P(x), P(x), 0, 1, 4, 4, 8, P(x), P(x), P(x), P(x), wsb(1, 4, 4, 8), s)    # fp64 needs twice that
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_down_train_bwd(P(x), 0, P(x), P(x), P(x), 0, 1, 4, 4, 8, P(x), P(x), None, P(x), 1 << 18, s)         # half a pair
    assert rc != 0 and "pair" in lib.uni_last_error().decode()
    rc = lib.uni_down_train_fwd(None, 0, P(x), P(x), 1e-6, 1, 4, 4, 8, 0, P(x), 0, P(x), s)
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    import ctypes
    off = ctypes.c_void_p(x.data_ptr() + 4)
    rc = lib.uni_down_train_fwd(P(x), 0, P(x), P(x), 1e-6, 1, 4, 4, 8, 0, off, 0, P(x), s)
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    for dims in ((1, 5, 8, 8), (1, 0, 8, 8), (1, 3, 3, 8), (1, 3, 8, 3), (0, 3, 8, 8)):
        rc = lib.uni_patch4_gather(P(x), 0, *dims, P(x), 0, s)
        assert rc != 0 and "outside" in lib.uni_last_error().decode(), dims
        rc = lib.uni_patch4_scatter(P(x), 0, *dims, P(x), 0, s)
        assert rc != 0 and "outside" in lib.uni_last_error().decode(), dims
    rc = lib.uni_patch4_gather(P(x), 0, 1, 3, 8, 8, None, 0, s)
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
