"""Guard-band runs of uni_pw_mlp_act_fwd / _bwd (fp32, fp64, fp16 and bf16 maps), the method of tests/test_lncf_train_bounds_gpu.py: every
buffer is a tests/guard.py allocation [front guard | payload | back guard].  h, grad_a and grad_y are NaN-poisoned beyond their last element,
so a read outside a map reaches an output; a, grad_h, grad_b1 and grad_b2 are filled with 0xA5 and must come back completely written; the
workspace is exactly what uni_pw_mlp_workspace_bytes returns (twice that for fp64) = 4 * 256 * (Hd + Co).  Guards must come back untouched and
every output BIT-EQUAL to the plain call on exact-size tensors.  Shapes: the fixtures `c24` (42 rows, a multiple of no rows-per-block value),
`h100` (Hd no multiple of 8: 25 vectors on 32 lanes) and `c48`, a single row of 768 hidden units, and three shapes whose last column tile has
idle vector slots that sit on the LAST row, where a lane that ignores `vok` leaves the buffer: 37 x 68 with Co = 164 and 37 x 136 with Co = 328
(three tiles of L = 8, seven slots idle, with four and with eight columns per lane; the column sums the same at L = 16) and 262 x 2020 with
Co = 68 (two tiles of L = 256, seven idle, one row per group and 262 groups on 256 rows of partials: the blocks loop).  Each partial call (a alone, grad_h
alone, the sums alone) leaves the others' buffers and a given workspace untouched."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import pw_mlp_ref as R  # noqa: E402

DEV = "cuda"
H_DTYPE = {torch.float32: 0, torch.float64: 0, torch.float16: 1, torch.bfloat16: 2}
ROWS = 256
RAGGED = {"m37n68": (37, 68, 164), "m37n136": (37, 136, 328), "m262n2020": (262, 2020, 68)}      # M, Hd, Co


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_pw_mlp_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def maps(tag):
    """-> h, grad_a (M, Hd), grad_y (M, Co) in fp64 on the CPU"""
    if tag == "row":
        g = torch.Generator().manual_seed(9)
        return torch.randn(1, 768, generator=g).double(), torch.randn(1, 768, generator=g).double(), torch.randn(1, 192, generator=g).double()
    if tag in RAGGED:
        return tuple(t.double() for t in R.draw_maps(*RAGGED[tag]))
    ins = [torch.from_numpy(R.load_case(tag)[n]) for n in R.INPUTS]
    full = R.value_and_grads(*ins, dtype=torch.float64)
    Hd, Co = full["h"].shape[-1], ins[5].shape[-1]
    return full["h"].reshape(-1, Hd), full["grad_a"].reshape(-1, Hd), ins[5].double().reshape(-1, Co)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.float16, torch.bfloat16], ids=["fp32", "fp64", "fp16", "bf16"])
@pytest.mark.parametrize("tag", ["c24", "h100", "c48", "row"] + sorted(RAGGED))
def test_pw_mlp_stays_inside_its_buffers(L, tag, dtype):
    h, ga, gy = (t.to(DEV, dtype) for t in maps(tag))
    (M, Hd), Co = h.shape, gy.shape[1]
    f64 = dtype == torch.float64
    sfx = "_f64" if f64 else ""
    sdt = torch.float64 if f64 else torch.float32
    hd = H_DTYPE[dtype]
    lib = L.lib()
    fwd, bwd = getattr(lib, "uni_pw_mlp_act_fwd" + sfx), getattr(lib, "uni_pw_mlp_act_bwd" + sfx)
    need = lib.uni_pw_mlp_workspace_bytes(M, Hd, Co) * (2 if f64 else 1)
    assert need == 4 * ROWS * (Hd + Co) * (2 if f64 else 1)
    s = L.stream_ptr()

    def run(h_, ga_, gy_, af_, a_, gh_, gb1_, gb2_, ws_, nws=need):
        if af_ is not None:
            L.check(fwd(P(h_), hd, M, Hd, P(af_), s), "uni_pw_mlp_act_fwd" + sfx)
        L.check(bwd(P(h_), hd, P(ga_), M, Hd, P(a_), P(gh_), P(gb1_), P(gy_), Co, P(gb2_), P(ws_), nws, s), "uni_pw_mlp_act_bwd" + sfx)
        torch.cuda.synchronize()

    e = lambda dt, *shape: torch.empty(*shape, device=DEV, dtype=dt)       # noqa: E731
    plain = dict(a_fwd=e(dtype, M, Hd), a=e(dtype, M, Hd), grad_h=e(dtype, M, Hd), g_b1=e(sdt, Hd), g_b2=e(sdt, Co))
    run(h, ga, gy, *plain.values(), torch.empty(need, dtype=torch.uint8, device=DEV))
    assert torch.equal(plain["a_fwd"], plain["a"])

    gb_ = lambda t: G.guard_bytes(t.shape[-1], t.element_size())   # noqa: E731

    def outs():
        return [G.guard_out(n, t.reshape(-1, t.shape[-1]).shape[0], t.shape[-1], t.dtype, DEV, guard=gb_(t)) for n, t in plain.items()]

    gi = [G.guard_in(n, t, guard=gb_(t)) for n, t in (("h", h), ("grad_a", ga), ("grad_y", gy))]
    go = outs()
    gw = G.guard_ws("workspace", need, DEV)
    run(*gi, *go, gw)
    G.check_all(*(gi + go + [gw]))
    for gd, t in zip(go, plain.values()):
        gd.check_equal(t)
    G.record("uni_pw_mlp_act_fwd/_bwd" + sfx, "h_dtype=%s" % dtype, "M=%d Hd=%d Co=%d" % (M, Hd, Co), {}, gi + go + [gw], workspace_bytes=need)

    # each partial call: its own output has the bits of the full call, the others' buffers and a given workspace stay as they were
    for name, pick in (("a alone", (1,)), ("grad_h alone", (2,)), ("sums alone", (3, 4)), ("grad_b1 alone", (3,)), ("grad_b2 alone", (4,))):
        go = outs()
        gw = G.guard_ws("workspace (%s)" % name, need, DEV)
        snaps = [b.base.clone() for b in go + [gw]]
        args = [go[i] if i in pick else None for i in range(5)]
        sums = 3 in pick or 4 in pick
        run(gi[0], gi[1] if pick != (1,) else None, gi[2] if 4 in pick else None, *args, gw)
        G.check_all(*gi)
        for i, (b, snap) in enumerate(zip(go + [gw], snaps)):
            if i in pick:
                b.check().check_equal(list(plain.values())[i], what="the full call (%s)" % name)
            elif i == 5 and sums:
                b.check()                             # the workspace is scratch here; its guards are not
            else:
                assert torch.equal(b.base, snap), (name, b.name)
        if not sums:                                  # the workspace may be NULL then
            lone = outs()[pick[0]]
            args = [lone if i in pick else None for i in range(5)]
            run(gi[0], gi[1], None, *args, None, 0)
            lone.check()
            lone.check_equal(list(plain.values())[pick[0]])

    # the in-place forms: a over h, grad_h over grad_a, guarded
    hi = G.guard_out("h -> a in place", M, Hd, dtype, DEV, guard=gb_(h), init=h)
    L.check(fwd(P(hi), hd, M, Hd, P(hi), s), "uni_pw_mlp_act_fwd" + sfx)
    hb = G.guard_out("h -> a in place (bwd)", M, Hd, dtype, DEV, guard=gb_(h), init=h)
    gbuf = G.guard_out("grad_a -> grad_h in place", M, Hd, dtype, DEV, guard=gb_(h), init=ga)
    b1 = G.guard_out("grad_b1 (in place)", 1, Hd, sdt, DEV, guard=gb_(plain["g_b1"]))
    gw = G.guard_ws("workspace (in place)", need, DEV)
    L.check(bwd(P(hb), hd, P(gbuf), M, Hd, P(hb), P(gbuf), P(b1), None, Co, None, P(gw), need, s), "uni_pw_mlp_act_bwd" + sfx)
    torch.cuda.synchronize()
    for b in (hi, hb, gbuf, b1, gw):
        b.check(complete=False)
    hi.check_equal(plain["a"]), hb.check_equal(plain["a"]), gbuf.check_equal(plain["grad_h"]), b1.check_equal(plain["g_b1"])


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(1 << 16, device=DEV)
    s = L.stream_ptr()
    wsb = lib.uni_pw_mlp_workspace_bytes
    ok = dict(M=4, Hd=8, Co=8, hd=0)

    def both(a, what, sfx=""):
        rc = getattr(lib, "uni_pw_mlp_act_bwd" + sfx)(P(x), a["hd"], P(x), a["M"], a["Hd"], P(x), P(x), P(x), P(x), a["Co"], P(x), P(x), 1 << 18, s)
        assert rc != 0 and what in lib.uni_last_error().decode(), (a, rc, lib.uni_last_error())
        if a["Co"] == ok["Co"]:
            rc = getattr(lib, "uni_pw_mlp_act_fwd" + sfx)(P(x), a["hd"], a["M"], a["Hd"], P(x), s)
            assert rc != 0 and what in lib.uni_last_error().decode(), (a, rc, lib.uni_last_error())

    for change, what in (({"Hd": 6}, "outside"), ({"Hd": 8196}, "outside"), ({"Hd": 0}, "outside"), ({"M": 0}, "outside"), ({"M": -1}, "outside"),
                         ({"Co": 6}, "outside"), ({"Co": 8196}, "outside"), ({"Co": 0}, "outside"), ({"hd": 3}, "h_dtype"), ({"hd": -1}, "h_dtype")):
        a = dict(ok, **change)
        both(a, what)
        if what == "outside":
            assert wsb(a["M"], a["Hd"], a["Co"]) == 0, a
    both(dict(ok, hd=1), "h_dtype", "_f64")
    both(dict(ok, hd=2), "h_dtype", "_f64")
    assert wsb(4, 8, 8) == 4 * ROWS * 16 and wsb((1 << 31) - 1, 8192, 8192) == 4 * ROWS * 16384 and wsb(1, 4, 4) == 4 * ROWS * 8
    bwd = lib.uni_pw_mlp_act_bwd
    rc = bwd(P(x), 0, P(x), 4, 8, P(x), P(x), P(x), P(x), 8, P(x), P(x), 16, s)                              # short
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = bwd(P(x), 0, P(x), 4, 8, P(x), P(x), P(x), P(x), 8, P(x), None, 1 << 20, s)                         # NULL
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = bwd(P(x), 0, P(x), 4, 8, None, None, None, P(x), 8, P(x), None, 0, s)                               # NULL with grad_b2 alone
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_pw_mlp_act_bwd_f64(P(x), 0, P(x), 4, 8, P(x), P(x), P(x), P(x), 8, P(x), P(x), wsb(4, 8, 8), s)   # fp64 needs twice that
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_pw_mlp_act_fwd(None, 0, 4, 8, P(x), s)
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = lib.uni_pw_mlp_act_fwd(P(x), 0, 4, 8, None, s)
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = bwd(None, 0, P(x), 4, 8, P(x), None, None, None, 8, None, None, 0, s)                               # a without h
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = bwd(P(x), 0, None, 4, 8, None, P(x), None, None, 8, None, None, 0, s)                               # grad_h without grad_a
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = bwd(None, 0, None, 4, 8, None, None, None, None, 8, P(x), P(x), 1 << 18, s)                         # grad_b2 without grad_y
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    off = C.c_void_p(x.data_ptr() + 4)
    rc = lib.uni_pw_mlp_act_fwd(off, 0, 4, 8, P(x), s)
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    rc = lib.uni_pw_mlp_act_fwd(P(x), 0, 4, 8, off, s)
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    for k in (0, 2, 5, 6, 7, 8, 10, 11):                                                                     # every pointer of the backward
        args = [P(x), 0, P(x), 4, 8, P(x), P(x), P(x), P(x), 8, P(x), P(x), 1 << 18, s]
        args[k] = off
        rc = bwd(*args)
        assert rc != 0 and "aligned" in lib.uni_last_error().decode(), k
    # nothing asked for: no launch, no error
    assert bwd(P(x), 0, P(x), 4, 8, None, None, None, None, 8, None, None, 0, s) == 0
    assert bwd(None, 0, None, 4, 8, None, None, None, None, 8, None, None, 0, s) == 0
    torch.cuda.synchronize()
