"""Guard-band runs of uni_dwln_train_fwd / _bwd (fp32 and fp64), the method of tests/test_mot_corr_bounds_gpu.py: every buffer is a
tests/guard.py allocation [front guard | payload | back guard].  x and grad_y are NaN-poisoned around rows that end after their last pixel,
so a halo read outside the map, or into the neighbouring image's guard, reaches an output; the parameters likewise; y, the statistics and
the five gradients are filled with 0xA5 and must come back completely written; the workspace is exactly what
uni_dwln_train_workspace_bytes returns (twice that for fp64).  Guards must come back untouched and every output BIT-EQUAL to the plain call on
exact-size tensors.  Shapes: the fixtures `c96` (two images: a halo across the image boundary) and `c100` (C no multiple of 64, three
images), held to the fixture values as well, and a single pixel of 192 channels."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import dwln_train_ref as R  # noqa: E402
import guard as G  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_dwln_train_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tag", ["c96", "c100", "pixel"])
def test_dwln_train_stays_inside_its_buffers(L, tag, dtype):
    if tag == "pixel":
        shape, c = (1, 192, 1, 1), None
        ins = R.draw("plain", 9, shape)
    else:
        shape, c = R.CASES[tag], R.load_case(tag)
        ins = [torch.from_numpy(c[n]) for n in R.INPUTS]
    B, Cc, H, W = shape
    M = B * H * W
    f64 = dtype == torch.float64
    sfx = "_f64" if f64 else ""
    lib = L.lib()
    fwd, bwd = getattr(lib, "uni_dwln_train_fwd" + sfx), getattr(lib, "uni_dwln_train_bwd" + sfx)
    need = lib.uni_dwln_train_workspace_bytes(B, H, W, Cc) * (2 if f64 else 1)
    assert need > 0
    x = ins[0].permute(0, 2, 3, 1).reshape(M, Cc).contiguous().to(DEV, dtype)
    wt = ins[1].reshape(Cc, 49).t().contiguous().to(DEV, dtype)
    bias, gamma, beta = (t.to(DEV, dtype) for t in ins[2:5])
    gy = ins[5].reshape(M, Cc).contiguous().to(DEV, dtype)
    es = x.element_size()

    def run(x_, wt_, bias_, gamma_, beta_, gy_, y_, st_, gx_, gw_, gb_, gg_, gbe_, ws_):
        L.check(fwd(P(x_), P(wt_), P(bias_), P(gamma_), P(beta_), R.EPS, B, H, W, Cc, P(y_), P(st_), L.stream_ptr()), "uni_dwln_train_fwd" + sfx)
        L.check(bwd(P(x_), P(wt_), P(bias_), P(gamma_), P(st_), P(gy_), B, H, W, Cc, P(gx_), P(gw_), P(gb_), P(gg_), P(gbe_), P(ws_), need,
                    L.stream_ptr()), "uni_dwln_train_bwd" + sfx)
        torch.cuda.synchronize()

    e = lambda *s: torch.empty(*s, device=DEV, dtype=dtype)       # noqa: E731
    plain = dict(y=e(M, Cc), stats=e(M, 2), gx=e(M, Cc), gw=e(49, Cc), gb=e(Cc), ggamma=e(Cc), gbeta=e(Cc))
    run(x, wt, bias, gamma, beta, gy, *plain.values(), torch.empty(need, dtype=torch.uint8, device=DEV))

    gi = [G.guard_in(n, t, guard=G.guard_bytes(t.shape[-1], es)) for n, t in (("x", x), ("weight", wt), ("bias", bias), ("ln_weight", gamma),
                                                                               ("ln_bias", beta), ("grad_y", gy))]
    go = [G.guard_out(n, t.reshape(-1, t.shape[-1]).shape[0], t.shape[-1], dtype, DEV, guard=G.guard_bytes(t.shape[-1], es)) for n, t in plain.items()]
    gw = G.guard_ws("workspace", need, DEV)
    run(*gi, *go, gw)
    G.check_all(*(gi + go + [gw]))
    for g, t in zip(go, plain.values()):
        g.check_equal(t)
    G.record("uni_dwln_train_fwd/_bwd" + sfx, "exact-size rows", "B=%d C=%d H=%d W=%d" % (B, Cc, H, W), {}, gi + go + [gw], workspace_bytes=need)
    # grad_x alone: the other gradient buffers are not touched at all, grad_x has the same bits
    lone = G.guard_out("grad_x alone", M, Cc, dtype, DEV, guard=G.guard_bytes(Cc, es))
    L.check(bwd(P(gi[0]), P(gi[1]), P(gi[2]), P(gi[3]), P(go[1]), P(gi[5]), B, H, W, Cc, P(lone), None, None, None, None, P(gw), need, L.stream_ptr()),
            "uni_dwln_train_bwd" + sfx)
    torch.cuda.synchronize()
    G.check_all(lone, gw, *gi)
    lone.check_equal(plain["gx"])
    if c is not None:                                 # the values: the fixture
        got = dict(plain, gx=plain["gx"].reshape(B, H, W, Cc).permute(0, 3, 1, 2), gw=plain["gw"].t().reshape(Cc, 1, 7, 7))
        for k in R.RESULTS:
            err = R.rel_err(got[k].reshape(c[k].shape), torch.from_numpy(c[k]))
            assert err <= (1e-12 if f64 else 4 * float(c[k + "_fp32_ref_err"])), (k, err)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(1 << 16, device=DEV)
    ok = dict(B=1, H=4, W=4, C=8, ws=1 << 20, eps=1e-6)
    for change, what in (({"C": 6}, "outside"), ({"C": 2052}, "outside"), ({"B": 0}, "outside"), ({"H": 0}, "outside"), ({"eps": 0.0}, "eps")):
        a = dict(ok, **change)
        rc = lib.uni_dwln_train_fwd(P(x), P(x), P(x), P(x), P(x), a["eps"], a["B"], a["H"], a["W"], a["C"], P(x), P(x), L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    assert lib.uni_dwln_train_workspace_bytes(1, 4, 4, 6) == 0 and lib.uni_dwln_train_workspace_bytes(1, 4, 4, 8) > 0
    rc = lib.uni_dwln_train_bwd(P(x), P(x), P(x), P(x), P(x), P(x), 1, 4, 4, 8, P(x), P(x), P(x), P(x), P(x), P(x), 16, L.stream_ptr())
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_dwln_train_bwd(P(x), P(x), P(x), P(x), P(x), P(x), 1, 4, 4, 8, P(x), P(x), None, P(x), P(x), P(x), 1 << 20, L.stream_ptr())
    assert rc != 0 and "pairs" in lib.uni_last_error().decode()
    rc = lib.uni_dwln_train_fwd(None, P(x), P(x), P(x), P(x), 1e-6, 1, 4, 4, 8, P(x), P(x), L.stream_ptr())
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
