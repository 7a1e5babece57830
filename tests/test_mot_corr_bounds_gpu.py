"""Guard-band runs of uni_mot_corr_loss_fwd / _bwd (fp32 and fp64), the method of tests/test_simota_bounds_gpu.py: every buffer is a
tests/guard.py allocation [front guard | payload | back guard].  The embedding maps are rows with a padded pitch -- channels-last rows of
C + 5 elements, or NCHW rows of W + 3 -- handed over by their element strides, NaN-poisoned around the payload and in the padding; the
losses and the two dense gradient maps (same padded pitches) are filled with 0xA5; the workspace is exactly what
uni_mot_corr_workspace_bytes returns (twice that for fp64).  Guards and padding must come back untouched, the outputs completely written
and BIT-EQUAL to the plain call on contiguous, exact-size tensors.  Shapes: the `edge` fixture (24 channels, centres outside the map, two
instances in one cell) and the `crowd` fixture (100 x 97 instances: more than one wave, many shared pixels).  The values are held to the
fixtures as well."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import mot_corr_ref as R  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_mot_corr_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def ST(strides):
    return (C.c_int64 * 4)(*strides)


def rows_of(t, layout):
    """(B, C, H, W) -> the 2-D rows of the layout: channels-last (B H W, C) or NCHW (B C H, W)"""
    B, Cc, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, Cc) if layout == "nhwc" else t.reshape(B * Cc * H, W)


def strides_of(shape, layout, ld):
    B, Cc, H, W = shape
    return (H * W * ld, 1, W * ld, ld) if layout == "nhwc" else (Cc * H * ld, H * ld, ld, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("tag", ["edge", "crowd"])
def test_mot_corr_loss_stays_inside_its_buffers(L, tag, layout, dtype):
    c = R.load_case(tag)
    B, Cc, H, W, M, bidirect, grid_sample, _ = R.CASES[tag]
    f64 = dtype == torch.float64
    sfx = "_f64" if f64 else ""
    lib = L.lib()
    fwd, bwd = getattr(lib, "uni_mot_corr_loss_fwd" + sfx), getattr(lib, "uni_mot_corr_loss_bwd" + sfx)
    need = lib.uni_mot_corr_workspace_bytes(B, M, Cc) * (2 if f64 else 1)
    assert need > 0
    flags = (1 if bidirect else 0) | (2 if grid_sample else 0)
    e0, e1 = torch.from_numpy(c["embed_0"]).to(DEV, dtype), torch.from_numpy(c["embed_1"]).to(DEV, dtype)
    t, g = torch.from_numpy(c["targets"]).to(DEV), torch.from_numpy(c["grad_loss"]).to(DEV, dtype)
    shape = (B, Cc, H, W)

    def run(e0_, e1_, s_in, t_, g_, loss_, g0_, g1_, s_out, ws_):
        L.check(fwd(P(e0_), ST(s_in), P(e1_), ST(s_in), P(t_), B, Cc, H, W, M, float(R.S), flags, P(loss_), P(ws_), need, L.stream_ptr()),
                "uni_mot_corr_loss_fwd" + sfx)
        L.check(bwd(P(e0_), ST(s_in), P(e1_), ST(s_in), P(t_), P(g_), B, Cc, H, W, M, float(R.S), flags, P(g0_), ST(s_out), P(g1_), ST(s_out),
                    P(ws_), need, L.stream_ptr()), "uni_mot_corr_loss_bwd" + sfx)
        torch.cuda.synchronize()

    # plain call: contiguous NCHW tensors of the exact size
    loss, g0, g1 = torch.empty(B, device=DEV, dtype=dtype), torch.empty_like(e0), torch.empty_like(e1)
    run(e0, e1, e0.stride(), t, g, loss, g0, g1, g0.stride(), torch.empty(need, dtype=torch.uint8, device=DEV))

    cols = Cc if layout == "nhwc" else W
    ld = cols + (5 if layout == "nhwc" else 3)
    es = e0.element_size()
    gi = [G.guard_in(n, rows_of(x, layout), ld=ld, guard=G.guard_bytes(ld, es)) for n, x in (("embed_0", e0), ("embed_1", e1))]
    gi += [G.guard_in("targets", t.reshape(B * 2 * M, 6), guard=G.guard_bytes(6, 4)), G.guard_in("grad_loss", g, guard=G.guard_bytes(B, es))]
    go = [G.guard_out("loss", 1, B, dtype, DEV, guard=G.guard_bytes(B, es))]
    go += [G.guard_out(n, gi[0].rows, cols, dtype, DEV, ld=ld, guard=G.guard_bytes(ld, es)) for n in ("grad_embed_0", "grad_embed_1")]
    gw = G.guard_ws("workspace", need, DEV)
    st = strides_of(shape, layout, ld)
    run(gi[0], gi[1], st, gi[2], gi[3], go[0], go[1], go[2], st, gw)
    G.check_all(*(gi + go + [gw]))
    go[0].check_equal(loss)
    go[1].check_equal(rows_of(g0, layout))
    go[2].check_equal(rows_of(g1, layout))
    G.record("uni_mot_corr_loss_fwd/_bwd" + sfx, "%s rows of pitch %d (%d columns)" % (layout, ld, cols), "B=%d C=%d H=%d W=%d M=%d" % (B, Cc, H, W, M),
             {"embed": list(st)}, gi + go + [gw], workspace_bytes=need)
    # one gradient only: the other buffer is not touched at all
    lone = G.guard_out("grad_embed_1 alone", gi[0].rows, cols, dtype, DEV, ld=ld, guard=G.guard_bytes(ld, es))
    L.check(bwd(P(gi[0]), ST(st), P(gi[1]), ST(st), P(gi[2]), P(gi[3]), B, Cc, H, W, M, float(R.S), flags, None, None, P(lone), ST(st), P(gw), need,
                L.stream_ptr()), "uni_mot_corr_loss_bwd" + sfx)
    torch.cuda.synchronize()
    G.check_all(lone, gw, *gi)
    lone.check_equal(rows_of(g1, layout))
    # the values: the fixture
    for k, got in (("loss", loss), ("g_embed_0", g0), ("g_embed_1", g1)):
        ref = torch.from_numpy(c[k])
        err = float((got.double().cpu() - ref).abs().max() / ref.abs().max())
        assert err <= (1e-12 if f64 else 4 * float(c[k + "_fp32_ref_err"])), (k, err)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(4096, device=DEV)
    s = ST((512, 64, 8, 1))
    ok = dict(B=1, C=8, H=8, W=8, M=4, stride=8.0, flags=3, ws=1 << 20)
    for change, what in (({"M": 2000}, "outside"), ({"C": 2000}, "outside"), ({"B": 0}, "outside"), ({"ws": 16}, "workspace"), ({"flags": 4}, "flags"),
                         ({"stride": 0.0}, "stride"), ({"H": 0}, "empty")):
        a = dict(ok, **change)
        rc = lib.uni_mot_corr_loss_fwd(P(x), s, P(x), s, P(x), a["B"], a["C"], a["H"], a["W"], a["M"], a["stride"], a["flags"], P(x), P(x), a["ws"],
                                       L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    rc = lib.uni_mot_corr_loss_bwd(P(x), s, P(x), s, P(x), P(x), 1, 8, 8, 8, 4, 8.0, 3, P(x), ST((512, 64, 8, 0)), None, None, P(x), 1 << 20,
                                   L.stream_ptr())
    assert rc != 0 and "strides of grad_embed_0" in lib.uni_last_error().decode()
    rc = lib.uni_mot_corr_loss_bwd(P(x), s, P(x), s, P(x), P(x), 1, 8, 8, 8, 4, 8.0, 3, None, None, P(x), ST((512, 32, 8, 1)), P(x), 1 << 20,
                                   L.stream_ptr())                                  # channel stride 32 < 8 rows of 8: channels overlap
    assert rc != 0 and "strides of grad_embed_1" in lib.uni_last_error().decode()
    rc = lib.uni_mot_corr_loss_fwd(None, s, P(x), s, P(x), 1, 8, 8, 8, 4, 8.0, 3, P(x), P(x), 1 << 20, L.stream_ptr())
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
