"""Guard-band runs of uni_block_tail_fwd / _bwd (fp32 and fp64, residual / grad_out in both layouts), the method of
tests/test_dwln_train_bounds_gpu.py: every buffer is a tests/guard.py allocation [front guard | payload | back guard].  y, residual, grad_out,
gamma and scale are NaN-poisoned beyond their last element, so a read outside a map reaches an output; out, grad_y and grad_gamma are filled
with 0xA5 and must come back completely written; the workspace is exactly what uni_block_tail_workspace_bytes returns (twice that for fp64).
Guards must come back untouched and every output BIT-EQUAL to the plain call on exact-size tensors.  Shapes: the fixtures `c96` (63 pixels per
image: a transpose tile that ends inside the second image), `c100` (C no multiple of 64, a dropped image) and `hw130` (three pixel tiles, the
last of 2 pixels), held to the fixture values as well, and a single pixel of 192 channels."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import block_tail_ref as R  # noqa: E402
import guard as G  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_block_tail_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


@pytest.mark.parametrize("nchw", [0, 1], ids=["cl", "nchw"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("tag", ["c96", "c100", "hw130", "pixel"])
def test_block_tail_stays_inside_its_buffers(L, tag, dtype, nchw):
    if tag == "pixel":
        shape, c = (1, 192, 1, 1), None
        ins = R.draw("plain", 9, shape, scale=(1 / 0.7,))
    else:
        shape, c = R.CASES[tag], R.load_case(tag)
        ins = [torch.from_numpy(c[n]) for n in R.INPUTS]
    B, Cc, H, W = shape
    M = B * H * W
    f64 = dtype == torch.float64
    sfx = "_f64" if f64 else ""
    lib = L.lib()
    fwd, bwd = getattr(lib, "uni_block_tail_fwd" + sfx), getattr(lib, "uni_block_tail_bwd" + sfx)
    need = lib.uni_block_tail_workspace_bytes(B, H, W, Cc) * (2 if f64 else 1)
    assert need == 4 * 1024 * Cc * (2 if f64 else 1)

    def lay(t):                                   # (B, C, H, W) -> rows of the layout under test
        return t.reshape(B * Cc, H * W).contiguous() if nchw else t.permute(0, 2, 3, 1).reshape(M, Cc).contiguous()

    y = ins[0].reshape(M, Cc).to(DEV, dtype)
    res, g = lay(ins[1]).to(DEV, dtype), lay(ins[4]).to(DEV, dtype)
    gamma, scale = ins[2].to(DEV, dtype), ins[3].to(DEV, dtype)
    es = y.element_size()

    def run(y_, res_, g_, gamma_, scale_, out_, gy_, gg_, ws_):
        L.check(fwd(P(y_), 0, P(res_), nchw, P(gamma_), P(scale_), B, H, W, Cc, P(out_), L.stream_ptr()), "uni_block_tail_fwd" + sfx)
        L.check(bwd(P(y_), 0, P(g_), nchw, P(gamma_), P(scale_), B, H, W, Cc, P(gy_), P(gg_), P(ws_), need, L.stream_ptr()), "uni_block_tail_bwd" + sfx)
        torch.cuda.synchronize()

    e = lambda *s: torch.empty(*s, device=DEV, dtype=dtype)       # noqa: E731
    plain = dict(out=e(M, Cc), g_y=e(M, Cc), g_gamma=e(Cc))
    run(y, res, g, gamma, scale, *plain.values(), torch.empty(need, dtype=torch.uint8, device=DEV))

    gi = [G.guard_in(n, t, guard=G.guard_bytes(t.shape[-1], es)) for n, t in (("y", y), ("residual", res), ("grad_out", g), ("gamma", gamma),
                                                                               ("scale", scale))]
    go = [G.guard_out(n, t.reshape(-1, t.shape[-1]).shape[0], t.shape[-1], dtype, DEV, guard=G.guard_bytes(t.shape[-1], es)) for n, t in plain.items()]
    gw = G.guard_ws("workspace", need, DEV)
    run(*gi, *go, gw)
    G.check_all(*(gi + go + [gw]))
    for gd, t in zip(go, plain.values()):
        gd.check_equal(t)
    G.record("uni_block_tail_fwd/_bwd" + sfx, "nchw=%d" % nchw, "B=%d C=%d H=%d W=%d" % (B, Cc, H, W), {}, gi + go + [gw], workspace_bytes=need)
    # grad_y alone: neither grad_gamma nor the workspace is touched (both NULL), grad_y has the same bits
    lone = G.guard_out("grad_y alone", M, Cc, dtype, DEV, guard=G.guard_bytes(Cc, es))
    L.check(bwd(P(gi[0]), 0, P(gi[2]), nchw, P(gi[3]), P(gi[4]), B, H, W, Cc, P(lone), None, None, 0, L.stream_ptr()), "uni_block_tail_bwd" + sfx)
    # grad_gamma alone: grad_y is not touched (NULL), grad_gamma has the same bits
    lone_g = G.guard_out("grad_gamma alone", 1, Cc, dtype, DEV, guard=G.guard_bytes(Cc, es))
    L.check(bwd(P(gi[0]), 0, P(gi[2]), nchw, P(gi[3]), P(gi[4]), B, H, W, Cc, None, P(lone_g), P(gw), need, L.stream_ptr()), "uni_block_tail_bwd" + sfx)
    torch.cuda.synchronize()
    G.check_all(lone, lone_g, gw, *gi)
    lone.check_equal(plain["g_y"])
    lone_g.check_equal(plain["g_gamma"])
    if c is not None:                                 # the values: the fixture
        got = dict(out=plain["out"].reshape(B, H, W, Cc).permute(0, 3, 1, 2), g_y=plain["g_y"].reshape(B, H, W, Cc), g_gamma=plain["g_gamma"])
        for k in got:
            err = R.rel_err(got[k], torch.from_numpy(c[k]))
            assert err <= (1e-12 if f64 else 4 * float(c[k + "_fp32_ref_err"])), (k, err)


@pytest.mark.parametrize("half", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("nchw", [0, 1], ids=["cl", "nchw"])
@pytest.mark.parametrize("tag", ["c96", "c100"])
def test_half_y_stays_inside_its_buffers(L, tag, nchw, half):
    """y and grad_y in fp16 / bf16 (y_dtype 1 / 2): rows of 2 C bytes; c96 takes 8 channels per lane in the channels-last kernels, c100 four"""
    c = R.load_case(tag)
    B, Cc, H, W = R.CASES[tag]
    M = B * H * W
    lib = L.lib()
    need = lib.uni_block_tail_workspace_bytes(B, H, W, Cc)
    yd = 1 if half == torch.float16 else 2
    lay = (lambda t: t.reshape(B * Cc, H * W).contiguous()) if nchw else (lambda t: t.permute(0, 2, 3, 1).reshape(M, Cc).contiguous())
    y = torch.from_numpy(c["y"]).reshape(M, Cc).to(DEV, half)
    res, g = (lay(torch.from_numpy(c[n])).to(DEV) for n in ("residual", "grad_out"))
    gamma, scale = torch.from_numpy(c["gamma"]).to(DEV), torch.from_numpy(c["scale"]).to(DEV)

    def run(y_, res_, g_, gamma_, scale_, out_, gy_, gg_, ws_):
        L.check(lib.uni_block_tail_fwd(P(y_), yd, P(res_), nchw, P(gamma_), P(scale_), B, H, W, Cc, P(out_), L.stream_ptr()), "uni_block_tail_fwd")
        L.check(lib.uni_block_tail_bwd(P(y_), yd, P(g_), nchw, P(gamma_), P(scale_), B, H, W, Cc, P(gy_), P(gg_), P(ws_), need, L.stream_ptr()),
                "uni_block_tail_bwd")
        torch.cuda.synchronize()

    plain = dict(out=torch.empty(M, Cc, device=DEV), g_y=torch.empty(M, Cc, device=DEV, dtype=half), g_gamma=torch.empty(Cc, device=DEV))
    run(y, res, g, gamma, scale, *plain.values(), torch.empty(need, dtype=torch.uint8, device=DEV))
    gi = [G.guard_in(n, t, guard=G.guard_bytes(t.shape[-1], t.element_size())) for n, t in (("y", y), ("residual", res), ("grad_out", g),
                                                                                             ("gamma", gamma), ("scale", scale))]
    go = [G.guard_out(n, t.reshape(-1, t.shape[-1]).shape[0], t.shape[-1], t.dtype, DEV, guard=G.guard_bytes(t.shape[-1], t.element_size()))
          for n, t in plain.items()]
    gw = G.guard_ws("workspace", need, DEV)
    run(*gi, *go, gw)
    G.check_all(*(gi + go + [gw]))
    for gd, t in zip(go, plain.values()):
        gd.check_equal(t)
    G.record("uni_block_tail_fwd/_bwd", "nchw=%d y=%s" % (nchw, half), "B=%d C=%d H=%d W=%d" % (B, Cc, H, W), {}, gi + go + [gw], workspace_bytes=need)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(1 << 16, device=DEV)
    ok = dict(B=1, H=4, W=4, C=8, yd=0)
    for change, what in (({"C": 6}, "outside"), ({"C": 2052}, "outside"), ({"B": 0}, "outside"), ({"H": 0}, "outside"), ({"yd": 3}, "y_dtype")):
        a = dict(ok, **change)
        rc = lib.uni_block_tail_fwd(P(x), a["yd"], P(x), 0, P(x), P(x), a["B"], a["H"], a["W"], a["C"], P(x), L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    rc = lib.uni_block_tail_fwd_f64(P(x), 1, P(x), 0, P(x), P(x), 1, 4, 4, 8, P(x), L.stream_ptr())
    assert rc != 0 and "y_dtype" in lib.uni_last_error().decode()
    assert lib.uni_block_tail_workspace_bytes(1, 4, 4, 6) == 0 and lib.uni_block_tail_workspace_bytes(1, 4, 4, 8) == 4 * 1024 * 8
    assert lib.uni_block_tail_workspace_bytes(1 << 11, 1 << 10, 1 << 10, 8) == 0                      # B H W = 2^31
    rc = lib.uni_block_tail_bwd(P(x), 0, P(x), 0, P(x), P(x), 1, 4, 4, 8, P(x), P(x), P(x), 16, L.stream_ptr())
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_block_tail_bwd(P(x), 0, P(x), 0, P(x), P(x), 1, 4, 4, 8, P(x), P(x), None, 1 << 20, L.stream_ptr())
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_block_tail_fwd(None, 0, P(x), 0, P(x), P(x), 1, 4, 4, 8, P(x), L.stream_ptr())
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = lib.uni_block_tail_fwd(C.c_void_p(x.data_ptr() + 4), 0, P(x), 0, P(x), P(x), 1, 4, 4, 8, P(x), L.stream_ptr())
    assert rc != 0 and "aligned" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
