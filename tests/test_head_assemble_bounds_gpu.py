"""Guard-band runs of uni_head_assemble_fwd / uni_head_assemble_bwd, the method of tests/test_head_loss_bounds_gpu.py: every buffer is a
tests/guard.py allocation [front guard | payload | back guard], inputs poisoned around the payload (NaN) and in the pitch padding of the
gradient rows, results filled with 0xA5.  Guards and padding must come back untouched -- the rows of outputs / dynamic_params and of their
gradients carry a pitch of three elements more than the row -- every result and gradient completely written and BIT-EQUAL to the plain call
(contiguous, exact-size tensors).  Shapes: the `cls8` fixture (80 anchors over three levels: ragged against the tile of 64, B = 3, no
controller maps) and the `edge` fixture (a level of 64 + 1 anchors, P = 169), from NCHW and from channels-last maps.  Refused shapes leave an
error string and write nothing."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import head_assemble_ref as R  # noqa: E402

DEV = "cuda"
PAD = 3


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_head_assemble_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def addr(x):
    return None if x is None else (x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def P(x):
    return None if x is None else C.c_void_p(addr(x))


def PP(xs):
    return None if xs is None else (C.c_void_p * len(xs))(*[addr(x) for x in xs])


def gin(name, t, ld=None):
    t2 = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    return G.guard_in(name, t2, ld=ld, guard=G.guard_bytes(t2.shape[1] if ld is None else ld, t.element_size()))


def gout(name, rows, cols, dtype, ld=None):
    return G.guard_out(name, rows, cols, dtype, DEV, ld=ld, guard=G.guard_bytes(cols if ld is None else ld, torch.empty((), dtype=dtype).element_size()))


def memory_of(t, nchw):
    """the map as the 2-D tensor of its memory: [B C h][w] or [B h w][C]"""
    return t.reshape(-1, t.shape[3]) if nchw else t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@pytest.mark.parametrize("nchw", [1, 0], ids=["nchw", "channels_last"])
@pytest.mark.parametrize("tag", ["cls8", "edge"])
def test_head_assemble_stays_inside_its_buffers(L, tag, nchw):
    p = R.problem(tag)
    B, Cn, Pn, A, Ln = p["B"], p["C"], p["P"], p["A"], len(p["levels"])
    roles = [m for m in R.MAPS if p[m] is not None]
    maps = {m: [t.to(DEV) for t in p[m]] for m in roles}
    mem = {m: [memory_of(t, nchw).contiguous() for t in maps[m]] for m in roles}
    hs = (C.c_int32 * Ln)(*[h for h, _ in p["levels"]])
    ws = (C.c_int32 * Ln)(*[w for _, w in p["levels"]])
    st = (C.c_double * Ln)(*[float(s) for s in p["strides"]])
    lay = (C.c_int32 * Ln)(*[15 * nchw] * Ln)
    lib, W = L.lib(), 5 + Cn
    g_out, g_org = p["g_outputs"].to(DEV), p["g_origin"].to(DEV)
    g_par = p["g_params"].to(DEV) if Pn else None

    def fwd(m_, out_, ld_, org_, xs_, ys_, st_, par_, ldp_, lvl_):
        return lib.uni_head_assemble_fwd(PP(m_["reg"]), PP(m_["obj"]), PP(m_["cls"]), PP(m_.get("ctrl")), hs, ws, st, lay, Ln, B, Cn, Pn, 0, P(out_),
                                         ld_, P(org_), P(xs_), P(ys_), P(st_), P(par_), ldp_, P(lvl_), L.stream_ptr())

    def bwd(reg_, go_, ldg_, gr_, gp_, ldgp_, grads_):
        return lib.uni_head_assemble_bwd(PP(reg_), hs, ws, st, lay, Ln, B, Cn, Pn, 0, P(go_), ldg_, P(gr_), P(gp_), ldgp_, PP(grads_["reg"]),
                                         PP(grads_["obj"]), PP(grads_["cls"]), PP(grads_.get("ctrl")), L.stream_ptr())
    # plain call: exact-size contiguous tensors
    plain = {"outputs": torch.empty(B * A, W, device=DEV), "origin_preds": torch.empty(B * A, 4, device=DEV),
             "x_shifts": torch.empty(1, A, device=DEV), "y_shifts": torch.empty(1, A, device=DEV), "expanded_strides": torch.empty(1, A, device=DEV),
             "dynamic_params": torch.empty(B * A, Pn, device=DEV) if Pn else None,
             "fpn_levels": torch.empty(1, B * A, dtype=torch.int32, device=DEV) if Pn else None}
    L.check(fwd(mem, plain["outputs"], W, plain["origin_preds"], plain["x_shifts"], plain["y_shifts"], plain["expanded_strides"],
                plain["dynamic_params"], Pn, plain["fpn_levels"]), "uni_head_assemble_fwd")
    plain_g = {m: [torch.empty(t.shape, device=DEV) for t in mem[m]] for m in roles}
    L.check(bwd(mem["reg"], g_out, W, g_org, g_par, Pn, plain_g), "uni_head_assemble_bwd")
    torch.cuda.synchronize()

    # forward between guards
    gi = {m: [gin("%s_%d" % (m, k), t) for k, t in enumerate(mem[m])] for m in roles}
    go = {"outputs": gout("outputs", B * A, W, torch.float32, ld=W + PAD), "origin_preds": gout("origin_preds", B * A, 4, torch.float32),
          "x_shifts": gout("x_shifts", 1, A, torch.float32), "y_shifts": gout("y_shifts", 1, A, torch.float32),
          "expanded_strides": gout("expanded_strides", 1, A, torch.float32),
          "dynamic_params": gout("dynamic_params", B * A, Pn, torch.float32, ld=Pn + PAD) if Pn else None,
          "fpn_levels": gout("fpn_levels", 1, B * A, torch.int32) if Pn else None}
    L.check(fwd(gi, go["outputs"], W + PAD, go["origin_preds"], go["x_shifts"], go["y_shifts"], go["expanded_strides"], go["dynamic_params"],
                Pn + PAD, go["fpn_levels"]), "uni_head_assemble_fwd")
    torch.cuda.synchronize()
    bufs = [b for m in roles for b in gi[m]] + [b for b in go.values() if b is not None]
    G.check_all(*bufs)
    for k, b in go.items():
        if b is not None:
            b.check_equal(plain[k])
    G.record("uni_head_assemble_fwd", "nchw=%d ld_out=%d (5 + C = %d) ld_par=%d (P = %d)" % (nchw, W + PAD, W, Pn + PAD, Pn),
             "B=%d A=%d C=%d P=%d levels %s" % (B, A, Cn, Pn, list(p["levels"])), {}, bufs)

    # backward between guards
    gg = [gin("grad_outputs", g_out.reshape(B * A, W), ld=W + PAD), gin("grad_origin", g_org.reshape(B * A, 4))]
    gg.append(gin("grad_params", g_par.reshape(B * A, Pn), ld=Pn + PAD) if Pn else None)
    gm = {m: [gout("grad_%s_%d" % (m, k), t.shape[0], t.shape[1], torch.float32) for k, t in enumerate(mem[m])] for m in roles}
    L.check(bwd(gi["reg"], gg[0], W + PAD, gg[1], gg[2], Pn + PAD, gm), "uni_head_assemble_bwd")        # the guarded reg maps of the forward
    torch.cuda.synchronize()
    bufs = gi["reg"] + [b for b in gg if b is not None] + [b for m in roles for b in gm[m]]
    G.check_all(*bufs)
    for m in roles:
        for b, t in zip(gm[m], plain_g[m]):
            b.check_equal(t)
    G.record("uni_head_assemble_bwd", "nchw=%d ld_gout=%d ld_gpar=%d" % (nchw, W + PAD, Pn + PAD),
             "B=%d A=%d C=%d P=%d levels %s" % (B, A, Cn, Pn, list(p["levels"])), {}, bufs)

    # the values: the fixture (NCHW order of the logical maps)
    c = R.load_case(tag)
    o = plain["outputs"].reshape(B, A, W).cpu()
    assert R.bits_equal(o[..., :2], torch.from_numpy(c["outputs_fp32"])[..., :2]) and R.bits_equal(o[..., 4:], torch.from_numpy(c["outputs_fp32"])[..., 4:])
    assert R.rel_err(o[..., 2:4], c["outputs"][..., 2:4]) <= 4 * float(c["outputs_exp_fp32_ref_err"])
    assert R.bits_equal(plain["origin_preds"].reshape(B, A, 4), c["origin_preds_fp32"])
    for m in ("obj", "cls") + (("ctrl",) if Pn else ()):
        for k, t in enumerate(plain_g[m]):
            logical = t.reshape(maps[m][k].shape) if nchw else t.reshape(B, *maps[m][k].shape[2:], -1).permute(0, 3, 1, 2)
            assert R.bits_equal(logical.contiguous(), c["grad_%s_%d_fp32" % (m, k)]), (m, k)


def test_refused_shapes_leave_an_error_string_and_write_nothing(L):
    lib = L.lib()
    t = torch.zeros(4096, device=DEV)
    out = gout("results", 1, 4096, torch.float32)
    maps = (C.c_void_p * 5)(*[t.data_ptr()] * 5)
    grads = (C.c_void_p * 5)(*[out.ptr] * 5)

    def arrays(hs, ws, strides):
        n = len(hs)
        return (C.c_int32 * n)(*hs), (C.c_int32 * n)(*ws), (C.c_double * n)(*strides), (C.c_int32 * n)(*[15] * n)
    cases = (((), 1, 1, "outside"),                                        # L = 0
             (((2, 2),) * 5, 1, 1, "outside"),                             # L = 5
             (((2, 2),), 1, 0, "outside"),                                 # C = 0
             (((2, 2), (0, 3)), 1, 1, "h=0"),                              # a level with h = 0
             (((2, 2),), 0, 1, "outside"),                                 # B = 0
             (((2, 2),), 1, 257, "outside"))
    for levels, B, Cn, what in cases:
        n = len(levels)
        hs, ws, st, lay = arrays([h for h, _ in levels] or [1], [w for _, w in levels] or [1], [8.0] * max(n, 1))
        rc = lib.uni_head_assemble_fwd(maps, maps, maps, None, hs, ws, st, lay, n, B, Cn, 0, 0, P(out), 5 + Cn, P(out), P(out), P(out), P(out), None, 0,
                                       None, L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (rc, lib.uni_last_error())
        rc = lib.uni_head_assemble_bwd(maps, hs, ws, st, lay, n, B, Cn, 0, 0, P(t), 5 + Cn, P(t), None, 0, grads, grads, grads, None, L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (rc, lib.uni_last_error())
    hs, ws, st, lay = arrays([2], [2], [8.0])
    for kw, what in ((dict(ld=5), "ld_out"), (dict(P=3), "controller maps"), (dict(dtype=3), "map_dtype"), (dict(stride=0.0), "stride")):
        st1 = (C.c_double * 1)(kw.get("stride", 8.0))
        rc = lib.uni_head_assemble_fwd(maps, maps, maps, None, hs, ws, st1, lay, 1, 1, 1, kw.get("P", 0), kw.get("dtype", 0), P(out), kw.get("ld", 6), P(out),
                                       P(out), P(out), P(out), None, 0, None, L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (kw, rc, lib.uni_last_error())
    torch.cuda.synchronize()
    out.check(complete=False)
    assert bool((out.base == G.FILL).all()), "a refused call wrote into its results"
