"""Guard-band runs of uni_condinst_loss_fwd / _bwd (+ the _f64 pair), the method of tests/test_kernel_bounds_gpu.py: every buffer is a
tests/guard.py allocation [front guard | payload | back guard], inputs poisoned around the payload, outputs and the workspace filled with
0xA5.  Guards and pitch padding must come back untouched, outputs completely written and BIT-EQUAL to the plain call (contiguous,
exact-size tensors).  The workspace is exactly what uni_condinst_loss_workspace_bytes returns (twice that for fp64, as the header says).
Shapes: the ragged fixture (7 x 13, up_rate 4, 3 instances, params rows of pitch 176 > 169) and one instance on a 1 x 1 map at the image
corner.  The fixture's values are held to the fixture bounds as well."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import condinst_loss_ref as R  # noqa: E402
import guard as G  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_condinst_loss_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    if x is None:
        return None
    return C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def gin(name, t, ld=None, poison=None):
    t2 = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    return G.guard_in(name, t2, ld=ld, guard=G.guard_bytes(t2.shape[1] if ld is None else ld, t.element_size()), poison=poison)


def gout(name, rows, cols, dtype, ld=None):
    es = torch.empty((), dtype=dtype).element_size()
    return G.guard_out(name, rows, cols, dtype, DEV, ld=ld, guard=G.guard_bytes(cols if ld is None else ld, es))


def relmax(got, ref):
    return float((got.detach().double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max())


def problem(which, dtype):
    """NHWC tensors of the C-ABI: mf (HW, 8), um (HW, 9 r r), params (n, 169), loc (n, 2), lvl (n) int32, gt (n rH, rW), grad_loss (n)"""
    if which == "ragged":
        c = R.load_case("ragged")
        H, W, r, n = R.CASES["ragged"]
        t = {k: torch.from_numpy(c[k]).to(DEV, dtype) for k in R.INPUTS}
        lvl = torch.from_numpy(c["inst_lvl"]).to(DEV)
    else:                                                # one instance, a 1 x 1 map, the instance at the image corner
        c, (H, W, r, n) = None, (1, 1, 4, 1)
        g = torch.Generator().manual_seed(3)
        t = {"mask_feats": torch.randn(1, 8, 1, 1, generator=g), "up_masks": torch.randn(1, 144, 1, 1, generator=g),
             "params": 0.5 * torch.randn(1, 169, generator=g), "inst_loc": torch.tensor([[7.0, 7.0]]),
             "gt": (torch.rand(1, 1, 4, 4, generator=g) < 0.5).float(), "grad_loss": torch.randn(1, generator=g)}
        t = {k: v.to(DEV, dtype) for k, v in t.items()}
        lvl = torch.zeros(1, dtype=torch.int32, device=DEV)
    mf = t["mask_feats"][0].permute(1, 2, 0).reshape(H * W, 8).contiguous()
    um = t["up_masks"][0].permute(1, 2, 0).reshape(H * W, 9 * r * r).contiguous()
    return c, (H, W, r, n), mf, um, t["params"].contiguous(), t["inst_loc"].contiguous(), lvl, t["gt"].reshape(n * r * H, r * W).contiguous(), t["grad_loss"]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("which", ["ragged", "corner_1x1"])
def test_condinst_loss_forward_and_backward(L, which, dtype):
    f64 = dtype == torch.float64
    c, (H, W, r, n), mf, um, p, loc, lvl, gt, go = problem(which, dtype)
    lib, sfx, ldp = L.lib(), "_f64" if f64 else "", 176
    need = lib.uni_condinst_loss_workspace_bytes(n, H, W, r) * (2 if f64 else 1)
    fwd_fn, bwd_fn = getattr(lib, "uni_condinst_loss_fwd" + sfx), getattr(lib, "uni_condinst_loss_bwd" + sfx)

    def fwd(mf_, um_, p_, ld, loc_, lvl_, gt_, loss_, sums_, ws_):
        return fwd_fn(P(mf_), P(um_), P(p_), ld, P(loc_), P(lvl_), P(gt_), n, H, W, r, P(loss_), P(sums_), P(ws_), need, L.stream_ptr())

    def bwd(mf_, um_, p_, ld, loc_, lvl_, gt_, sums_, go_, a, b, c_, ldg, ws_):
        # grad_params shares ldp with params in the C-ABI: the plain call uses rows of the same pitch
        assert ld == ldg
        return bwd_fn(P(mf_), P(um_), P(p_), ld, P(loc_), P(lvl_), P(gt_), P(sums_), P(go_), n, H, W, r, P(a), P(b), P(c_), P(ws_), need,
                      L.stream_ptr())

    # plain calls: exact-size tensors; params rows of the same pitch (a pitched plain tensor, padding zero)
    pw = torch.zeros((n, ldp), device=DEV, dtype=dtype)
    pw[:, :169] = p
    ws = torch.empty(need, device=DEV, dtype=torch.uint8)
    loss, sums = torch.empty(n, device=DEV, dtype=dtype), torch.empty((n, 3), device=DEV, dtype=dtype)
    L.check(fwd(mf, um, pw, ldp, loc, lvl, gt, loss, sums, ws), "condinst_loss_fwd")
    torch.cuda.synchronize()

    gi = [gin("mask_feats", mf), gin("up_masks", um), gin("params", p, ld=ldp), gin("inst_loc", loc), gin("inst_lvl", lvl, poison=0x7F),
          gin("gt", gt)]
    gl, gs, gw = gout("loss", 1, n, dtype), gout("sums", n, 3, dtype), G.guard_ws("workspace", need, DEV)
    L.check(fwd(gi[0], gi[1], gi[2], ldp, gi[3], gi[4], gi[5], gl, gs, gw), "condinst_loss_fwd")
    torch.cuda.synchronize()
    G.check_all(*(gi + [gl, gs, gw]))
    gl.check_equal(loss)
    gs.check_equal(sums)
    G.record("uni_condinst_loss_fwd" + sfx, "ldp=%d" % ldp, "n=%d H8=%d W8=%d r=%d" % (n, H, W, r), {}, gi + [gl, gs, gw], workspace_bytes=need)
    if c is not None:
        e = relmax(gl.payload().reshape(n), torch.from_numpy(c["loss"]))
        assert e <= (1e-12 if f64 else 4 * float(c["loss_fp32_ref_err"])), e
    else:                                                # the corner case against the restatement in fp64
        def restated(dt):
            return R.dice_loss(mf.to(dt).reshape(1, 1, 1, 8).permute(0, 3, 1, 2), um.to(dt).reshape(1, 1, 1, 144).permute(0, 3, 1, 2),
                               p.to(dt), loc.to(dt), lvl, gt.to(dt).reshape(1, 4, 4), r)
        ref = restated(torch.float64)                    # fp32 bound: 4 x the restatement's own fp32 error, at least one rounding of the result
        assert relmax(gl.payload().reshape(n), ref) <= (1e-12 if f64 else 4 * max(relmax(restated(torch.float32), ref), 2.0 ** -24))

    full = None
    for needs in ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (True, False, True)):
        pa = torch.empty((H * W, 8), device=DEV, dtype=dtype) if needs[0] else None
        pb = torch.empty((H * W, 9 * r * r), device=DEV, dtype=dtype) if needs[1] else None
        pc = torch.zeros((n, ldp), device=DEV, dtype=dtype) if needs[2] else None
        L.check(bwd(mf, um, pw, ldp, loc, lvl, gt, sums, go, pa, pb, pc, ldp, ws), "condinst_loss_bwd")
        torch.cuda.synchronize()
        gi = [gin("mask_feats", mf), gin("up_masks", um), gin("params", p, ld=ldp), gin("inst_loc", loc), gin("inst_lvl", lvl, poison=0x7F),
              gin("gt", gt), gin("sums", sums), gin("grad_loss", go)]
        oa = gout("grad_mask_feats", H * W, 8, dtype) if needs[0] else None
        ob = gout("grad_up_masks", H * W, 9 * r * r, dtype) if needs[1] else None
        oc = gout("grad_params", n, 169, dtype, ld=ldp) if needs[2] else None
        gw = G.guard_ws("workspace", need, DEV)
        L.check(bwd(gi[0], gi[1], gi[2], ldp, gi[3], gi[4], gi[5], gi[6], gi[7], oa, ob, oc, ldp, gw), "condinst_loss_bwd")
        torch.cuda.synchronize()
        G.check_all(*(gi + [oa, ob, oc, gw]))
        plain = (pa, pb, None if pc is None else pc[:, :169].contiguous())
        if all(needs):
            full = plain
        for i, (o_, p_) in enumerate(zip((oa, ob, oc), plain)):
            if o_ is None:
                continue
            o_.check_equal(p_)
            o_.check_equal(full[i], "the call with all three outputs")          # one writer per element: the same bits
        if pc is not None:
            assert not pc[:, 169:].any()                                         # the plain call leaves the pitch padding alone as well
        G.record("uni_condinst_loss_bwd" + sfx, "outputs %s, ldp=%d" % ("".join("x" if k else "-" for k in needs), ldp),
                 "n=%d H8=%d W8=%d r=%d" % (n, H, W, r), {}, gi + [oa, ob, oc, gw], workspace_bytes=need)
    if c is not None:
        got = {"g_mask_feats": full[0].reshape(H, W, 8).permute(2, 0, 1)[None], "g_up_masks": full[1].reshape(H, W, -1).permute(2, 0, 1)[None],
               "g_params": full[2]}
        for k, t in got.items():
            e = relmax(t, torch.from_numpy(c[k]))
            assert e <= (1e-12 if f64 else 4 * float(c[k + "_fp32_ref_err"])), (k, e)
