"""Guard-band runs of uni_head_loss_fwd / uni_head_loss_bwd, the method of tests/test_simota_bounds_gpu.py: every buffer is a tests/guard.py
allocation [front guard | payload | back guard], inputs poisoned around the payload (NaN for floats, an illegal byte for the integer
arrays), in the pitch padding of `outputs` / `origin_preds` and in the `labels` rows beyond num_gt; outputs and the workspace -- exactly
uni_head_loss_workspace_bytes -- filled with 0xA5.  Guards and padding must come back untouched, out[5] and both gradients completely
written (the padding columns of grad_outputs excepted) and BIT-EQUAL to the plain call (contiguous, exact-size tensors, clean labels).
Shapes: the `edge` fixture (147 anchors: no multiple of 64) and the `batch` fixture (three images with 4 / 0 / 9 boxes in labels padded to
12 rows), each with exact pitch and with ld_out = 5 + C + 3.  The values are held to the fixtures as well."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import head_loss_ref as R  # noqa: E402
import simota_ref as S  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_head_loss_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def gin(name, t, ld=None, poison=None):
    t2 = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    return G.guard_in(name, t2, ld=ld, guard=G.guard_bytes(t2.shape[1] if ld is None else ld, t.element_size()), poison=poison)


def gout(name, rows, cols, dtype, ld=None):
    return G.guard_out(name, rows, cols, dtype, DEV, ld=ld, guard=G.guard_bytes(cols if ld is None else ld, torch.empty((), dtype=dtype).element_size()))


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("tag", ["edge", "batch"])
def test_head_loss_stays_inside_its_buffers(L, tag, pad):
    c = R.load_case(tag)
    H, W, Cn = (int(v) for v in c["shape"])
    outputs, origin, labels = (torch.from_numpy(c[n]).to(DEV) for n in ("outputs", "origin_preds", "labels"))
    B, A, M = outputs.shape[0], outputs.shape[1], labels.shape[1]
    xs, ys, st = S.anchors(H, W, DEV)
    fg = torch.from_numpy(c["fg_mask"]).to(DEV).to(torch.uint8)
    mg = torch.from_numpy(c["matched_gt_inds"]).to(DEV).to(torch.int32)
    mi = torch.from_numpy(c["matched_ious_fp32"]).to(DEV)
    nf = torch.from_numpy(c["num_fg_per_image"]).to(DEV).to(torch.int32)
    ng = (labels.sum(2) > 0).sum(1).to(torch.int32)
    gw_ = torch.from_numpy(c["grad_out"]).float().to(DEV)
    poisoned = labels.clone()                                       # the rows beyond num_gt: never read (matched_gt < num_gt)
    for b in range(B):
        poisoned[b, int(ng[b]):] = float("nan")
    assert tag != "batch" or bool(poisoned.isnan().any())
    lib, ld, ldo = L.lib(), 5 + Cn + pad, 4 + pad
    need = lib.uni_head_loss_workspace_bytes(B, A, Cn)
    assert need > 0

    def fwd(out_, ld_, org_, ldo_, lab_, fg_, mg_, mi_, nf_, ng_, xs_, ys_, st_, res_, ws_):
        return lib.uni_head_loss_fwd(P(out_), ld_, P(org_), ldo_, P(lab_), M, P(fg_), P(mg_), P(mi_), P(nf_), P(ng_), P(xs_), P(ys_), P(st_), B, A, Cn,
                                     5.0, P(res_), P(ws_), need, L.stream_ptr())

    def bwd(out_, ld_, org_, ldo_, lab_, fg_, mg_, mi_, nf_, ng_, xs_, ys_, st_, g_, go_, ldg_, gr_, ws_):
        return lib.uni_head_loss_bwd(P(out_), ld_, P(org_), ldo_, P(lab_), M, P(fg_), P(mg_), P(mi_), P(nf_), P(ng_), P(xs_), P(ys_), P(st_), P(g_), B, A,
                                     Cn, 5.0, P(go_), ldg_, P(gr_), P(ws_), need, L.stream_ptr())
    # plain call: exact-size contiguous tensors, clean labels
    res, ws = torch.empty(5, device=DEV), torch.empty(need, dtype=torch.uint8, device=DEV)
    g_out, g_org = torch.empty(B, A, 5 + Cn, device=DEV), torch.empty(B, A, 4, device=DEV)
    plain_in = (outputs, 5 + Cn, origin, 4, labels, fg, mg, mi, nf, ng, xs, ys, st)
    L.check(fwd(*plain_in, res, ws), "uni_head_loss_fwd")
    L.check(bwd(*plain_in, gw_, g_out, 5 + Cn, g_org, ws), "uni_head_loss_bwd")
    torch.cuda.synchronize()

    for which in ("fwd", "bwd"):
        gi = [gin("outputs", outputs.reshape(B * A, 5 + Cn), ld=ld), gin("origin_preds", origin.reshape(B * A, 4), ld=ldo),
              gin("labels", poisoned.reshape(B * M, 5)), gin("fg_mask", fg, poison=0x7F), gin("matched_gt", mg, poison=0x7F), gin("matched_iou", mi),
              gin("num_fg", nf, poison=0x7F), gin("num_gt", ng, poison=0x7F), gin("x_shifts", xs), gin("y_shifts", ys), gin("strides", st)]
        gws = G.guard_ws("workspace", need, DEV)
        ins = (gi[0], ld, gi[1], ldo) + tuple(gi[2:])
        if which == "fwd":
            go = [gout("out", 1, 5, torch.float32)]
            L.check(fwd(*ins, go[0], gws), "uni_head_loss_fwd")
            plain = [res]
        else:
            gi.append(gin("grad_out", gw_))
            go = [gout("grad_outputs", B * A, 5 + Cn, torch.float32, ld=ld), gout("grad_origin", B * A, 4, torch.float32)]
            L.check(bwd(*ins, gi[-1], go[0], ld, go[1], gws), "uni_head_loss_bwd")
            plain = [g_out, g_org]
        torch.cuda.synchronize()
        G.check_all(*(gi + go + [gws]))
        for g_, p_ in zip(go, plain):
            g_.check_equal(p_)
        G.record("uni_head_loss_" + which, "ld_out=%d (5 + C = %d), ld_org=%d" % (ld, 5 + Cn, ldo), "B=%d A=%d M=%d C=%d" % (B, A, M, Cn), {},
                 gi + go + [gws], workspace_bytes=need)
    # the values: the fixture
    got = dict(zip(R.QUANTITIES[:5], res.cpu()))
    got["grad_outputs"], got["grad_origin"] = g_out, g_org
    for k in R.QUANTITIES:
        e, bound = R.rel_err(got[k], c[k]), R.bound32(c[k + "_fp32_ref_err"])
        print("%-12s err %.3g  bound %.3g" % (k, e, bound))
        assert e <= bound, (k, e, bound)


def test_refused_shapes_leave_an_error_string(L):
    lib = L.lib()
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    for B, A, M, Cn, ld, wsb, what in ((1, 4, 2000, 1, 6, 1 << 20, "outside"), (1, 4, 1, 300, 305, 1 << 20, "outside"), (1, 4, 1, 1, 5, 1 << 20, "ld_out"),
                                       (1, 4, 1, 1, 6, 16, "workspace")):
        rc = lib.uni_head_loss_fwd(P(t), ld, P(t), 4, P(t), M, P(i), P(i), P(t), P(i), P(i), P(t), P(t), P(t), B, A, Cn, 5.0, P(t), P(t), wsb,
                                   L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (rc, lib.uni_last_error())
        rc = lib.uni_head_loss_bwd(P(t), ld, P(t), 4, P(t), M, P(i), P(i), P(t), P(i), P(i), P(t), P(t), P(t), P(t), B, A, Cn, 5.0, P(t), ld, P(t), P(t),
                                   wsb, L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (rc, lib.uni_last_error())
    rc = lib.uni_head_loss_bwd(P(t), 6, None, 0, P(t), 1, P(i), P(i), P(t), P(i), P(i), P(t), P(t), P(t), P(t), 1, 4, 1, 5.0, P(t), 6, P(t), P(t), 1 << 20,
                               L.stream_ptr())
    assert rc != 0 and "grad_origin without origin_preds" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
