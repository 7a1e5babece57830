"""Guard-band runs of uni_simota_assign, the method of tests/test_condinst_loss_bounds_gpu.py: every buffer is a tests/guard.py allocation
[front guard | payload | back guard], inputs poisoned around the payload (NaN for floats, an illegal byte for num_gt), outputs and the
workspace filled with 0xA5.  Guards and pitch padding must come back untouched, outputs completely written and BIT-EQUAL to the plain call
(contiguous, exact-size tensors).  The workspace is exactly what uni_simota_workspace_bytes returns.  Shapes: the `edge` fixture (147
anchors: no multiple of 64, box centres outside the image) and the `batch` fixture (three images with 4 / 0 / 9 boxes in labels padded to
12 rows), each with output rows of exact pitch and of pitch ld_out > 5 + C.  The values are held to the fixtures as well."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import simota_ref as R  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_simota_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def gin(name, t, ld=None, poison=None):
    t2 = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    return G.guard_in(name, t2, ld=ld, guard=G.guard_bytes(t2.shape[1] if ld is None else ld, t.element_size()), poison=poison)


def gout(name, rows, cols, dtype):
    return G.guard_out(name, rows, cols, dtype, DEV, guard=G.guard_bytes(cols, torch.empty((), dtype=dtype).element_size()))


def problem(tag):
    """outputs (B, A, 5 + C), labels (B, M, 5), num_gt (B,) int32 and the fixture's per-image results"""
    H, W, Gs, Cn, _ = R.CASES[tag]
    c = R.load_case(tag)
    if len(Gs) == 1:
        outputs = torch.from_numpy(np.concatenate([c["bbox"], c["obj"], c["cls"]], 1))[None]
        labels = torch.from_numpy(np.concatenate([c["gt_classes"][:, None], c["gt_bboxes"]], 1))[None]
        sfx = [""]
    else:
        outputs, labels, sfx = torch.from_numpy(c["outputs"]), torch.from_numpy(c["labels"]), ["_%d" % b if g else None for b, g in enumerate(Gs)]
    return c, (H, W, Cn), outputs.to(DEV).contiguous(), labels.to(DEV).contiguous(), torch.tensor(Gs, dtype=torch.int32, device=DEV), sfx


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("tag", ["edge", "batch"])
def test_simota_assign_stays_inside_its_buffers(L, tag, pad):
    c, (H, W, Cn), outputs, labels, num_gt, sfx = problem(tag)
    B, A, M = outputs.shape[0], outputs.shape[1], labels.shape[1]
    xs, ys, st = R.anchors(H, W, DEV)
    lib, ld = L.lib(), 5 + Cn + pad
    need = lib.uni_simota_workspace_bytes(B, A, M, Cn)
    assert need > 0

    def call(out_, ld_, lab_, ng_, xs_, ys_, st_, fg_, mg_, mi_, nf_, ws_):
        return lib.uni_simota_assign(P(out_), ld_, P(lab_), P(ng_), M, P(xs_), P(ys_), P(st_), B, A, Cn, H, W, P(fg_), P(mg_), P(mi_), P(nf_),
                                     P(ws_), need, L.stream_ptr())
    # plain call: exact-size contiguous tensors
    fg = torch.empty((B, A), dtype=torch.uint8, device=DEV)
    mg, mi = torch.empty((B, A), dtype=torch.int32, device=DEV), torch.empty((B, A), dtype=torch.float32, device=DEV)
    nf, ws = torch.empty((B,), dtype=torch.int32, device=DEV), torch.empty(need, dtype=torch.uint8, device=DEV)
    L.check(call(outputs, 5 + Cn, labels, num_gt, xs, ys, st, fg, mg, mi, nf, ws), "uni_simota_assign")
    torch.cuda.synchronize()

    gi = [gin("outputs", outputs.reshape(B * A, 5 + Cn), ld=ld), gin("labels", labels.reshape(B * M, 5)), gin("num_gt", num_gt, poison=0x7F),
          gin("x_shifts", xs), gin("y_shifts", ys), gin("strides", st)]
    go = [gout("fg_mask", B, A, torch.uint8), gout("matched_gt", B, A, torch.int32), gout("matched_iou", B, A, torch.float32),
          gout("num_fg", 1, B, torch.int32)]
    gw = G.guard_ws("workspace", need, DEV)
    L.check(call(gi[0], ld, gi[1], gi[2], gi[3], gi[4], gi[5], go[0], go[1], go[2], go[3], gw), "uni_simota_assign")
    torch.cuda.synchronize()
    G.check_all(*(gi + go + [gw]))
    for g_, plain in zip(go, (fg, mg, mi, nf)):
        g_.check_equal(plain)
    assert bool((fg <= 1).all())                                    # byte outputs are exempt from the fill-pattern check: 0 / 1 everywhere
    G.record("uni_simota_assign", "ld_out=%d (5 + C = %d)" % (ld, 5 + Cn), "B=%d A=%d M=%d C=%d" % (B, A, M, Cn), {}, gi + go + [gw],
             workspace_bytes=need)
    # the values: the fixture of every image
    for b, s in enumerate(sfx):
        if s is None:
            assert int(nf[b]) == 0 and not fg[b].any() and bool((mg[b] == -1).all()) and not mi[b].any()
            continue
        m = fg[b].bool().cpu().numpy()
        assert int(nf[b]) == int(c["num_fg" + s]) and np.array_equal(m, c["fg_mask" + s])
        assert np.array_equal(mg[b].cpu().numpy()[m], c["matched_gt_inds" + s]) and bool((mg[b][~fg[b].bool()] == -1).all())
        assert float(np.abs(mi[b].cpu().numpy()[m].astype(np.float64) - c["pred_ious_this_matching" + s]).max()) <= 4 * float(c["margin_iou_dev" + s])


def test_refused_shapes_leave_an_error_string(L):
    lib = L.lib()
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(64, dtype=torch.int32, device=DEV)
    for B, A, M, Cn, ld, wsb, what in ((1, 4, 2000, 1, 6, 1 << 20, "outside"), (1, 4, 1, 300, 305, 1 << 20, "outside"), (1, 4, 1, 1, 5, 1 << 20, "ld_out"),
                                       (1, 4, 1, 1, 6, 16, "workspace")):
        rc = lib.uni_simota_assign(P(t), ld, P(t), P(i), M, P(t), P(t), P(t), B, A, Cn, 32, 32, P(i), P(i), P(t), P(i), P(t), wsb, L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (rc, lib.uni_last_error())
    torch.cuda.synchronize()
