"""Guard-band runs of uni_prop_labels, uni_prop_dice_pyramid_fwd and uni_prop_dice_pyramid_bwd (fp32 and fp64), the method of
tests/test_mot_corr_bounds_gpu.py: every buffer is a tests/guard.py allocation [front guard | payload | back guard]; inputs are
NaN-poisoned around the payload (0xEE bytes for integer data), outputs filled with 0xA5; the workspace is exactly what
uni_prop_workspace_bytes returns.  Guards must come back untouched, the outputs completely written and BIT-EQUAL to the plain call on
exact-size tensors.  Shapes: the ragged fixtures -- `sot_ragged` (13 x 18: odd H8, W8 % 4 == 2, scalar form), `vos_mask_r4` (6 x 9, masks
read in place, H8 W8 % 4 == 2), `vos_k9` (8 x 8: the 16-byte form, 12 slots of which 9 are live) and `vos_mask_r2` (uint8 masks)."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import prop_loss_ref as R  # noqa: E402

DEV = "cuda"


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_prop_loss_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("tag", ["sot_ragged", "vos_mask_r4", "vos_k9", "vos_mask_r2"])
def test_prop_loss_entries_stay_inside_their_buffers(L, tag, dtype):
    c = R.load_case(tag)
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    Kc, Q, sot = R.case_kc(tag), H8 * W8, kind == "sot"
    f64 = dtype == torch.float64
    sfx, es = ("_f64", 8) if f64 else ("", 4)
    lib = L.lib()
    labels, fwd, bwd = (getattr(lib, n + sfx) for n in ("uni_prop_labels", "uni_prop_dice_pyramid_fwd", "uni_prop_dice_pyramid_bwd"))
    need = lib.uni_prop_workspace_bytes(B, Kc, Q)
    assert need > 0
    t = torch.from_numpy(c["targets"]).to(DEV)
    masks = torch.from_numpy(c["masks"]).to(DEV) if r else None
    pred = torch.from_numpy(c["p8"]).to(DEV, dtype)
    up = [torch.from_numpy(c[k]).to(DEV, dtype) for k in ("w8", "w16", "w32")]
    g_loss = torch.full(() if sot else (B, Kc), 0.75, device=DEV, dtype=dtype)
    groups = 1 if sot else B * Kc
    H16, W16, H32, W32 = H8 // 2, W8 // 2, H8 // 4, W8 // 4

    def run(t_, m_, matched_, num_, gt0_, gt1_, pred_, p16_, p32_, loss_, sums_, ws_, up_, gl_, gpred_):
        L.check(labels(P(t_), P(m_), 1 if mdt == "uint8" else 0, B, M, Kc, int(sot), H8, W8, r, P(matched_), P(num_), P(gt0_), P(gt1_), L.stream_ptr()),
                "uni_prop_labels" + sfx)
        L.check(fwd(P(pred_), P(gt1_), None if sot else P(num_), B, Kc, H8, W8, P(p16_), P(p32_), P(loss_), P(sums_), P(ws_), need, L.stream_ptr()),
                "uni_prop_dice_pyramid_fwd" + sfx)
        L.check(bwd(P(pred_), P(gt1_), None if sot else P(num_), P(sums_), P(up_[0]), P(up_[1]), P(up_[2]), P(gl_), B, Kc, H8, W8, P(gpred_),
                    L.stream_ptr()), "uni_prop_dice_pyramid_bwd" + sfx)
        torch.cuda.synchronize()

    def new(shape, dt):
        return torch.empty(shape, device=DEV, dtype=dt)
    plain = dict(matched=new((B, Kc, 2), torch.int32), num=new((B,), torch.int32), gt0=new((B, Kc, Q), dtype), gt1=new((B, Kc, Q), dtype),
                 p16=new((B * Kc * H16, W16), dtype), p32=new((B * Kc * H32, W32), dtype), loss=new((groups,), dtype),
                 sums=new((groups, 3), torch.float64), gpred=new((B * Kc * H8, W8), dtype))
    run(t, masks, plain["matched"], plain["num"], plain["gt0"], plain["gt1"], pred, plain["p16"], plain["p32"], plain["loss"], plain["sums"],
        torch.empty(need, dtype=torch.uint8, device=DEV), up, g_loss, plain["gpred"])

    gb = G.guard_bytes
    gi = [G.guard_in("targets", t.reshape(B * 2 * M, 6), guard=gb(6, 4)), G.guard_in("pred", pred.reshape(B * Kc * H8, W8), guard=gb(W8, es)),
          G.guard_in("grad_p8", up[0].reshape(-1, W8), guard=gb(W8, es)), G.guard_in("grad_p16", up[1].reshape(-1, W16), guard=gb(W16, es)),
          G.guard_in("grad_p32", up[2].reshape(-1, W32), guard=gb(W32, es)), G.guard_in("grad_loss", g_loss.reshape(-1), guard=gb(groups, es))]
    gm = None
    if r:
        gm = G.guard_in("masks", masks.reshape(-1, r * W8), guard=gb(r * W8, masks.element_size()), poison=0xEE if mdt == "uint8" else None)
    go = {"matched": G.guard_out("matched", B * Kc, 2, torch.int32, DEV), "num": G.guard_out("num_matched", 1, B, torch.int32, DEV),
          "gt0": G.guard_out("gt0", B * Kc, Q, dtype, DEV, guard=gb(Q, es)), "gt1": G.guard_out("gt1", B * Kc, Q, dtype, DEV, guard=gb(Q, es)),
          "p16": G.guard_out("p16", B * Kc * H16, W16, dtype, DEV), "p32": G.guard_out("p32", B * Kc * H32, W32, dtype, DEV),
          "loss": G.guard_out("loss", 1, groups, dtype, DEV), "sums": G.guard_out("sums", groups, 3, torch.float64, DEV),
          "gpred": G.guard_out("grad_pred", B * Kc * H8, W8, dtype, DEV, guard=gb(W8, es))}
    gw = G.guard_ws("workspace", need, DEV)
    run(gi[0], gm, go["matched"], go["num"], go["gt0"], go["gt1"], gi[1], go["p16"], go["p32"], go["loss"], go["sums"], gw, gi[2:5], gi[5], go["gpred"])
    # gt rows of empty slots are zeros and a Dice of an empty slot is an exact zero: 0xA5A5A5A5 is no legal value of either, so "completely
    # written" is checked for every output
    G.check_all(*(gi + [gm] + list(go.values()) + [gw]))
    for k, g_ in go.items():
        g_.check_equal(plain[k])
    G.record("uni_prop_labels / uni_prop_dice_pyramid_fwd/_bwd" + sfx, "%s, %s labels" % (kind, "mask r=%d %s" % (r, mdt) if r else "box"),
             "B=%d Kc=%d H8=%d W8=%d M=%d" % (B, Kc, H8, W8, M), {}, gi + [gm] + list(go.values()) + [gw], workspace_bytes=need)
    # the values: the fixture (labels exactly; p16 / p32 / the Dice at the bound of the precision, from the fixture's own p8)
    assert torch.equal(plain["gt0"].double().cpu(), torch.from_numpy(c["gt0"])) and torch.equal(plain["matched"].cpu(), torch.from_numpy(c["matched"]))
    for k in ("p16", "p32"):
        ref = torch.from_numpy(c[k])
        assert float((plain[k].double().cpu().reshape(ref.shape) - ref).abs().max() / ref.abs().max()) <= (1e-12 if f64 else 2.0 ** -22), k
    ref = torch.from_numpy(c["corr_loss"]).reshape(-1)
    assert float((plain["loss"].double().cpu() - ref).abs().max() / ref.abs().max()) <= (1e-12 if f64 else 2.0 ** -21)


def test_refused_arguments_leave_an_error_string(L):
    lib = L.lib()
    x = torch.zeros(1 << 16, device=DEV)
    ok = dict(B=1, M=4, Kc=2, sot=0, H8=8, W8=8, r=0)
    for change, what in (({"Kc": 5}, "Kc=5 > M"), ({"M": 2000, "Kc": 2}, "M=2000"), ({"H8": 3}, "outside"), ({"sot": 1}, "SOT form"), ({"B": 0}, "outside"),
                         ({"r": 3, "masks": True}, "mask rate")):
        a = dict(ok, **change)
        rc = lib.uni_prop_labels(P(x), P(x) if a.get("masks") else None, 0, a["B"], a["M"], a["Kc"], a["sot"], a["H8"], a["W8"], a["r"], P(x), P(x), P(x), P(x),
                                 L.stream_ptr())
        assert rc != 0 and what in lib.uni_last_error().decode(), (change, rc, lib.uni_last_error())
    rc = lib.uni_prop_dice_pyramid_fwd(P(x), P(x), None, 1, 1, 8, 8, P(x), P(x), P(x), P(x), P(x), 16, L.stream_ptr())
    assert rc != 0 and "workspace" in lib.uni_last_error().decode()
    rc = lib.uni_prop_dice_pyramid_fwd(None, P(x), None, 1, 1, 8, 8, P(x), P(x), P(x), P(x), P(x), 1 << 16, L.stream_ptr())
    assert rc != 0 and "NULL" in lib.uni_last_error().decode()
    rc = lib.uni_prop_dice_pyramid_bwd(P(x), P(x), None, P(x), None, None, None, None, 1, 1, 2, 8, P(x), L.stream_ptr())
    assert rc != 0 and "outside" in lib.uni_last_error().decode()
    torch.cuda.synchronize()
