"""CPU-side checks of the batched CondInst mask loss (uni_head_mask_loss_fwd / _bwd, ops.head_mask_loss): the restatement
(tests/head_mask_loss_ref.py) equals the fixtures the reference's own get_losses produced; the fixtures are what their generator says; the
new symbols are declared, exported and bound; the Python surface exists and fails the library's way without a device."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import condinst_loss_ref as CR
import head_mask_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_head_mask_loss_workspace_bytes": 6, "uni_head_mask_loss_fwd": 23, "uni_head_mask_loss_bwd": 27,
               "uni_head_mask_loss_fwd_f64": 23, "uni_head_mask_loss_bwd_f64": 27}
# tag -> (B, A, H8, W8, up_rate, M, foreground anchors per image)
GEOMETRY = {"sot": (1, 126, 8, 12, 4, 1, [7]), "batch": (3, 126, 8, 12, 4, 12, [23, 0, 29]), "edge": (1, 147, 9, 13, 4, 6, [29]),
            "small_r2": (1, 315, 12, 20, 2, 12, [57]), "tiny_r8": (1, 21, 4, 4, 8, 1, [1]), "empty": (3, 126, 8, 12, 4, 12, [0, 0, 0])}


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_equals_the_fixture(tag):
    c = R.load_case(tag)
    args = R.fixture_tensors(c, tag)
    got = R.loss_and_grads(*args, float(c["grad_out"]))
    want = R.expected(c, tag)
    for k in R.QUANTITIES:
        assert want[k].dtype == torch.float64 and got[k].shape == want[k].shape, k
        e = R.rel_err(got[k], want[k])
        assert e <= 1e-12, (tag, k, e)
    chunked = R.loss_and_grads(*args, float(c["grad_out"]), chunk=3)
    for k in R.QUANTITIES:
        assert R.rel_err(chunked[k], got[k]) <= 1e-13, (tag, k)
    fg = args[5]
    assert not got["g_dynamic_params"][~fg].any()                                      # background rows: exact zeros
    for b in range(fg.shape[0]):
        if not bool(fg[b].any()):                                                       # an image without foreground: exact zeros
            assert float(got["per_image"][b]) == 0.0 and not got["g_mask_feats"][b].any() and not got["g_up_masks"][b].any()


def test_fixture_cases_are_the_described_ones():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(R.GOLD, "head_mask_loss_*.npz"))) == \
        sorted("head_mask_loss_%s.npz" % t for t in R.CASES)
    assert sorted(R.CASES) == sorted(GEOMETRY)
    for tag, (B, A, H8, W8, r, M, counts) in GEOMETRY.items():
        path = os.path.join(R.GOLD, "head_mask_loss_%s.npz" % tag)
        assert os.path.getsize(path) < (1 << 20), "a committed file stays below 1 MiB"
        c = R.load_case(tag)
        (H, W), fg, matched, _, M_ = R.load_assignment(tag)
        assert tuple(c["shape"]) == (B, A, H8, W8, r, M) and (H // 8, W // 8, M_, R.CASES[tag][1]) == (H8, W8, M, r)
        assert fg.shape == (B, A) and fg.sum(dim=1).tolist() == counts
        assert c["mask_feats"].shape == (B, 8, H8, W8) and c["up_masks"].shape == (B, 9 * r * r, H8, W8)
        assert c["dynamic_params"].shape == (B, A, 169) and c["fpn_levels"].shape == (B, A) and c["masks"].shape == (B, M, r * H8, r * W8)
        assert all(c[k].dtype == np.float32 for k in R.INPUTS if k != "fpn_levels") and c["fpn_levels"].dtype == np.int32
        assert set(np.unique(c["masks"])) <= {0.0, 1.0} and 0 <= c["fpn_levels"].min() and c["fpn_levels"].max() <= 4
        assert float(c["grad_out"]) == np.float32(R.GRAD_OUT) != 1.0
        assert c["g_dynamic_params_fg"].shape == (sum(counts), 169) and c["per_image"].shape == (B,) and c["loss_condinst"].shape == ()
        for k in R.QUANTITIES:
            e = float(c[k + "_fp32_ref_err"])
            assert 0.0 <= e < 1e-5, (tag, k, e)
            if sum(counts) == 0:
                assert e == 0.0 and not np.asarray(c["g_dynamic_params_fg" if k == "g_dynamic_params" else k]).any(), (tag, k)
            elif k != "loss_condinst":                               # a scalar may round to the same fp32 value
                assert e > 1e-9, (tag, k, e)
        # no hidden pre-activation of a foreground instance sits on a ReLU kink: fp32 and fp64 take the same branches
        args = R.fixture_tensors(c, tag)
        worst = float("inf")
        for b in range(B):
            if counts[b]:
                p, loc, lvl, _ = R.instances(b, *args[2:10])
                _, p0, p1 = CR.pre_activations(args[0][b:b + 1], p, loc, lvl)
                worst = min(worst, float(p0.abs().min()), float(p1.abs().min()))
                _, q0, q1 = CR.pre_activations(args[0][b:b + 1].float(), p.float(), loc.float(), lvl)
                assert torch.equal(q0 > 0, p0 > 0) and torch.equal(q1 > 0, p1 > 0)
        assert worst > 1e-6 and (worst == float("inf") or abs(worst - float(c["min_abs_pre_activation"])) <= 1e-12)
    sot = R.load_assignment("sot")
    assert len(set(sot[2][sot[1]].tolist())) == 1                                       # all instances share one ground-truth row
    batch = R.load_case("batch")
    assert float(batch["per_image"][1]) == 0.0 and float(batch["per_image"][0]) > 0 and float(batch["per_image"][2]) > 0
    assert abs(float(batch["loss_condinst"]) - float(batch["per_image"].sum()) / 2) <= 1e-15      # num_valid = 2, not B = 3


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn_head_mask.py:568-569, :675-694, :731-732" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s, arity in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, code)
        assert m, "%s is not declared in include/unicorn_hip.h" % s
        assert len(m.group(1).split(",")) == arity, (s, m.group(1))
        assert s in _lib.PROTOS, "%s is not bound in _lib.PROTOS" % s
        assert len(_lib.PROTOS[s][1]) == arity, (s, len(_lib.PROTOS[s][1]))
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    # host-side part that needs no device: the documented formula, O(capacity H8 W8), below one (N, r H8, r W8) map per instance slot
    B, A, H8, W8, r, cap = 2, 21000, 100, 160, 4, 200
    ws = lib.uni_head_mask_loss_workspace_bytes(B, A, H8, W8, r, cap)
    hw = H8 * W8
    table = (4 * (4 + 2 * B + 4 * cap + B * A) + 7) // 8 * 8
    assert ws == table + 4 * (cap * (2 * hw + 3 * -(-hw // (256 // (r * r))) + 169 * -(-hw // 1024) + 3) + 9 * -(-cap // 8) * hw + 64 * B * hw)
    assert 3 * cap * hw * 4 <= ws < cap * hw * r * r * 4 // 3
    for bad in ((0, A, H8, W8, r, cap), (B, 0, H8, W8, r, cap), (B, A, 0, W8, r, cap), (B, A, H8, W8, 17, cap), (B, A, H8, W8, r, 0),
                (B, A, H8, W8, r, -1), (65536, A, H8, W8, r, cap)):
        assert lib.uni_head_mask_loss_workspace_bytes(*bad) == 0, bad
    assert lib.uni_head_mask_loss_workspace_bytes(1, 1, 1, 1, 4, 1) > 0


def test_python_surface_rejects_cpu_tensors_bad_shapes_and_dtypes():
    from unicorn_amd import _lib, ops
    assert issubclass(ops.HeadMaskLossFunction, torch.autograd.Function) and callable(ops.head_mask_loss)
    B, A, H, W, r, M = 2, 6, 3, 5, 4, 3
    mf, um, dp = torch.zeros(B, 8, H, W), torch.zeros(B, 9 * r * r, H, W), torch.zeros(B, A, 169)
    lvl, masks = torch.zeros(B, A, dtype=torch.int64), torch.zeros(B, M, r * H, r * W)
    asg = (torch.zeros(B, A, dtype=torch.bool), torch.zeros(B, A, dtype=torch.int64), torch.zeros(B, A), torch.zeros(B, dtype=torch.int64))
    xs, ys, st = torch.zeros(1, A), torch.zeros(1, A), torch.full((1, A), 8.0)

    def call(mf=mf, um=um, dp=dp, lvl=lvl, masks=masks, asg=asg, xs=xs, r=r, **kw):
        return ops.head_mask_loss(mf, um, dp, lvl, masks, asg, xs, ys, st, r, **kw)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.UnicornHipError, match="HIP device tensors"):
            call()
        with pytest.raises(_lib.UnicornHipError, match="HIP device tensors"):
            ops.head_mask_loss(mf.double(), um.double(), dp.double(), lvl, masks.double(), asg, xs.double(), ys.double(), st.double(), r)
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        ops.head_mask_loss(mf.half(), um.half(), dp.half(), lvl, masks.half(), asg, xs.half(), ys.half(), st.half(), r)
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        ops.head_mask_loss(mf.bfloat16(), um.bfloat16(), dp.bfloat16(), lvl, masks.bfloat16(), asg, xs.bfloat16(), ys.bfloat16(),
                           st.bfloat16(), r)
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        call(um=um.double())
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        call(masks=masks.bool())                                                           # uint8 / bool ground truth is out of scope
    with pytest.raises(_lib.UnicornHipError, match="exactly"):
        call(masks=torch.zeros(B, M, r * H, r * W + 1))                                    # not exactly up_rate x the feature map
    with pytest.raises(_lib.UnicornHipError, match="exactly"):
        call(masks=torch.zeros(B, M, 2 * r * H, 2 * r * W))
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        call(r=2)                                                                          # up_masks of another rate
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        call(dp=torch.zeros(B, A, 168))
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        call(lvl=torch.zeros(B, A + 1, dtype=torch.int64))
    with pytest.raises(_lib.UnicornHipError, match="does not fit"):
        call(xs=torch.zeros(1, A + 1))
    with pytest.raises(_lib.UnicornHipError, match="integer"):
        call(lvl=lvl.float())
    with pytest.raises(_lib.UnicornHipError, match="assignment"):
        call(asg=asg[:3])
    with pytest.raises(_lib.UnicornHipError, match="capacity"):
        call(capacity=-1)
    with pytest.raises(_lib.UnicornHipError, match="capacity"):
        call(capacity=0)
