"""CPU-side checks of the fused CondInst mask loss (uni_condinst_loss_fwd / _bwd, ops.condinst_dice_loss): the formulas the kernels implement
(tests/condinst_loss_ref.py) equal the fixtures the reference's own functions produced; the fixtures are what their generator says; the
new symbols are declared, exported and bound; the Python surface exists and fails the library's way without a device."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import condinst_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_condinst_loss_workspace_bytes": 4, "uni_condinst_loss_fwd": 16, "uni_condinst_loss_bwd": 19,
               "uni_condinst_loss_fwd_f64": 16, "uni_condinst_loss_bwd_f64": 19}


def fixture_tensors(c, dtype):
    return [torch.from_numpy(c[n]).to(dtype) for n in ("mask_feats", "up_masks", "params", "inst_loc")] + \
           [torch.from_numpy(c["inst_lvl"]), torch.from_numpy(c["gt"]).to(dtype)]


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_equals_the_fixture(tag):
    c = R.load_case(tag)
    r = R.CASES[tag][2]
    got = R.loss_and_grads(*fixture_tensors(c, torch.float64), r, torch.from_numpy(c["grad_loss"]).double())
    for n in R.OUTPUTS:
        ref = torch.from_numpy(c[n])
        assert ref.dtype == torch.float64 and got[n].shape == ref.shape, n
        err = float((got[n] - ref).abs().max() / ref.abs().max())
        assert err <= 1e-12, (tag, n, err)
    chunked = R.loss_and_grads(*fixture_tensors(c, torch.float64), r, torch.from_numpy(c["grad_loss"]).double(), chunk=2)
    for n in R.OUTPUTS:
        assert float((chunked[n] - got[n]).abs().max()) <= 1e-13 * float(got[n].abs().max()), (tag, n)


def test_fixture_cases_are_the_described_ones():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(R.GOLD, "condinst_loss_*.npz"))) == \
        sorted("condinst_loss_%s.npz" % t for t in R.CASES)
    assert R.CASES["flat"] == (12, 20, 4, 5) and R.CASES["ragged"] == (7, 13, 4, 3) and R.CASES["r2"][2] == 2 and R.CASES["r8"][2] == 8
    for tag, (H, W, r, n) in R.CASES.items():
        path = os.path.join(R.GOLD, "condinst_loss_%s.npz" % tag)
        assert os.path.getsize(path) < (1 << 20), "a committed file stays below 1 MiB"
        c = R.load_case(tag)
        assert tuple(c["shape"]) == (H, W, r, n)
        assert c["mask_feats"].shape == (1, 8, H, W) and c["up_masks"].shape == (1, 9 * r * r, H, W) and c["params"].shape == (n, 169)
        assert c["inst_loc"].shape == (n, 2) and c["inst_lvl"].shape == (n,) and c["gt"].shape == (n, 1, r * H, r * W)
        assert c["grad_loss"].shape == (n,) and c["loss"].shape == (n,)
        assert all(c[k].dtype == np.float32 for k in R.INPUTS) and c["inst_lvl"].dtype == np.int32
        assert set(np.unique(c["gt"])) <= {0.0, 1.0} and 0 <= c["inst_lvl"].min() and c["inst_lvl"].max() <= 4
        for k in R.OUTPUTS:
            e = float(c[k + "_fp32_ref_err"])
            assert 1e-9 < e < 1e-5, (tag, k, e)                    # an fp32 evaluation's error: neither zero nor large
            assert float(np.abs(c[k]).max()) > 1e-4, (tag, k)       # no comparison divides by something degenerate
        # no input sits on a ReLU kink: fp32 and fp64 take the same branches
        mf, um, p, loc, lvl, gt = fixture_tensors(c, torch.float64)
        _, p0, p1 = R.pre_activations(mf, p, loc, lvl)
        kink = min(float(p0.abs().min()), float(p1.abs().min()))
        assert kink > 1e-6 and abs(kink - float(c["min_abs_pre_activation"])) <= 1e-12
        _, q0, q1 = R.pre_activations(mf.float(), p.float(), loc.float(), lvl)
        assert torch.equal(q0 > 0, p0 > 0) and torch.equal(q1 > 0, p1 > 0)
    e = R.load_case("edge")
    H, W = R.CASES["edge"][:2]
    assert sorted(map(tuple, e["inst_loc"][:4].tolist())) == sorted([(0., 0.), (8 * W - 1., 0.), (0., 8 * H - 1.), (8 * W - 1., 8 * H - 1.)])
    assert set(e["inst_lvl"].tolist()) == {0, 1, 2}
    assert not e["gt"][4].any() and e["gt"][:4].any()                                   # one all-zero ground truth
    assert float(np.abs(e["params"][5]).max()) > 20 * float(np.abs(e["params"][0]).max()) / 4      # one instance scaled into saturation
    mf, um, p, loc, lvl, gt = fixture_tensors(e, torch.float64)
    logits, p0, _ = R.pre_activations(mf, p, loc, lvl)
    assert float(logits[5].abs().median()) > 30                                         # ... its sigmoid saturates
    assert float((p0[3] <= 0).double().mean()) > 0.85                                   # ReLUs mostly dead in one instance


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "dynamic_mask_head.py:247-278" in src
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
    # host-side part that needs no device: the workspace is O(n H8 W8), far below one (n, r H8, r W8) map per instance
    n, H8, W8, r = 128, 100, 160, 4
    ws = lib.uni_condinst_loss_workspace_bytes(n, H8, W8, r)
    assert 2 * n * H8 * W8 * 4 <= ws < n * H8 * W8 * r * r * 4 // 2
    assert lib.uni_condinst_loss_workspace_bytes(0, H8, W8, r) == 0
    assert lib.uni_condinst_loss_workspace_bytes(1, 1, 1, 4) > 0


def test_python_surface_rejects_cpu_tensors_bad_shapes_and_mixed_dtypes():
    from unicorn_amd import _lib, ops
    assert issubclass(ops.CondInstDiceFunction, torch.autograd.Function)
    H, W, r, n = 3, 5, 4, 2
    mf, um, p = torch.zeros(1, 8, H, W), torch.zeros(1, 9 * r * r, H, W), torch.zeros(n, 169)
    loc, lvl, gt = torch.zeros(n, 2), torch.zeros(n, dtype=torch.int64), torch.zeros(n, 1, r * H, r * W)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.UnicornHipError, match="HIP device tensors"):
            ops.condinst_dice_loss(mf, um, p, loc, lvl, gt, r)
        with pytest.raises(_lib.UnicornHipError, match="HIP device tensors"):
            ops.condinst_dice_loss(mf.double(), um.double(), p.double(), loc.double(), lvl, gt[:, 0].double(), r)
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.condinst_dice_loss(mf, um, p, loc, lvl, torch.zeros(n, 1, r * H, r * W + 1), r)        # not exactly up_rate x the feature map
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.condinst_dice_loss(mf, um, p, loc, lvl, torch.zeros(n, 1, 2 * r * H, 2 * r * W), r)    # the reference's 1/4-resolution maps of another rate
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.condinst_dice_loss(mf, um, p, loc, lvl, gt, 2)                                         # up_masks of another rate
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.condinst_dice_loss(mf, um, torch.zeros(n, 168), loc, lvl, gt, r)
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.condinst_dice_loss(mf, um, p, torch.zeros(n + 1, 2), lvl, gt, r)
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.condinst_dice_loss(torch.zeros(2, 8, H, W), um, p, loc, lvl, gt, r)                    # one image per call
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        ops.condinst_dice_loss(mf, um.double(), p, loc, lvl, gt, r)
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        ops.condinst_dice_loss(mf, um, p, loc, lvl, gt.bool(), r)
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        ops.condinst_dice_loss(mf.half(), um.half(), p.half(), loc.half(), lvl, gt.half(), r)
    with pytest.raises(_lib.UnicornHipError, match="integer"):
        ops.condinst_dice_loss(mf, um, p, loc, lvl.float(), gt, r)
