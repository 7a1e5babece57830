"""CPU-side checks of the fused detection-head loss (uni_head_loss_fwd / _bwd, ops.HeadLossFunction / head_det_loss): the restatement the
GPU tests use (tests/head_loss_ref.py) equals every fixture that the reference's own get_losses produced -- within 1e-12 of scale in fp64
and within 4 x max(the reference's own fp32-vs-fp64 deviation, one fp32 ulp) in fp32; the fixtures are the described ones; the workspace
size follows the documented formula and is 0 just outside every limit; every argument check of head_det_loss raises without a device."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import head_loss_ref as R
import simota_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_head_loss_workspace_bytes": 3, "uni_head_loss_fwd": 22, "uni_head_loss_bwd": 25, "uni_head_loss_fwd_f64": 22,
               "uni_head_loss_bwd_f64": 25}


def restated(c, tag, dtype):
    H, W, _ = (int(v) for v in c["shape"])
    xs, ys, st = S.anchors(H, W)
    origin = torch.from_numpy(c["origin_preds"]) if bool(c["use_l1"]) else None
    iou = torch.from_numpy(c["matched_ious" if dtype == torch.float64 else "matched_ious_fp32"])
    return R.run(torch.from_numpy(c["outputs"]), origin, torch.from_numpy(c["labels"]), torch.from_numpy(c["fg_mask"]),
                 torch.from_numpy(c["matched_gt_inds"]), iou, xs, ys, st, c["grad_out"], dtype)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_matches_the_fixture_in_fp64_and_fp32(tag):
    c = R.load_case(tag)
    r64, r32 = restated(c, tag, torch.float64), restated(c, tag, torch.float32)
    for k in R.QUANTITIES:
        if k not in c:
            assert k == "grad_origin" and not bool(c["use_l1"]) and r64[k] is None
            continue
        e64, e32, bound = R.rel_err(r64[k], c[k]), R.rel_err(r32[k], c[k]), R.bound32(c[k + "_fp32_ref_err"])
        print("%-12s fp64 %.3g (1e-12)   fp32 %.3g (%.3g)" % (k, e64, e32, bound))
        assert e64 <= 1e-12, (k, e64)
        assert e32 <= bound, (k, e32, bound)
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64


def test_fixture_cases_are_the_described_ones():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(R.GOLD, "head_loss_*.npz"))) == sorted("head_loss_%s.npz" % t for t in R.CASES)
    assert sorted(R.CASES) == ["batch", "batch_nol1", "cls4", "edge", "empty", "small", "sot", "tiny"]
    for tag, (src, use_l1, zero) in R.CASES.items():
        path = os.path.join(R.GOLD, "head_loss_%s.npz" % tag)
        assert os.path.getsize(path) < (1 << 20), "a committed file stays below 1 MiB"
        c = R.load_case(tag)
        outputs, labels, (H, W, C) = R.problem(tag)
        assert np.array_equal(c["outputs"], outputs.numpy()) and np.array_equal(c["labels"], labels.numpy()) and tuple(c["shape"]) == (H, W, C)
        B, A = outputs.shape[:2]
        assert bool(c["use_l1"]) == use_l1 and ("origin_preds" in c) == use_l1 and ("grad_origin" in c) == use_l1
        assert c["fg_mask"].shape == (B, A) and c["fg_mask"].dtype == np.bool_ and c["matched_gt_inds"].dtype == np.int64
        assert np.array_equal(c["fg_mask"].sum(1), c["num_fg_per_image"]) and ((c["matched_gt_inds"] >= 0) == c["fg_mask"]).all()
        assert c["grad_outputs"].shape == (B, A, 5 + C) and c["grad_outputs"].dtype == np.float64 and c["grad_outputs_fp32"].dtype == np.float32
        assert len(set(c["grad_out"].tolist())) == 4 and tuple(c["grad_out"]) == R.GRAD_OUT
        assert min(float(c["kink_edge"]), float(c["kink_span"])) > 1e-6 and (not use_l1 or float(c["kink_l1"]) > 1e-6)
        if not zero and src != "batch":                            # the assignment of the reference's get_losses is the simota fixture's
            s = S.load_case(src)
            assert np.array_equal(c["fg_mask"][0], s["fg_mask"]) and np.array_equal(c["matched_gt_inds"][0][c["fg_mask"][0]], s["matched_gt_inds"])
        for k in R.QUANTITIES[:5]:
            assert c[k].shape == () and 0 <= float(c[k + "_fp32_ref_err"]) < 1e-5
    assert {t: int(R.load_case(t)["prop_disjoint"]) for t in ("cls4", "small", "edge")} == {"cls4": 9, "small": 11, "edge": 5}
    e = R.load_case("empty")
    assert not e["labels"].any() and not e["fg_mask"].any() and float(e["num_fg"]) == 1.0 and float(e["iou_loss"]) == 0.0
    assert not e["grad_outputs"][:, :, :4].any() and not e["grad_outputs"][:, :, 5:].any() and not e["grad_origin"].any()
    n = R.load_case("batch_nol1")
    assert float(n["l1_loss"]) == 0.0 and float(n["l1_loss_fp32"]) == 0.0


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn_head_mask.py:646-745" in src and "losses.py:15-36" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s, arity in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, code)
        assert m, "%s is not declared in include/unicorn_hip.h" % s
        assert len(m.group(1).split(",")) == arity, (s, m.group(1))
        assert s in _lib.PROTOS and len(_lib.PROTOS[s][1]) == arity, s
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)


def test_workspace_equals_the_documented_formula_and_is_zero_outside_the_limits():
    from unicorn_amd import _lib
    ws = _lib.lib().uni_head_loss_workspace_bytes
    for B, A, C in ((1, 21000, 1), (8, 21000, 80), (3, 126, 2), (1, 21, 1), (1, 1, 256), (65535, 1, 1), (1, (1 << 24) - 1, 1), (2, 256, 3),
                    (2, 257, 3)):
        want = -(-(B * -(-A // 256) * 32) // 256) * 256               # B ceil(A / 256) x 4 doubles, rounded up to 256 bytes
        assert ws(B, A, C) == want > 0, (B, A, C, ws(B, A, C), want)
    for bad in ((0, 100, 1), (65536, 100, 1), (1, 0, 1), (1, 1 << 24, 1), (1, 100, 0), (1, 100, 257), (-1, 100, 1), (1, -1, 1)):
        assert ws(*bad) == 0, bad


def test_head_det_loss_rejects_bad_arguments_without_a_device():
    from unicorn_amd import ops
    A, M, C = 21, 4, 3
    xs, ys, st = S.anchors(32, 32)
    good = {"outputs": torch.zeros(2, A, 5 + C), "origin": torch.zeros(2, A, 4), "labels": torch.zeros(2, M, 5), "xs": xs, "ys": ys[None], "st": st,
            "img": (32, 32), "C": C}

    def bad(match, assignment=None, **kw):
        a = dict(good, **kw)
        with pytest.raises(ValueError, match=match):
            ops.head_det_loss(a["outputs"], a["origin"], a["labels"], a["xs"], a["ys"], a["st"], a["img"], a["C"], assignment=assignment)
    bad("fp16", outputs=good["outputs"].half())
    bad("bf16", origin=good["origin"].bfloat16())
    bad("only fp32", labels=good["labels"].double())
    bad("only fp32", st=st.double())
    bad("not a tensor", outputs=None)
    bad("not a tensor", origin=[good["origin"], None])
    bad("do not fit", outputs=torch.zeros(2, A, 4 + C))
    bad("do not fit", outputs=torch.zeros(A, 5 + C))
    bad("do not fit", labels=torch.zeros(3, M, 5))
    bad("do not fit", labels=torch.zeros(2, M, 6))
    bad("do not fit", C=C + 1)
    bad("do not fit", origin=torch.zeros(2, A + 1, 4))
    bad("do not fit", origin=torch.zeros(2, A, 5))
    bad("do not fit", origin=[torch.zeros(2, 16, 4), torch.zeros(2, 4, 4)])        # 20 anchors in all
    bad("does not fit", origin=[torch.zeros(2, 16, 4), torch.zeros(2, 5, 3)])
    bad("does not fit", xs=xs[:-1])
    bad("img_size", img=None)
    bad("empty batch", outputs=torch.zeros(0, A, 5 + C), labels=torch.zeros(0, M, 5), origin=None)
    bad("assignment", assignment=(torch.zeros(2, A),) * 3)
    bad("assignment", assignment=(torch.zeros(2, A, dtype=torch.bool), torch.zeros(2, A, dtype=torch.int64), torch.zeros(2, A + 1), torch.zeros(2)))
    if not torch.cuda.is_available():
        bad("CPU tensor")                                           # all checks passed: the device check is the last one
        bad("CPU tensor", origin=None)
        bad("CPU tensor", origin=[torch.zeros(2, 16, 4), torch.zeros(2, 5, 4)])
