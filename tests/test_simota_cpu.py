"""CPU-side checks of the SimOTA label assignment (uni_simota_assign, ops.simota_assign / simota_assign_batch): the restatement the GPU tests
use (tests/simota_ref.py) equals, in fp32, every fixture the reference's own get_assignments produced; the fixtures hold the properties
and margins their generator promises; the new symbols are declared, exported and bound; the workspace respects the stated bound; every
argument check of the wrappers raises without a device."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import simota_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_simota_workspace_bytes": 4, "uni_simota_assign": 20}
SINGLE = sorted(t for t in R.CASES if len(R.CASES[t][2]) == 1)


def images(tag):
    """(suffix, H, W, G, C) of every image of a case that has boxes"""
    H, W, Gs, C, _ = R.CASES[tag]
    return [("" if len(Gs) == 1 else "_%d" % b, H, W, G, C) for b, G in enumerate(Gs) if G]


def restated(c, sfx, H, W, C, dtype=torch.float32):
    ins = [torch.from_numpy(c[n + sfx]).to(dtype) for n in R.INPUTS]
    return R.assign(*ins, *R.anchors(H, W, dtype=dtype), (H, W), C)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_in_fp32_equals_the_fixture(tag):
    c = R.load_case(tag)
    for sfx, H, W, G, C in images(tag):
        r = restated(c, sfx, H, W, C)
        assert r["num_fg"] == int(c["num_fg" + sfx])
        assert np.array_equal(r["fg_mask"].numpy(), c["fg_mask" + sfx]) and c["fg_mask" + sfx].dtype == np.bool_
        assert np.array_equal(r["matched_gt_inds"].numpy(), c["matched_gt_inds" + sfx]) and c["matched_gt_inds" + sfx].dtype == np.int64
        assert np.array_equal(r["gt_matched_classes"].numpy(), c["gt_matched_classes" + sfx])
        assert np.array_equal(r["pred_ious_this_matching"].numpy(), c["pred_ious_this_matching" + sfx])
        assert np.array_equal(r["iou"].numpy(), c["iou" + sfx])                      # the same operations in the same order: the same bits
        assert np.array_equal(r["cost"].numpy(), c["cost" + sfx])
        # the reference's own per-box topk loop selects the same anchors (no tie decides anything in a fixture)
        ins = [torch.from_numpy(c[n + sfx]) for n in R.INPUTS]
        assert torch.equal(R.assign(*ins, *R.anchors(H, W), (H, W), C, loop=True)["matching"], r["matching"])


def test_fixture_cases_are_the_described_ones():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(R.GOLD, "simota_*.npz"))) == sorted("simota_%s.npz" % t for t in R.CASES)
    want = {"sot": (64, 96, 126, (1,), 1), "cls4": (64, 96, 126, (5,), 4), "small": (96, 160, 315, (12,), 1), "crowd": (96, 160, 315, (70,), 1),
            "edge": (72, 104, 147, (6,), 8), "tiny": (32, 32, 21, (1,), 1), "batch": (64, 96, 126, (4, 0, 9), 2)}
    for tag, (H, W, A, Gs, C) in want.items():
        assert R.CASES[tag][:4] == (H, W, Gs, C) and R.anchors(H, W)[0].shape[0] == A
        assert os.path.getsize(os.path.join(R.GOLD, "simota_%s.npz" % tag)) < (1 << 20), "a committed file stays below 1 MiB"
        c = R.load_case(tag)
        assert tuple(c["shape"]) == (H, W, C) + Gs
        for sfx, _, _, G, _ in images(tag):
            assert c["bbox" + sfx].shape == (A, 4) and c["obj" + sfx].shape == (A, 1) and c["cls" + sfx].shape == (A, C)
            assert c["gt_bboxes" + sfx].shape == (G, 4) and c["gt_classes" + sfx].shape == (G,)
            assert all(c[n + sfx].dtype == np.float32 for n in R.INPUTS)
            assert c["cost" + sfx].shape == c["iou" + sfx].shape and c["cost" + sfx].shape[0] == G
            assert 0 <= c["gt_classes" + sfx].min() and c["gt_classes" + sfx].max() < C
    assert A % 64 != 0 and R.anchors(72, 104)[0].shape[0] % 64 != 0
    b = R.load_case("batch")
    assert b["outputs"].shape == (3, 126, 7) and b["labels"].shape == (3, R.BATCH_M, 5)
    assert ((b["labels"].sum(2) > 0).sum(1) == np.array([4, 0, 9])).all(), "the reference's nlabel counts the boxes of the padded labels"
    assert not b["labels"][1].any() and not b["labels"][0, 4:].any()
    for i in (0, 2):
        assert np.array_equal(b["outputs"][i], np.concatenate([b["bbox_%d" % i], b["obj_%d" % i], b["cls_%d" % i]], 1))
    e = R.load_case("edge")
    cx, cy = e["gt_bboxes"][:, 0], e["gt_bboxes"][:, 1]
    assert (cx < 0).any() and (cx > 104).any() and (cy < 0).any() and (cy > 72).any(), "centres beyond every side: the clip path"
    s = R.load_case("small")
    assert 4 <= s["gt_bboxes"][:, 2:].min() and s["gt_bboxes"][:, 2:].max() <= 24


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fixtures_hold_their_properties_and_margins(tag):
    c = R.load_case(tag)
    for sfx, H, W, G, C in images(tag):
        ins = [torch.from_numpy(c[n + sfx]) for n in R.INPUTS]
        m, r32, r64 = R.margins_of(*ins, *R.anchors(H, W), (H, W), C)
        assert m["ok"], m
        assert m["min_gap_ratio"] > R.MARGIN and m["ksum_margin"] > R.MARGIN * 10 * m["iou_dev"] and m["min_abs_delta"] > R.MIN_DELTA
        for n in ("cost_dev", "iou_dev", "min_gap_ratio", "ksum_margin", "min_abs_delta"):
            assert m[n] == pytest.approx(float(c["margin_" + n + sfx]), rel=1e-9), n
        assert 0 < m["iou_dev"] < 1e-5 and 0 < m["cost_dev"] < 1e-2                   # an fp32 evaluation's deviation: neither zero nor large
        assert torch.equal(r32["matching"], r64["matching"]) and torch.equal(r32["k"], r64["k"])
        contested = int(r64["contested"].sum())
        won_without_selecting = int((r64["matching"] & ~r64["selected"]).any(0).sum())
        penalised = int((r64["selected"] & (r64["cost"] >= 5e4)).any(1).sum())
        assert (contested, won_without_selecting, penalised, int(r64["cand"].sum())) == tuple(
            int(c["prop_" + n + sfx]) for n in ("contested", "won_without_selecting", "boxes_selecting_penalised", "candidates"))
        if tag == "sot":
            assert contested == 0
        if tag == "cls4":
            assert contested >= 1 and len(set(c["gt_classes"].tolist())) > 1
        if tag == "small":
            assert penalised >= 1
        if tag == "crowd":
            assert G > 64 and contested >= 30 and won_without_selecting >= 1
        if tag == "tiny":
            assert int(r64["cand"].sum()) < 10


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn_head_mask.py:754-983" in src
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


def test_workspace_respects_the_stated_bound_and_refuses_what_the_call_refuses():
    from unicorn_amd import _lib
    ws = _lib.lib().uni_simota_workspace_bytes
    for B, A, G, C in ((1, 21000, 100, 1), (8, 21000, 100, 1), (1, 21000, 64, 80), (3, 126, 12, 2), (1, 21, 1, 1), (2, 147, 0, 8), (1, 1, 1024, 256)):
        got = ws(B, A, G, C)
        assert 2 * B * G * A * 4 + B * A * (C + 1) * 4 <= got <= 3 * B * G * A * 4 + 4 * B * A * (C + 4) + 2048, (B, A, G, C, got)
    assert ws(1, 21000, 64, 80) < 21000 * 64 * 80 * 4 // 8                           # far below one (G, A, C) tensor
    for bad in ((0, 100, 1, 1), (1, 0, 1, 1), (1, 100, -1, 1), (1, 100, 1025, 1), (1, 100, 1, 0), (1, 100, 1, 257), (1, 1 << 24, 1, 1),
                (65536, 100, 1, 1)):
        assert ws(*bad) == 0, bad


def test_python_surface_rejects_bad_arguments_without_a_device():
    from unicorn_amd import ops
    A, G, C = 21, 2, 3
    box, obj, cls = torch.zeros(A, 4), torch.zeros(A, 1), torch.zeros(A, C)
    gtb, gtc = torch.ones(G, 4), torch.zeros(G)
    xs, ys, st = R.anchors(32, 32)
    one = (box, obj, cls, gtb, gtc, xs[None], ys[None], st[None], (32, 32), C)

    def bad_one(match, **kw):
        names = ("box", "obj", "cls", "gtb", "gtc", "xs", "ys", "st", "img", "C")
        args = [kw.get(n, v) for n, v in zip(names, one)]
        with pytest.raises(ValueError, match=match):
            ops.simota_assign(*args)
    bad_one("only fp32", box=box.double())
    bad_one("only fp32", cls=cls.half())
    bad_one("only fp32", gtc=gtc.long())
    bad_one("only fp32", st=st.double())
    bad_one("not a tensor", obj=None)
    bad_one("do not fit", box=torch.zeros(A, 5))
    bad_one("do not fit", cls=torch.zeros(A, C + 1))
    bad_one("do not fit", cls=torch.zeros(A + 1, C))
    bad_one("do not fit", obj=torch.zeros(A + 1, 1))
    bad_one("do not fit", gtb=torch.ones(G, 5))
    bad_one("do not fit", gtc=torch.zeros(G + 1))
    bad_one("do not fit", C=0)
    bad_one("does not fit", xs=xs[:-1])
    bad_one("does not fit", ys=torch.zeros(2, A))
    bad_one("does not fit", st=st[None, None])
    bad_one("img_size", img=32)
    bad_one("img_size", img=(0, 32))
    if not torch.cuda.is_available():
        bad_one("CPU tensor")                                       # all checks passed: the device check is the last one
        with pytest.raises(ValueError, match="CPU tensor"):
            ops.simota_assign(box, obj, cls, gtb[:0], gtc[:0], xs, ys, st, (32, 32), C)

    outputs, labels = torch.zeros(2, A, 5 + C), torch.zeros(2, 4, 5)
    batch = (outputs, labels, xs, ys, st, (32, 32), C)

    def bad_batch(match, **kw):
        names = ("outputs", "labels", "xs", "ys", "st", "img", "C")
        args = [kw.get(n, v) for n, v in zip(names, batch)]
        with pytest.raises(ValueError, match=match):
            ops.simota_assign_batch(*args)
    bad_batch("only fp32", outputs=outputs.half())
    bad_batch("only fp32", labels=labels.double())
    bad_batch("do not fit", outputs=torch.zeros(2, A, 4 + C))
    bad_batch("do not fit", outputs=torch.zeros(A, 5 + C))
    bad_batch("do not fit", labels=torch.zeros(3, 4, 5))
    bad_batch("do not fit", labels=torch.zeros(2, 4, 6))
    bad_batch("do not fit", C=C + 1)
    bad_batch("does not fit", xs=torch.zeros(1, A + 1))
    bad_batch("img_size", img=None)
    bad_batch("empty batch", outputs=torch.zeros(0, A, 5 + C), labels=torch.zeros(0, 4, 5))
    if not torch.cuda.is_available():
        bad_batch("CPU tensor")
