"""CPU-side checks of the head-output assembly (uni_head_assemble_fwd / _bwd, ops.HeadAssembleFunction / head_assemble): the restatement the
GPU tests use (tests/head_assemble_ref.py) equals every fixture that the reference's own lines produced -- within 1e-12 of scale in fp64, bit
for bit in fp32; the fixtures are the described ones; the header declares the four entries and _lib.py binds them; the anchor tile the
shapes are chosen around is the kernel's; every argument check of head_assemble raises without a device."""
import glob
import os
import re

import numpy as np
import pytest
import torch

import head_assemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_head_assemble_fwd": 23, "uni_head_assemble_bwd": 20, "uni_head_assemble_fwd_f64": 23, "uni_head_assemble_bwd_f64": 20}


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_matches_the_fixture_in_fp64_and_fp32(tag):
    c, p = R.load_case(tag), R.problem(tag)
    r64, r32 = R.run(p, torch.float64), R.run(p, torch.float32)
    names, wide = R.stored_names(p)
    for k in names:
        e64 = R.rel_err(r64[k], c[k])
        print("%-18s fp64 %.3g (1e-12)   fp32 bits %s" % (k, e64, R.bits_equal(r32[k], c[k + "_fp32"])))
        assert e64 <= 1e-12, (k, e64)
        assert r64[k].dtype == torch.float64 and R.bits_equal(r32[k], c[k + "_fp32"]), k
    for k in wide:
        assert R.bits_equal(r32[k], c[k + "_fp32"]) and torch.equal(r64[k].double(), torch.from_numpy(c[k + "_fp32"]).double()), k


def test_fixture_cases_are_the_described_ones():
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(R.GOLD, "head_assemble_*.npz"))) == sorted(
        "head_assemble_%s.npz" % t for t in R.CASES)
    assert sorted(R.CASES) == ["c80", "cls8", "edge", "one", "small"]
    want = {"small": (2, 1, ((8, 12), (4, 6), (2, 3)), 169), "cls8": (3, 8, ((7, 9), (3, 5), (1, 2)), 0), "one": (1, 1, ((1, 1),), 0),
            "edge": (1, 1, ((5, 13), (1, 1)), 169), "c80": (2, 80, ((5, 13), (2, 3)), 0)}
    for tag, (B, C, levels, P, seed) in R.CASES.items():
        assert (B, C, levels, P) == want[tag]
        path = os.path.join(R.GOLD, "head_assemble_%s.npz" % tag)
        assert os.path.getsize(path) < 256 * 1024, "a fixture stays below 256 KB"
        c, p = R.load_case(tag), R.problem(tag)
        A = sum(h * w for h, w in levels)
        assert tuple(c["shape"]) == (B, C, P, A) and int(c["seed"]) == seed and tuple(map(tuple, c["levels"])) == levels
        assert tuple(c["strides"]) == R.STRIDES[:len(levels)]
        for m in R.MAPS[:3]:
            for k in range(len(levels)):
                assert np.array_equal(c["%s_%d" % (m, k)], p[m][k].numpy()), (m, k)
        assert c["outputs"].shape == (B, A, 5 + C) and c["outputs"].dtype == np.float64 and c["outputs_fp32"].dtype == np.float32
        assert c["origin_preds"].shape == (B, A, 4) and c["x_shifts"].shape == (1, A) and c["expanded_strides"].shape == (1, A)
        assert ("dynamic_params_fp32" in c) == (P > 0) == ("fpn_levels_fp32" in c) == ("grad_ctrl_0_fp32" in c)
        if P:
            assert c["dynamic_params_fp32"].shape == (B, A, P) and c["fpn_levels_fp32"].shape == (B, A)
        # exact in fp32: everything but the decoded box columns and the gradient of reg
        for k in ("origin_preds", "x_shifts", "y_shifts", "expanded_strides") + tuple("grad_%s_%d" % (m, l) for m in ("obj", "cls")
                                                                                       for l in range(len(levels))):
            assert float(c[k + "_fp32_ref_err"]) == 0.0, k
        assert 0 < float(c["outputs_exp_fp32_ref_err"]) < 2e-7 and all(0 < float(c["grad_reg_%d_exp_fp32_ref_err" % l]) < 2e-7
                                                                         for l in range(len(levels)))
        g = p["g_outputs"]
        assert len(set(g[0, 0, :5].tolist())) == 5, "unequal gradient weights, so that a swapped column shows"
    assert 80 % R.TILE and sum(h * w for h, w in R.CASES["cls8"][2]) == 80                     # ragged against the tile
    assert R.CASES["edge"][2][0][0] * R.CASES["edge"][2][0][1] == R.TILE + 1 == R.CASES["c80"][2][0][0] * R.CASES["c80"][2][0][1]


def test_the_tile_of_the_shapes_is_the_kernels():
    from unicorn_amd import ops
    src = open(os.path.join(ROOT, "unicorn_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr int HA_TILE = (\d+);", src)
    assert m and int(m.group(1)) == R.TILE == ops.HEAD_ASSEMBLE_TILE
    m = re.search(r"constexpr int HA_MAX_L = (\d+);", src)
    assert m and int(m.group(1)) == ops.HEAD_ASSEMBLE_MAX_LEVELS == 4
    assert "head_assemble" in open(os.path.join(ROOT, "unicorn_amd", "csrc", "build.sh")).read()


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn_head_mask.py:339-366" in src and ":476-500" in src and ":396-401" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s, arity in NEW_SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % s, code)
        assert m, "%s is not declared in include/unicorn_hip.h" % s
        assert len(m.group(1).split(",")) == arity, (s, m.group(1))
        assert s in _lib.PROTOS and len(_lib.PROTOS[s][1]) == arity, s
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)


def test_head_assemble_rejects_bad_arguments_without_a_device():
    from unicorn_amd import _lib, ops
    B, C, P = 2, 3, 5
    levels = ((4, 6), (2, 3))

    def maps(nc, dtype=torch.float32):
        return [torch.zeros(B, nc, h, w, dtype=dtype) for h, w in levels]
    good = {"reg": maps(4), "obj": maps(1), "cls": maps(C), "strides": (8, 16), "ctrl": maps(P)}

    def bad(match, **kw):
        a = dict(good, **kw)
        with pytest.raises(_lib.UnicornHipError, match=match):
            ops.head_assemble(a["reg"], a["obj"], a["cls"], a["strides"], a["ctrl"])
    bad("not a list", reg=good["reg"][0])
    bad("not a tensor", obj=[good["obj"][0], None])
    bad("not a tensor", ctrl=[None, None])
    bad("levels", reg=[], obj=[], cls=[], ctrl=[], strides=())
    bad("levels", reg=maps(4) * 3, obj=maps(1) * 3, cls=maps(C) * 3, ctrl=maps(P) * 3, strides=(8,) * 6)      # L = 6
    bad("levels", obj=good["obj"][:1])
    bad("levels", ctrl=good["ctrl"][:1])
    bad("positive numbers", strides=(8,))
    bad("positive numbers", strides=(8, 0))
    bad("positive numbers", strides=(8, -16))
    bad("positive numbers", strides=(8, float("inf")))
    bad("positive numbers", strides=(8, float("nan")))
    bad("numbers", strides=(8, "x"))
    bad("numbers", strides=None)
    bad(r"is not \(N, C, H, W\)", reg=[good["reg"][0], torch.zeros(B, 4, 6)])
    bad("level's size", reg=[good["reg"][0], torch.zeros(B, 5, 2, 3)])
    bad("level's size", obj=[good["obj"][0], torch.zeros(B, 2, 2, 3)])
    bad("level's size", cls=[good["cls"][0], torch.zeros(B, C + 1, 2, 3)])
    bad("level's size", cls=[good["cls"][0], torch.zeros(B, C, 3, 2)])
    bad("level's size", ctrl=[good["ctrl"][0], torch.zeros(B + 1, P, 2, 3)])
    bad("outside", cls=maps(0))
    bad("outside", cls=maps(257))
    bad("outside", ctrl=maps(1025))
    bad("outside", reg=[torch.zeros(0, 4, 4, 6), torch.zeros(0, 4, 2, 3)], obj=[torch.zeros(0, 1, 4, 6), torch.zeros(0, 1, 2, 3)],
        cls=[torch.zeros(0, C, 4, 6), torch.zeros(0, C, 2, 3)], ctrl=None)
    bad("outside", reg=[good["reg"][0], torch.zeros(B, 4, 0, 3)], obj=[good["obj"][0], torch.zeros(B, 1, 0, 3)],
        cls=[good["cls"][0], torch.zeros(B, C, 0, 3)], ctrl=None)
    bad("dtypes", cls=maps(C, torch.float16))
    bad("dtypes", reg=maps(4, torch.float64))
    bad("dtypes", reg=maps(4, torch.int32), obj=maps(1, torch.int32), cls=maps(C, torch.int32), ctrl=maps(P, torch.int32))
    if not torch.cuda.is_available():
        bad("CPU tensor")                                           # all checks passed: the device check is the last one
        bad("CPU tensor", ctrl=None)
        bad("CPU tensor", reg=maps(4, torch.bfloat16), obj=maps(1, torch.bfloat16), cls=maps(C, torch.bfloat16), ctrl=maps(P, torch.bfloat16))
