"""CPU side of the fused MOT instance-contrastive loss (uni_mot_corr_loss_fwd / _bwd, ops.mot_corr_loss): the two torch restatements of
tests/mot_corr_ref.py reproduce the fixtures that the reference's own compute_loss_mot_corr produced (tests/golden/mot_corr_*.npz) to
1e-12 of scale in fp64, NaN positions included; the fixtures keep their rule, show what each case is there for and stay small; the C-ABI
symbols are declared, bound and exported; the Python surface refuses bad arguments before it touches the library."""
import os
import re

import numpy as np
import pytest
import torch

import mot_corr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_mot_corr_workspace_bytes": 3, "uni_mot_corr_loss_fwd": 16, "uni_mot_corr_loss_bwd": 20, "uni_mot_corr_loss_fwd_f64": 16,
               "uni_mot_corr_loss_bwd_f64": 20}


def inputs(c, dtype):
    return (torch.from_numpy(c["embed_0"]).to(dtype), torch.from_numpy(c["embed_1"]).to(dtype), torch.from_numpy(c["targets"]),
            torch.from_numpy(c["grad_loss"]))


@pytest.fixture(scope="module")
def cases():
    return {tag: R.load_case(tag) for tag in R.CASES}


@pytest.mark.parametrize("form", ["loop", "vectorised"])
@pytest.mark.parametrize("tag", list(R.CASES))
def test_restatement_reproduces_the_fixture_in_fp64(cases, tag, form):
    c = cases[tag]
    bidirect, grid_sample = R.CASES[tag][5:7]
    assert (bool(c["bidirect"]), bool(c["grid_sample"])) == (bidirect, grid_sample) and tuple(c["shape"]) == R.CASES[tag][:5]
    got = R.loss_and_grads(R.loss_loop if form == "loop" else R.loss_vectorised, *inputs(c, torch.float64), bidirect, grid_sample)
    for k in R.RESULTS:
        ref = torch.from_numpy(c[k])
        assert ref.dtype == torch.float64 and got[k].dtype == torch.float64
        fin = torch.isfinite(ref)
        assert torch.equal(fin, torch.isfinite(got[k])), (tag, k, "NaN positions differ")
        err = float((got[k] - ref)[fin].abs().max() / ref[fin].abs().max())
        assert err <= 1e-12, (tag, form, k, err)


def test_fixtures_keep_their_rule_and_show_their_property(cases):
    for tag, c in cases.items():
        B, C, H, W, M, _, grid_sample, kind = R.CASES[tag]
        t = torch.from_numpy(c["targets"])
        assert all(c[k].dtype == np.float32 for k in ("embed_0", "embed_1", "targets", "grad_loss"))
        assert c["embed_0"].shape == c["embed_1"].shape == (B, C, H, W) and t.shape == (B, 2, M, 6)
        assert R.rule_violations(t, H, W, grid_sample) == [], tag
        assert R.has_property(tag, t, H, W), tag
        for k in R.RESULTS:
            e = float(c[k + "_fp32_ref_err"])
            assert R.REF_ERR_MIN < e < R.REF_ERR_MAX, (tag, k, e)                # an fp32 evaluation's error: no rounding accident, not large
            assert float(np.nanmax(np.abs(c[k]))) > 1e-3, (tag, k)                  # no comparison divides by something degenerate
        redrawn = R.draw(kind, int(c["seed"]))                                      # the stored inputs are the seeded draw
        for k, v in zip(("embed_0", "embed_1", "targets", "grad_loss"), redrawn):
            assert np.array_equal(c[k], v.numpy()), (tag, k)
    for k in ("embed_0", "embed_1", "targets", "grad_loss"):
        assert np.array_equal(cases["unidir"][k], cases["plain"][k])
    nm = cases["nomatch"]
    assert np.isnan(nm["loss"]).tolist() == [False, True, False]
    assert not nm["g_embed_0"][1].any() and not nm["g_embed_1"][1].any() and nm["g_embed_0"][0].any() and nm["g_embed_1"][2].any()
    # `edge`: the labels the reference's overwrite order gives (5 is repeated in frame 0, 9 in frame 1, row 2 of frame 0 has id 0)
    ids = torch.from_numpy(cases["edge"]["targets"])[0, :, :, 5]
    row, col = R.labels_vectorised(ids[0, :6], ids[1, :5])
    assert row.tolist() == [1, 0, -1, 0, -1, 2] and col.tolist() == [3, 0, 5, -1, -1]


def test_fixture_files_are_small():
    total = 0
    for tag in R.CASES:
        size = os.path.getsize(os.path.join(R.GOLDEN, "mot_corr_%s.npz" % tag))
        assert size < 1 << 20, (tag, size)
        total += size
    assert total < 3 << 19
    src = open(os.path.join(R.GOLDEN, "make_golden_mot_corr.py")).read()
    assert "compute_loss_mot_corr" in src and "ref_bootstrap" in src


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn.py:407-466" in src
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


def test_workspace_size_and_refused_shapes():
    from unicorn_amd import _lib
    ws = _lib.lib().uni_mot_corr_workspace_bytes
    for B, M, C in ((1, 100, 128), (8, 100, 128), (1, 10, 24), (3, 6, 16), (1, 1, 1), (2, 1024, 1024)):
        got = ws(B, M, C)
        assert 4 * B * M * (4 * C + M) <= got <= 4 * B * M * (4 * C + M + 16) + 9 * 256, (B, M, C, got)       # O(B M (C + M))
    for bad in ((0, 10, 8), (65536, 10, 8), (1, 0, 8), (1, 1025, 8), (1, 10, 0), (1, 10, 1025)):
        assert ws(*bad) == 0, bad


def test_python_surface_rejects_bad_arguments_before_any_library_call(monkeypatch):
    from unicorn_amd import _lib, ops

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    e, t = torch.zeros(2, 8, 4, 6), torch.zeros(2, 2, 5, 6)

    def bad(match, e0=e, e1=e, tg=t, **kw):
        with pytest.raises(_lib.UnicornHipError, match=match):
            ops.mot_corr_loss(e0, e1, tg, **kw)
    bad("do not fit", e0=e[0])
    bad("do not fit", e1=torch.zeros(2, 8, 4, 5))
    bad("do not fit", tg=torch.zeros(2, 2, 5, 5))
    bad("do not fit", tg=torch.zeros(2, 3, 5, 6))
    bad("do not fit", tg=torch.zeros(3, 2, 5, 6))
    bad("do not fit", tg=torch.zeros(2, 5, 6))
    bad("not a tensor", tg=None)
    bad("no fp16", e0=e.half(), e1=e.half())
    bad("no fp16", e0=e.bfloat16(), e1=e.bfloat16())
    bad("unsupported", e1=e.double())                                               # mixed dtypes
    bad("CPU tensor")                                                               # every other check passed: the device check is the last
    bad("CPU tensor", e0=e.double(), e1=e.double(), tg=t.half())                    # targets of any dtype: they are converted with .float()
