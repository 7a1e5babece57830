"""CPU side of the SOT / VOS label-propagation losses (uni_prop_labels, uni_prop_dice_pyramid_fwd / _bwd, ops.sot_prop_loss /
vos_prop_loss): the torch restatement of tests/prop_loss_ref.py reproduces the fixtures that the reference's own compute_loss_sot /
compute_loss_vos produced (tests/golden/prop_loss_*.npz) to 1e-12 of scale in fp64, labels and match table exactly; the fixtures keep
their rules, show what each case is there for and stay small; the C-ABI symbols are declared, bound and exported; the Python surface
refuses bad arguments before it touches the library."""
import os
import re

import numpy as np
import pytest
import torch

import prop_loss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"uni_prop_workspace_bytes": 3, "uni_prop_labels": 15, "uni_prop_labels_f64": 15, "uni_prop_dice_pyramid_fwd": 14,
               "uni_prop_dice_pyramid_fwd_f64": 14, "uni_prop_dice_pyramid_bwd": 14, "uni_prop_dice_pyramid_bwd_f64": 14}


@pytest.fixture(scope="module")
def cases():
    return {tag: R.load_case(tag) for tag in R.CASES}


def restated(tag, c, dtype):
    kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
    t = {k: torch.from_numpy(c[k]) for k in R.INPUTS}
    masks = torch.from_numpy(c["masks"]) if r else None
    return R.loss_and_grads(kind, t["embed_0"].to(dtype), t["embed_1"].to(dtype), t["targets"], (8 * H8, 8 * W8), t["w8"], t["w16"], t["w32"],
                            masks, max_inst)


@pytest.mark.parametrize("tag", list(R.CASES))
def test_restatement_reproduces_the_fixture_in_fp64(cases, tag):
    c = cases[tag]
    got = restated(tag, c, torch.float64)
    for k in R.EXACT_RESULTS:
        assert np.array_equal(got[k].cpu().numpy().astype(c[k].dtype), c[k]), (tag, k)
    for k in R.FLOAT_RESULTS:
        ref = torch.from_numpy(c[k])
        assert ref.dtype == torch.float64 and got[k].dtype == torch.float64 and got[k].shape == ref.shape, (tag, k)
        err = float((got[k] - ref).abs().max() / ref.abs().max())
        assert err <= 1e-12, (tag, k, err)


def test_fixtures_keep_their_rules_and_show_their_property(cases):
    for tag, c in cases.items():
        kind, B, H8, W8, M, nz, max_inst, r, mdt = R.CASES[tag]
        Kc = R.case_kc(tag)
        ins = R.draw(tag, int(c["seed"]))                                          # the stored inputs are the seeded draw
        for k, v in ins.items():
            assert np.array_equal(c[k], v.numpy()) and c[k].dtype == v.numpy().dtype, (tag, k)
        assert c["embed_0"].shape == (B, 128, H8, W8) and c["targets"].shape == (B, 2, M, 6) and c["p8"].shape == (B, Kc, H8, W8)
        assert c["p16"].shape == (B, Kc, H8 // 2, W8 // 2) and c["p32"].shape == (B, Kc, H8 // 4, W8 // 4)
        assert c["matched"].shape == (B, Kc, 2) and c["matched"].dtype == np.int32 and c["num_matched"].dtype == np.int32
        assert R.rule_violations(ins["targets"]) == [], tag
        assert R.has_property(tag, ins), tag
        for e in ("embed_0", "embed_1"):
            assert int((np.abs(c[e]).sum(axis=(0, 2, 3)) > 0).sum()) == nz, (tag, e)
        for k in R.FLOAT_RESULTS:
            e = float(c[k + "_fp32_ref_err"])
            assert R.REF_ERR_MIN < e < R.REF_ERR_MAX, (tag, k, e)
            assert float(np.abs(c[k]).max()) > 1e-3, (tag, k)
        # empty slots: -1, zero loss, zero priors; a sample without a match has an exactly zero gradient
        for b in range(B):
            n = int(c["num_matched"][b])
            assert (c["matched"][b, n:] == -1).all() and (c["matched"][b, :n] >= 0).all()
            assert not c["corr_loss"].reshape(B, -1)[b, n:].any() if kind == "vos" else True
            assert not c["p8"][b, n:].any() and not c["gt0"][b, n:].any() and not c["gt1"][b, n:].any()
    vb = cases["vos_box"]
    assert vb["num_matched"].tolist() == [4, 0] and not vb["g_embed_0"][1].any() and not vb["g_embed_1"][1].any() and vb["g_embed_0"][0].any()
    # the ragged shapes the kernels need: odd H8, W8 no multiple of 4, H8 W8 no multiple of 4
    assert R.CASES["sot_ragged"][2] % 2 == 1 and R.CASES["sot_ragged"][3] % 4 == 2 and (R.CASES["vos_mask_r4"][2] * R.CASES["vos_mask_r4"][3]) % 4 == 2


def test_label_restatement_follows_python_slicing():
    H, W = 72, 112
    rows = torch.tensor([R.EDGE_BOXES[k] for k in sorted(R.EDGE_BOXES)])
    full = torch.zeros(len(rows), H, W)
    c = torch.round(torch.stack([rows[:, 0] - 0.5 * rows[:, 2], rows[:, 1] - 0.5 * rows[:, 3], rows[:, 0] + 0.5 * rows[:, 2],
                                 rows[:, 1] + 0.5 * rows[:, 3]], -1)).int().tolist()
    for n, (x1, y1, x2, y2) in enumerate(c):
        full[n, max(0, y1):y2, max(0, x1):x2] = 1.0
    exp = torch.nn.functional.interpolate(full[:, None], scale_factor=1 / 8, mode="bilinear", align_corners=False).flatten(-2)[:, 0]
    assert torch.equal(R.labels_from_boxes(rows, H, W, torch.float32, "cpu"), exp)


def test_fixture_files_are_small():
    for tag in R.CASES:
        size = os.path.getsize(os.path.join(R.GOLDEN, "prop_loss_%s.npz" % tag))
        assert size <= R.FIXTURE_SIZE_LIMIT, (tag, size)
    assert R.FIXTURE_SIZE_LIMIT == max(os.path.getsize(os.path.join(R.GOLDEN, f)) for f in os.listdir(R.GOLDEN)
                                       if f.startswith(("mot_corr_", "corr_backward_")) and f.endswith(".npz"))
    src = open(os.path.join(R.GOLDEN, "make_golden_prop_loss.py")).read()
    assert "compute_loss_sot" in src and "compute_loss_vos" in src and "ref_bootstrap" in src


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn.py:315-337" in src
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
    ws = _lib.lib().uni_prop_workspace_bytes
    for B, Kc, Q in ((1, 1, 16000), (8, 1, 16000), (2, 8, 16000), (3, 1, 234), (1, 12, 64), (1, 1, 16)):
        got = ws(B, Kc, Q)
        assert 24 * B * Kc * ((Q + 1023) // 1024) <= got < 24 * B * Kc * ((Q + 1023) // 1024) + 256 and got % 256 == 0, (B, Kc, Q, got)
    for bad in ((0, 1, 64), (1, 0, 64), (1, 1025, 64), (40, 1000, 64), (1, 1, 15), (1, 1, 0), (2, 1024, 1 << 20)):
        assert ws(*bad) == 0, bad


def test_python_surface_rejects_bad_arguments_before_any_library_call(monkeypatch):
    from unicorn_amd import _lib, ops
    assert hasattr(ops, "PropDiceFunction") and hasattr(ops, "prop_labels")

    def no_library():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_library)
    e, t = torch.zeros(2, 128, 4, 6), torch.zeros(2, 2, 5, 6)

    def bad(match, e0=e, e1=e, tg=t, size=(32, 48), **kw):
        for fn in (ops.sot_prop_loss, ops.vos_prop_loss):
            with pytest.raises(_lib.UnicornHipError, match=match):
                fn(e0, e1, tg, size, **(kw if fn is ops.vos_prop_loss else {}))
    bad("do not fit", e0=e[0])
    bad("do not fit", e1=torch.zeros(2, 128, 4, 5))
    bad("do not fit", tg=torch.zeros(2, 2, 5, 5))
    bad("do not fit", tg=torch.zeros(2, 3, 5, 6))
    bad("do not fit", tg=torch.zeros(3, 2, 5, 6))
    bad("do not fit", tg=torch.zeros(2, 2, 0, 6))
    bad("not a tensor", tg=None)
    bad("is not 8 x", size=(32, 40))
    bad("is not 8 x", size=(24, 48), e0=torch.zeros(2, 128, 3, 6), e1=torch.zeros(2, 128, 3, 6))       # a map side below 4
    bad("not \\(height, width\\)", size=32)
    bad("no fp16", e0=e.half(), e1=e.half())
    bad("no fp16", e0=e.bfloat16(), e1=e.bfloat16())
    bad("unsupported", e1=e.double())                                               # mixed dtypes
    bad("C == 128", e0=e[:, :64], e1=e[:, :64])                                     # fp32 needs 128 channels
    bad("C <= 128", e0=torch.zeros(2, 130, 4, 6).double(), e1=torch.zeros(2, 130, 4, 6).double())
    bad("CPU tensor")                                                               # every other check passed: the device check is the last
    bad("CPU tensor", e0=e[:, :5].double(), e1=e[:, :5].double(), tg=t.half())      # fp64 takes fewer channels; targets of any dtype
    for kw, match in (({"masks": torch.zeros(2, 2, 5, 12, 18)}, "masks"), ({"masks": torch.zeros(2, 2, 4, 8, 12)}, "masks"),
                      ({"masks": torch.zeros(2, 2, 5, 8, 12).double()}, "fp32 or uint8"), ({"masks": 3}, "masks"), ({"max_inst": 0}, "max_inst")):
        with pytest.raises(_lib.UnicornHipError, match=match):
            ops.vos_prop_loss(e, e, t, (32, 48), **kw)
    with pytest.raises(_lib.UnicornHipError, match="CPU tensor"):
        ops.vos_prop_loss(e, e, t, (32, 48), masks=torch.zeros(2, 2, 5, 8, 12, dtype=torch.uint8), max_inst=2)
