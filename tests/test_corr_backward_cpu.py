"""CPU-side checks of the differentiable label propagation (uni_corr_softmax_pv_lse / _bwd, ops.propagate_labels): the closed-form
gradients the kernels implement equal the fixture the reference's own lines produced; the fixture is what its generator says; the
new symbols are declared, exported and bound; the Python surface exists and fails the library's way without a device."""
import glob
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = {"flat": (1, 160, 130, 1, 0.3), "ragged": (1, 97, 203, 3, 0.3), "peaky": (1, 130, 110, 9, 1.0), "batch": (2, 64, 96, 2, 0.5)}
TENSORS = ("out", "lse", "g_embed_0", "g_embed_1", "g_labels")
NEW_SYMBOLS = ("uni_corr_bwd_workspace_bytes", "uni_corr_softmax_pv_lse", "uni_corr_softmax_pv_bwd", "uni_corr_softmax_pv_lse_f64",
               "uni_corr_softmax_pv_bwd_f64")


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "corr_backward_%s.npz" % tag)))


def closed_form(e_ref, e_cur, v, g):
    """The Mathematics of the operator in plain fp64 torch: e_ref (B,R,D), e_cur (B,Q,D), v (B,K,R), g (B,K,Q)."""
    S = torch.einsum("brd,bqd->brq", e_ref, e_cur)
    lse = torch.logsumexp(S, dim=1)                              # (B,Q)
    P = torch.exp(S - lse[:, None, :])
    out = torch.einsum("bkr,brq->bkq", v, P)
    delta = (g * out).sum(dim=1)                                 # (B,Q)
    T = torch.einsum("bkr,bkq->brq", v, g)
    dS = P * (T - delta[:, None, :])
    dV = torch.einsum("bkq,brq->bkr", g, P)
    dEr = torch.einsum("brq,bqd->brd", dS, e_cur)
    dEc = torch.einsum("brq,brd->bqd", dS, e_ref)
    return out, lse, dEr, dEc, dV


@pytest.mark.parametrize("tag", sorted(CASES))
def test_closed_form_gradients_equal_the_fixture(tag):
    c = load_case(tag)
    e0, e1 = torch.from_numpy(c["embed_0"]).double(), torch.from_numpy(c["embed_1"]).double()       # (B, C, HW)
    v, g = torch.from_numpy(c["labels"]).double(), torch.from_numpy(c["grad_out"]).double()
    out, lse, dEr, dEc, dV = closed_form(e0.transpose(1, 2), e1.transpose(1, 2), v, g)
    got = {"out": out, "lse": lse, "g_embed_0": dEr.transpose(1, 2), "g_embed_1": dEc.transpose(1, 2), "g_labels": dV}
    for n in TENSORS:
        ref = torch.from_numpy(c[n])
        assert ref.dtype == torch.float64 and got[n].shape == ref.shape, n
        err = float((got[n] - ref).abs().max() / ref.abs().max())
        assert err <= 1e-12, (tag, n, err)


def test_fixture_cases_are_the_described_ones():
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "corr_backward_*.npz"))) == \
        sorted("corr_backward_%s.npz" % t for t in CASES)
    total = 0
    for tag, (B, R, Q, K, scale) in CASES.items():
        path = os.path.join(GOLD, "corr_backward_%s.npz" % tag)
        assert os.path.getsize(path) < (1 << 20), "a committed file stays below 1 MiB"
        c = load_case(tag)
        assert tuple(c["shape"]) == (B, R, Q, K) and float(c["scale"]) == scale
        assert c["embed_0"].shape == (B, 128, R) and c["embed_1"].shape == (B, 128, Q) and c["labels"].shape == (B, K, R)
        assert c["grad_out"].shape == (B, K, Q) and c["out"].shape == (B, K, Q) and c["lse"].shape == (B, Q)
        assert all(c[n].dtype == np.float32 for n in ("embed_0", "embed_1", "labels", "grad_out"))
        assert abs(float(c["embed_0"].std()) / scale - 1) < 0.05 and 0 <= c["labels"].min() and c["labels"].max() <= 1
        for n in TENSORS:
            e = float(c[n + "_fp32_ref_err"])
            assert 1e-8 < e < 1e-5, (tag, n, e)                    # an fp32 evaluation's error: neither zero nor large
            assert float(np.abs(c[n]).max()) > 0.05, (tag, n)       # no comparison divides by something degenerate
            total += c[n].nbytes
        simi = torch.bmm(torch.from_numpy(c["embed_0"]).double().transpose(1, 2), torch.from_numpy(c["embed_1"]).double())
        med = float(torch.softmax(simi, dim=1).max(dim=1).values.median())          # median column maximum: flat vs peaky softmax
        if tag == "peaky":
            assert med > 0.7, med
        if tag == "flat":
            assert med < 0.15, med
    assert CASES["ragged"][1] % 32 and CASES["ragged"][2] % 32
    assert total < 2e6


def test_header_declares_and_protos_bind_the_new_symbols():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    assert "unicorn/models/unicorn.py:321-326" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), "%s is not declared in include/unicorn_hip.h" % s
        assert s in _lib.PROTOS, "%s is not bound in _lib.PROTOS" % s
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    assert lib.uni_version() == 1
    # host-side parts of the new entry points that need no device: sizes, and validation before anything is enqueued
    assert lib.uni_corr_bwd_workspace_bytes(1, 97, 203, 3) >= 203 * 4
    assert lib.uni_corr_bwd_workspace_bytes(0, 97, 203, 3) == 0


def test_python_surface_rejects_cpu_tensors_and_bad_shapes():
    from unicorn_amd import _lib, ops
    assert issubclass(ops.CorrSoftmaxPVFunction, torch.autograd.Function)
    e0, e1, lb = torch.zeros(1, 128, 4, 5), torch.zeros(1, 128, 4, 5), torch.zeros(1, 2, 20)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.UnicornHipError, match="HIP device tensors"):
            ops.propagate_labels(e0, e1, lb)
        with pytest.raises(_lib.UnicornHipError, match="HIP device tensors"):
            ops.CorrSoftmaxPVFunction.apply(torch.zeros(1, 20, 128), torch.zeros(1, 20, 128), lb)
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.propagate_labels(e0, e1, torch.zeros(1, 2, 19))                  # labels of another map size
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.propagate_labels(e0, torch.zeros(2, 128, 4, 5), lb)              # batch mismatch
    with pytest.raises(_lib.UnicornHipError, match="do not fit"):
        ops.CorrSoftmaxPVFunction.apply(torch.zeros(20, 128), torch.zeros(20, 128), torch.zeros(2, 20))
    with pytest.raises(_lib.UnicornHipError, match="dtypes"):
        ops.propagate_labels(e0, e1.double(), lb)
    with pytest.raises(_lib.UnicornHipError, match="B, C, H, W"):
        ops.propagate_labels(torch.zeros(128, 20), e1, lb)
