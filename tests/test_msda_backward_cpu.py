"""CPU-side checks of the MSDeformAttn backward boundary: the three new C-ABI symbols, the fixture tests/golden/msda_backward.npz
(lattice condition; oracle.msda_core under fp64 autograd reproduces the reference's gradients), loud failure on CPU tensors, and
unicorn_amd.msda_ext.install()."""
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("uni_msda_bwd", "uni_msda_fwd_f64", "uni_msda_bwd_f64")
CASES = ("a", "b", "c")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_msda_backward",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_msda_backward.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_new_symbols_declared_exported_and_bound():
    from unicorn_amd import _lib
    src = open(os.path.join(ROOT, "include", "unicorn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(uni_[a-z0-9_]+)\s*\(", src))
    lib = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in declared, "%s is not declared in include/unicorn_hip.h" % s
        assert s in _lib.PROTOS, "%s is missing from _lib.PROTOS" % s
        assert hasattr(lib, s), "libunicorn_hip.so does not export %s" % s
    # 16 pointer / size arguments + the stream for the backward, one fewer pointer pair for the forward
    assert len(_lib.PROTOS["uni_msda_bwd"][1]) == len(_lib.PROTOS["uni_msda_bwd_f64"][1]) == 17
    assert len(_lib.PROTOS["uni_msda_fwd_f64"][1]) == len(_lib.PROTOS["uni_msda_fwd"][1]) == 14
    assert lib.uni_version() == 1


def test_null_arguments_are_rejected():
    from unicorn_amd import _lib
    lib = _lib.lib()
    for name, nptr in (("uni_msda_bwd", 9), ("uni_msda_bwd_f64", 9), ("uni_msda_fwd_f64", 6)):
        rc = getattr(lib, name)(*([None] * nptr + [1, 1, 1, 1, 1, 1, 1, None]))
        assert rc < 0
        assert b"NULL" in lib.uni_last_error()


def test_fixture_is_small_and_lattice_safe(golden_dir):
    path = os.path.join(golden_dir, "msda_backward.npz")
    assert os.path.getsize(path) < 1000000
    gen = _generator()
    g = np.load(path)
    assert float(g["margin"]) == gen.MARGIN == 1e-3
    for c in CASES:
        shapes = [tuple(int(v) for v in r) for r in g["shapes_" + c]]
        loc = torch.from_numpy(g["loc_" + c])
        assert loc.dtype == torch.float32 and g["grad_value_" + c].dtype == np.float64
        assert gen.lattice_ok(loc, shapes), "case %s has a sample within 1e-3 of a pixel line" % c
        assert g["fp32_ref_err_" + c].shape == (3,) and (g["fp32_ref_err_" + c] > 0).all()
    # the construction moves a sample that sits on a pixel line and keeps one that does not
    loc = torch.tensor([0.125, 0.33]).view(1, 1, 1, 1, 1, 2).float()          # x * 4 - 0.5 = 0 exactly
    assert not gen.lattice_ok(loc, [(5, 4)])
    safe = gen.make_lattice_safe(loc, [(5, 4)])
    assert gen.lattice_ok(safe, [(5, 4)]) and safe[..., 1] == loc[..., 1] and safe[..., 0] != loc[..., 0]


@pytest.mark.parametrize("case", CASES)
def test_oracle_autograd_reproduces_fixture(case, golden_dir):
    """msda_core (the oracle's statement of the CUDA kernel) under fp64 autograd == the reference core's out and three gradients within
    1e-12 x tensor max: an fp64 evaluation of the same formula (measured disagreement <= 5e-13 absolute on gradients up to ~80).  This is
    what makes the oracle a valid second yardstick on the GPU box, where the reference is absent."""
    import unicorn_oracle as uo
    g = np.load(os.path.join(golden_dir, "msda_backward.npz"))
    shapes = [tuple(int(v) for v in r) for r in g["shapes_" + case]]
    v, l, a = (torch.from_numpy(g[k + "_" + case]).double().requires_grad_(True) for k in ("value", "loc", "attn"))
    out = uo.msda_core(v, shapes, l, a)
    out.backward(torch.from_numpy(g["grad_out_" + case]).double())
    for name, got in (("out", out.detach()), ("grad_value", v.grad), ("grad_loc", l.grad), ("grad_attn", a.grad)):
        ref = torch.from_numpy(g[name + "_" + case])
        err = float((got - ref).abs().max() / ref.abs().max())
        print("case %s %s: rel-to-max err %.3e" % (case, name, err))
        assert got.shape == ref.shape and err <= 1e-12, (name, err)


def test_cpu_tensors_raise():
    from unicorn_amd import _lib
    from unicorn_amd.ops import MSDeformAttnFunction, msda_backward, msda_forward
    shapes = torch.as_tensor([(6, 4), (3, 2)], dtype=torch.long)
    lsi = torch.tensor([0, 24])
    value = torch.rand(1, 30, 2, 2, requires_grad=True)
    loc = torch.rand(1, 2, 2, 2, 2, 2)
    attn = torch.rand(1, 2, 2, 2, 2)
    with pytest.raises(_lib.UnicornHipError):
        msda_backward(value, shapes, lsi, loc, attn, torch.rand(1, 2, 4))
    with pytest.raises(_lib.UnicornHipError):
        MSDeformAttnFunction.apply(value, shapes, lsi, loc, attn, 64)
    with pytest.raises(_lib.UnicornHipError):
        msda_forward(value.double(), shapes, lsi, loc.double(), attn.double())


@pytest.fixture
def clean_msda_module():
    saved = sys.modules.pop("MultiScaleDeformableAttention", None)
    yield
    sys.modules.pop("MultiScaleDeformableAttention", None)
    if saved is not None:
        sys.modules["MultiScaleDeformableAttention"] = saved


def test_install_exposes_both_names(clean_msda_module):
    from unicorn_amd import msda_ext
    m = msda_ext.install()
    assert sys.modules["MultiScaleDeformableAttention"] is m
    assert callable(m.ms_deform_attn_forward) and callable(m.ms_deform_attn_backward)
    import MultiScaleDeformableAttention as MSDA
    assert MSDA is m
    assert msda_ext.install() is m                                       # idempotent


def test_install_keeps_a_registered_module(clean_msda_module):
    from unicorn_amd import msda_ext
    other = types.ModuleType("MultiScaleDeformableAttention")
    sys.modules["MultiScaleDeformableAttention"] = other
    assert msda_ext.install() is other
    assert sys.modules["MultiScaleDeformableAttention"] is other and not hasattr(other, "ms_deform_attn_backward")


def test_reference_function_resolves_backward_after_install(clean_msda_module):
    """The reference's ops/functions/ms_deform_attn_func.py, loaded unmodified from its path after install(), binds MSDA to the
    stand-in: its MSDeformAttnFunction.backward reaches MSDA.ms_deform_attn_backward."""
    import ref_bootstrap as rb
    path = os.path.join(rb.REF_ROOT, "unicorn", "models", "ops", "functions", "ms_deform_attn_func.py")
    if not os.path.exists(path):
        pytest.skip("reference tree not present")
    from unicorn_amd import msda_ext
    m = msda_ext.install()
    spec = importlib.util.spec_from_file_location("ref_ms_deform_attn_func", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MSDA is m
    assert issubclass(mod.MSDeformAttnFunction, torch.autograd.Function)
    assert "MSDA" in mod.MSDeformAttnFunction.backward.__globals__ or "MSDA" in vars(mod)
    assert mod.MSDA.ms_deform_attn_backward is msda_ext.ms_deform_attn_backward
    assert mod.MSDA.ms_deform_attn_forward is msda_ext.ms_deform_attn_forward
