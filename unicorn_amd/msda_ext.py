"""Stand-in for the reference's compiled extension `MultiScaleDeformableAttention` (unicorn/models/ops/src/vision.cpp:13-16), which
exists for CUDA only (ops/src/ms_deform_attn.h:19-61 has no CPU or ROCm branch).

    import unicorn_amd.msda_ext
    unicorn_amd.msda_ext.install()

registers a module object with the extension's two functions under that name, so that the reference's
`ops/functions/ms_deform_attn_func.py` (`import MultiScaleDeformableAttention as MSDA`) and its `MSDeformAttn` module run unmodified on
ROCm, forward and backward, on the HIP kernels of libunicorn_hip.so (uni_msda_fwd / uni_msda_bwd and their _f64 forms).  Nothing is
registered at import; install() must be called before the reference's ops package is imported."""
import importlib.util
import sys
import types

from . import ops

NAME = "MultiScaleDeformableAttention"


def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step):
    return ops.msda_forward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, im2col_step)


def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step):
    return list(ops.msda_backward(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_output, im2col_step))


def module():
    """A fresh module object carrying the two pybind names."""
    m = types.ModuleType(NAME, "HIP implementation of the MultiScaleDeformableAttention extension (unicorn_amd.msda_ext)")
    m.ms_deform_attn_forward = ms_deform_attn_forward
    m.ms_deform_attn_backward = ms_deform_attn_backward
    return m


def install():
    """Make `import MultiScaleDeformableAttention` resolve.  A module already registered under the name, or a real extension that can be
    imported, wins and is returned untouched; otherwise the HIP stand-in is registered in sys.modules and returned."""
    if NAME in sys.modules:
        return sys.modules[NAME]
    if importlib.util.find_spec(NAME) is not None:
        return importlib.import_module(NAME)
    sys.modules[NAME] = module()
    return sys.modules[NAME]
