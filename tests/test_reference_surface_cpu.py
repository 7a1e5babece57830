"""Drop-in boundary against the REAL reference tree (skipped where /root/reference is absent, e.g. on the GPU box):

  * `unicorn.exp.get_exp("exps/default/<file>.py")` of every experiment file the reference ships, patched with
    `unicorn_amd.exp.patch_exp`, builds the HIP model with that file's configuration (ConvNeXt exps) or fails loudly (ResNet-50);
  * every `model.<attr>` / `model.head.<attr>` the reference's inference drivers touch (external/lib/test/tracker/unicorn_sot.py,
    unicorn_vos.py, unicorn/evaluators/mot_evaluator.py, tools/track.py, tools/demo.py) exists on `unicorn_amd.models.Unicorn`.
"""
import ast
import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_bootstrap as rb  # noqa: E402

pytestmark = pytest.mark.skipif(not rb.reference_available(), reason="reference tree not present")


def _exp_files():
    """exps/default/<name>.py for every name of the stand-alone table plus every further file the reference ships: the case ids do
    not depend on whether the reference tree is present (without it every case skips with the module's reason)"""
    from unicorn_amd.exp import _DEFAULT_EXPS
    names = set(_DEFAULT_EXPS)
    if rb.reference_available():
        names |= {os.path.basename(p)[:-3] for p in glob.glob(os.path.join(rb.REF_ROOT, "exps", "default", "*.py"))}
    return [os.path.join(rb.REF_ROOT, "exps", "default", n + ".py") for n in sorted(names)]


@pytest.mark.parametrize("path", _exp_files(), ids=lambda p: os.path.basename(p)[:-3])
def test_real_reference_exp_files_build_the_hip_model(path):
    rb.boot()
    import warnings
    from unicorn.exp import get_exp as ref_get_exp
    from unicorn_amd.exp import patch_exp
    from unicorn_amd.models import Unicorn
    cwd = os.getcwd()
    os.chdir(rb.REF_ROOT)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            exp = ref_get_exp(os.path.relpath(path, rb.REF_ROOT), None)
    finally:
        os.chdir(cwd)
    name = os.path.basename(path)[:-3]
    backbone = getattr(exp, "backbone_name", None)
    if "r50" in name or (backbone is not None and not str(backbone).startswith("convnext")):
        with pytest.raises(ValueError):
            patch_exp(exp).get_model(load_pretrain=False)
        return
    if not hasattr(exp, "embed_dim"):          # detection-only experiments (unicorn_det_*, unicorn_inst_*): not the tracking model
        return
    m = patch_exp(exp).get_model(load_pretrain=False)
    assert isinstance(m, Unicorn) and m.precision == "f16x2"
    large = backbone == "convnext_large"
    assert m.dims == ((192, 384, 768, 1536) if large else (96, 192, 384, 768))
    assert m.depths == ((3, 3, 27, 3) if large else (3, 3, 9, 3))
    assert m.num_classes == exp.num_classes
    assert m.mask == (hasattr(exp, "d_rate") or hasattr(exp, "use_raft"))
    assert tuple(exp.test_size) in ((800, 1280), (640, 1024))
    # the stand-alone table (used where the reference is absent) must agree with the real file
    from unicorn_amd.exp import Exp, _DEFAULT_EXPS, model_cfg_from_exp
    assert name in _DEFAULT_EXPS, "exps/default/%s.py has no stand-alone entry" % name
    alone = Exp(name)
    assert tuple(alone.test_size) == tuple(exp.test_size)
    assert model_cfg_from_exp(alone) == model_cfg_from_exp(exp)


def _model_attrs(src, first_line=1, last_line=10 ** 9):
    """(first-level attributes of `model` / `self.model`, attributes of `model.head`) used between the two lines"""
    top, head = set(), set()

    def root(node):                                   # ... .model.<a>.<b>: returns the chain of attribute names after `model`
        chain = []
        while isinstance(node, ast.Attribute):
            chain.append(node.attr)
            node = node.value
        if isinstance(node, ast.Name):
            chain.append(node.id)
        chain.reverse()
        return chain
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Attribute) and first_line <= getattr(node, "lineno", 0) <= last_line:
            ch = root(node)
            if "model" in ch:
                k = ch.index("model")
                rest = ch[k + 1:]
                if rest and rest[0] == "module":          # DDP wrapper (tools/track.py -d > 1, test_omni.py:77,90): see INTEGRATION.md
                    rest = rest[1:]
                if rest:
                    top.add(rest[0])
                    if rest[0] == "head" and len(rest) > 1:
                        head.add(rest[1])
    return top, head


DRIVERS = [
    ("external/lib/test/tracker/unicorn_sot.py", 1, 10 ** 9),
    ("external/lib/test/tracker/unicorn_vos.py", 1, 10 ** 9),
    ("unicorn/evaluators/mot_evaluator.py", 100, 1100),
    ("tools/track.py", 170, 215),
    ("unicorn/utils/boxes.py", 80, 152),
]


def test_every_model_attribute_the_reference_drivers_touch_exists():
    from unicorn_amd.models import Unicorn
    m = Unicorn("unicorn_track_tiny_mask")               # no device needed for the surface
    top, head = set(), set()
    for rel, a, b in DRIVERS:
        src = open(os.path.join(rb.REF_ROOT, rel)).read()
        t, h = _model_attrs(src, a, b)
        top |= t
        head |= h
    assert {"head", "eval", "cuda", "load_state_dict"} <= top, top      # the walk found the calls it is meant to find
    assert "mask_head" in head or "decode_in_inference" in head, head
    for a in sorted(top):
        assert hasattr(m, a), "reference drivers use model.%s, unicorn_amd.models.Unicorn has no such attribute" % a
    for a in sorted(head):
        assert hasattr(m.head, a), "reference drivers use model.head.%s, missing on the HIP head" % a
    # tools/demo.py does not parse as shipped; its intended calls are model(img) and model.head as above


def test_model_call_signatures_match_reference_forward():
    """Unicorn.forward keyword names of the reference (unicorn/models/unicorn.py:110-139) and head(fpn_outs, masks, mode=...)"""
    import inspect
    rb.boot()
    from unicorn.models.unicorn import Unicorn as RefUnicorn
    from unicorn_amd.models import Unicorn
    ref = inspect.signature(RefUnicorn.forward).parameters
    ours = inspect.signature(Unicorn.forward).parameters
    for k in ("imgs", "seq_dict0", "seq_dict1", "feat", "mode"):
        assert k in ref and k in ours, k
    assert ours["mode"].default == ref["mode"].default == "whole"


def test_model_is_an_nn_module_shell():
    """The reference's tools treat the model as a torch.nn.Module: DDP(model, device_ids=[local_rank]) (tools/track.py:193-194),
    model.module.head (external/qdtrack/qdtrack/apis/test_omni.py:77,90), .eval() / .half().  unicorn_amd.models.Unicorn is a Module
    shell around the HIP context: those accessors work without a GPU; torch.jit.trace (tools/export_torchscript.py:70) raises.
    (Own process: the reference bootstrap of the other tests leaves stub modules in sys.modules that torch's DDP import chain probes.)"""
    import subprocess
    import sys
    code = r"""
import os, sys
sys.path.insert(0, %r)
import torch, torch.distributed as dist
from unicorn_amd import _lib as L
from unicorn_amd.models import Unicorn
m = Unicorn("unicorn_track_tiny_mask")
assert isinstance(m, torch.nn.Module) and isinstance(m.head, torch.nn.Module) and isinstance(m.head.mask_head, torch.nn.Module)
assert [n for n, _ in m.named_modules()] == ["", "head", "head.mask_head"]
assert m.eval() is m and not m.training and not m.head.training and m.half() is m and m.float() is m
assert next(m.parameters()).device.type == "cpu" and list(m.state_dict()) == ["_hip_anchor"]
try:
    m.train()
    raise SystemExit("train() must raise")
except L.UnicornHipError:
    pass
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", "29571")
dist.init_process_group("gloo", rank=0, world_size=1)
d = torch.nn.parallel.DistributedDataParallel(m)
assert d.module is m and d.module.head is m.head and d.module.head.num_classes == 8
dist.destroy_process_group()
try:
    torch.jit.trace(m, torch.zeros(1, 3, 64, 64))
    raise SystemExit("trace must raise")
except SystemExit:
    raise
except Exception:
    pass
print("MODULE_SURFACE_OK")
""" % (ROOT,)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and "MODULE_SURFACE_OK" in out.stdout, out.stderr[-1500:]


@pytest.mark.skipif(not rb.reference_available(), reason="reference tree absent")
def test_tracker_call_signatures_match_reference():
    """`unicorn.tracker` API kept: constructor and call signatures of the two association classes the evaluators drive
    (mot_evaluator.py:145,212 `BYTETracker(args).update(outputs[0], info_imgs, img_size)`; :968,1045 `QuasiDenseEmbedTracker().match(bboxes, labels, feats, frame_id)`),
    and the attributes read from the tracks `update` returns (:214-222)."""
    import inspect
    from types import SimpleNamespace
    rb.boot()
    from unicorn.tracker.byte_tracker import BYTETracker as RefByte, STrack as RefSTrack
    from unicorn.tracker.quasi_dense_embed_tracker import QuasiDenseEmbedTracker as RefQD
    from unicorn_amd.tracker import BYTETracker, QuasiDenseEmbedTracker
    from unicorn_amd.tracker.byte_tracker import STrack

    def names(fn):
        return [p for p in inspect.signature(fn).parameters if p != "self"]
    assert names(BYTETracker.__init__) == names(RefByte.__init__) == ["args", "frame_rate"]
    assert names(BYTETracker.update) == names(RefByte.update) == ["output_results", "img_info", "img_size"]
    ref_init, our_init = inspect.signature(RefQD.__init__).parameters, inspect.signature(QuasiDenseEmbedTracker.__init__).parameters
    assert list(ref_init) == list(our_init)
    for k in ref_init:
        if k != "self":
            assert ref_init[k].default == our_init[k].default, k                 # evaluate_omni constructs the tracker with its DEFAULTS
    assert names(QuasiDenseEmbedTracker.match)[:4] == names(RefQD.match)[:4] == ["bboxes", "labels", "track_feats", "frame_id"]
    for attr in ("tlwh", "track_id", "score", "tlbr"):
        assert hasattr(RefSTrack, attr) or attr in ("track_id", "score")
        assert attr in STrack.__slots__ or hasattr(STrack, attr), attr
    t = BYTETracker(SimpleNamespace(track_thresh=0.5, track_buffer=30, match_thresh=0.8, mot20=False))
    assert t.update(__import__("numpy").zeros((0, 5), dtype="float32"), (100, 100), (100, 100)) == []
