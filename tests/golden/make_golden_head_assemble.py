"""Golden vectors for the head-output assembly (uni_head_assemble_fwd / _bwd, ops.HeadAssembleFunction / head_assemble), produced by
EXECUTING the reference's own lines on the CPU, once in fp64 and once in fp32, with a backward:

  * UnicornHeadMask.get_output_and_grid (unicorn/models/unicorn_head_mask.py:476-500) is CALLED on a head made with __new__ (it reads mode,
    num_classes, num_classes_sot, n_anchors and grids; grids is reset between the two runs: the reference caches the grid in the dtype of
    the first call);
  * the inline lines of forward around it -- :339-343 (dynamic_params, fpn_levels) and :345-366 (the cat :346, the call, shifts, strides and
    origin_preds :358-366) -- and the level cats :396, :400, :401 and :554-558 are READ from the reference at generation time, dedented and
    exec'd in a namespace that holds the names they use, as make_golden_sample.py does.  No reference text is stored.

Inputs and the unequal gradients of the recorded backward come from tests/head_assemble_ref.py::problem (a recorded seed per case).  Every file
holds the narrow inputs, the results and gradients of the fp64 run, the same of the fp32 run (<name>_fp32) and per quantity
<name>_fp32_ref_err = max |fp32 - fp64| / max |fp64| (an exact 0.0 where the two agree bit for bit after widening).  The P-wide quantities
(dynamic_params, fpn_levels, grad_ctrl_*) are pass-through: asserted equal in the two runs and stored once, in fp32.

    python tests/golden/make_golden_head_assemble.py        -> tests/golden/head_assemble_<case>.npz
"""
import os
import sys
import textwrap

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import head_assemble_ref as R  # noqa: E402


def reference_lines():
    """the code objects of the inline lines, read from the reference"""
    import ref_bootstrap
    src = open(os.path.join(ref_bootstrap.REF_ROOT, "unicorn", "models", "unicorn_head_mask.py")).read().split("\n")

    def block(first, last, head, tail):          # 1-based, inclusive
        lines = src[first - 1:last]
        assert head in lines[0] and tail in lines[-1], (lines[0], lines[-1])
        return textwrap.dedent("\n".join(lines))

    def expr(line, text):                        # an argument line of the get_losses call: `torch.cat(outputs, 1),`
        assert src[line - 1].strip() == text + ",", src[line - 1]
        return text
    ctrl = block(339, 343, "d_param = d_param.flatten(-2).permute((0, 2, 1))", "fpn_levels.append(fpn_level)")
    level = block(345, 366, "if self.training:", "origin_preds.append(reg_output.clone())")
    assert "output = torch.cat([reg_output, obj_output, cls_output], 1)" in level and "self.get_output_and_grid(" in level
    cats = {"outputs": expr(396, "torch.cat(outputs, 1)"), "dynamic_params": expr(400, "torch.cat(dynamic_params, 1)"),
            "fpn_levels": expr(401, "torch.cat(fpn_levels, 1)")}
    late = block(554, 558, "x_shifts = torch.cat(x_shifts, 1)", "origin_preds = torch.cat(origin_preds, 1)")
    return ctrl, level, cats, late


def reference_run(p, dtype, code):
    """the reference's lines + backward on the CPU in `dtype` -> dict of results and gradients"""
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.unicorn_head_mask import UnicornHeadMask
    ctrl_code, level_code, cats, late = code
    head = UnicornHeadMask.__new__(UnicornHeadMask)
    nn.Module.__init__(head)
    head.mode, head.num_classes, head.num_classes_sot, head.n_anchors, head.use_l1 = "mot", p["C"], p["C"], 1, True
    head.grids = [torch.zeros(1)] * len(p["levels"])                      # fresh: the cache keeps the dtype of its first call
    assert head.training
    reg, obj, cls, ctrl = R.leaves(p, dtype)
    ns = {"torch": torch, "self": head, "xin": [reg[0]], "outputs": [], "origin_preds": [], "x_shifts": [], "y_shifts": [],
          "expanded_strides": [], "dynamic_params": [], "fpn_levels": []}
    for k, stride in enumerate(p["strides"]):
        ns.update(k=k, stride_this_level=stride, reg_output=reg[k], obj_output=obj[k], cls_output=cls[k])
        if ctrl is not None:
            ns["d_param"] = ctrl[k]
            exec(ctrl_code, ns)
        exec(level_code, ns)
        ns["outputs"].append(ns["output"])                                 # :372
    res = {k: eval(v, ns) for k, v in cats.items() if ctrl is not None or k == "outputs"}
    exec(late, ns)
    for k in ("origin_preds", "x_shifts", "y_shifts", "expanded_strides"):
        res[k] = ns[k]
    ordered = tuple(res.get(k) for k in R.RESULTS)
    R.weighted(ordered, p, dtype).backward()
    out = {k: (None if t is None else t.detach()) for k, t in zip(R.RESULTS, ordered)}
    for m, ts in zip(R.MAPS, (reg, obj, cls, ctrl)):
        for k, t in enumerate(ts or ()):
            out["grad_%s_%d" % (m, k)] = t.grad
    return out


def one_case(tag, code):
    p = R.problem(tag)
    r64, r32 = reference_run(p, torch.float64, code), reference_run(p, torch.float32, code)
    res = {"levels": np.array(p["levels"], dtype=np.int64), "strides": np.array(p["strides"], dtype=np.float64),
           "shape": np.array([p["B"], p["C"], p["P"], p["A"]], dtype=np.int64), "seed": np.int64(R.CASES[tag][4])}
    for m in R.MAPS[:3]:
        for k, t in enumerate(p[m]):
            res["%s_%d" % (m, k)] = t.numpy()
    names, wide = R.stored_names(p)
    for k in names:
        assert r64[k].dtype == torch.float64 and r32[k].dtype == torch.float32, k
        res[k], res[k + "_fp32"] = r64[k].numpy(), r32[k].numpy()
        res[k + "_fp32_ref_err"] = np.float64(0.0 if torch.equal(r32[k].double(), r64[k]) else R.rel_err(r32[k], r64[k]))
    for k in wide:
        assert torch.equal(r32[k].double(), r64[k].double()), k
        res[k + "_fp32"] = r32[k].numpy()
        res[k + "_fp32_ref_err"] = np.float64(0.0)
    # what the tests lean on: everything but the two exp columns and their gradient is exact in fp32
    o64, o32 = r64["outputs"], r32["outputs"].double()
    assert torch.equal(o32[..., 4:], o64[..., 4:]), "pass-through columns differ between the runs"
    res["outputs_exp_fp32_ref_err"] = np.float64(R.rel_err(o32[..., 2:4], o64[..., 2:4]))
    res["outputs_xy_fp32_ref_err"] = np.float64(R.rel_err(o32[..., :2], o64[..., :2]))
    for k in range(len(p["levels"])):
        g64, g32 = r64["grad_reg_%d" % k], r32["grad_reg_%d" % k].double()
        res["grad_reg_%d_exp_fp32_ref_err" % k] = np.float64(R.rel_err(g32[:, 2:], g64[:, 2:]))
        res["grad_reg_%d_xy_fp32_ref_err" % k] = np.float64(R.rel_err(g32[:, :2], g64[:, :2]))
    print("%-6s B %d C %d P %d A %d  %s" % (tag, p["B"], p["C"], p["P"], p["A"], "  ".join(
        "%s %.2g" % (k[:-13], float(v)) for k, v in sorted(res.items()) if k.endswith("_fp32_ref_err") and float(v) > 0)))
    return res


def main():
    code = reference_lines()
    for tag in R.CASES:
        res = one_case(tag, code)
        path = os.path.join(HERE, "head_assemble_%s.npz" % tag)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        print(path, size, "bytes")
        assert size < 256 * 1024, "a fixture stays below 256 KB"


if __name__ == "__main__":
    main()
