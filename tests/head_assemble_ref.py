"""Pure-torch restatement of the eager lines between the head's prediction convolutions and get_losses (unicorn/models/unicorn_head_mask.py
:339-366 of forward, get_output_and_grid :476-500, the level cats :396-401 and :554-558; n_anchors == 1), in the dtype and on the device of
its inputs, the per-level host-built tensors included: what ops.head_assemble replaces.  tests/test_head_assemble_cpu.py pins it to the
fixtures that the reference's own lines produced (tests/golden/make_golden_head_assemble.py); the GPU tests and tools/head_assemble_bench.py
use it where no fixture exists.  A plain module imported like tests/planted.py; it holds no fixture and changes no pytest setting."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TILE = 64                       # the anchor tile of csrc/head_assemble.hip (HA_TILE; tests/test_head_assemble_cpu.py holds the two together)
# tag -> (B, C, levels (h, w), P or 0, seed); strides 8, 16, 32, 64 by level
CASES = {"small": (2, 1, ((8, 12), (4, 6), (2, 3)), 169, 4100),
         "cls8": (3, 8, ((7, 9), (3, 5), (1, 2)), 0, 4200),
         "one": (1, 1, ((1, 1),), 0, 4300),
         "edge": (1, 1, ((5, 13), (1, 1)), 169, 4400),           # 5 x 13 = TILE + 1 anchors
         "c80": (2, 80, ((5, 13), (2, 3)), 0, 4500)}
STRIDES = (8, 16, 32, 64)
MAPS = ("reg", "obj", "cls", "ctrl")
RESULTS = ("outputs", "origin_preds", "x_shifts", "y_shifts", "expanded_strides", "dynamic_params", "fpn_levels")


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "head_assemble_%s.npz" % tag)))


def _coarse(shape, g):
    """values on a grid of 1 / 8 in [-8, 8): what a pass-through quantity carries (it compresses well; the values do not matter)"""
    return torch.randint(-64, 64, shape, generator=g).float() / 8


def problem(tag):
    """-> dict: the fp32 maps reg / obj / cls / ctrl (lists over the levels, ctrl None without controller maps), strides, and the unequal
    gradients g_outputs (B, A, 5 + C), g_origin (B, A, 4), g_params (B, A, P) of the recorded backward -- all from the case's seed.  reg,
    obj and the five leading gradient columns are normal draws; cls, ctrl and their gradients lie on a coarse grid."""
    B, C, levels, P, seed = CASES[tag]
    g = torch.Generator().manual_seed(seed)
    A = sum(h * w for h, w in levels)
    p = {"B": B, "C": C, "P": P, "A": A, "levels": levels, "strides": STRIDES[:len(levels)],
         "reg": [torch.randn(B, 4, h, w, generator=g) for h, w in levels],
         "obj": [torch.randn(B, 1, h, w, generator=g) for h, w in levels],
         "cls": [_coarse((B, C, h, w), g) for h, w in levels],
         "ctrl": [_coarse((B, P, h, w), g) for h, w in levels] if P else None}
    p["g_outputs"] = torch.cat([torch.randn(B, A, 5, generator=g), _coarse((B, A, C), g)], 2)
    p["g_origin"] = torch.randn(B, A, 4, generator=g)
    p["g_params"] = _coarse((B, A, P), g) if P else None
    return p


def assemble(reg_outputs, obj_outputs, cls_outputs, strides, controller_outputs=None, use_l1=True):
    """the eager lines -> (outputs, origin_preds, x_shifts, y_shifts, expanded_strides, dynamic_params, fpn_levels) as get_losses sees them
    after its own cats; fpn_levels stays where torch.full builds it (the host), as in the reference"""
    xin0 = reg_outputs[0]
    outputs, origin_preds, x_shifts, y_shifts, expanded_strides, dynamic_params, fpn_levels = [], [], [], [], [], [], []
    for k, (reg_output, obj_output, cls_output, stride_this_level) in enumerate(zip(reg_outputs, obj_outputs, cls_outputs, strides)):
        if controller_outputs is not None:
            d_param = controller_outputs[k].flatten(-2).permute((0, 2, 1))                      # :339
            dynamic_params.append(d_param)
            fpn_levels.append(torch.full((d_param.size(0), d_param.size(1)), k))                # :342
        output = torch.cat([reg_output, obj_output, cls_output], 1)                              # :346
        # get_output_and_grid :476-500 (the grid cache is a speed-up of the reference and does not change the values)
        batch_size, n_ch = output.shape[0], output.shape[1]
        hsize, wsize = output.shape[-2:]
        yv, xv = torch.meshgrid([torch.arange(hsize), torch.arange(wsize)], indexing="ij")
        grid = torch.stack((xv, yv), 2).view(1, 1, hsize, wsize, 2).type(xin0.type())
        output = output.view(batch_size, 1, n_ch, hsize, wsize)
        output = output.permute(0, 1, 3, 4, 2).reshape(batch_size, hsize * wsize, -1)
        grid = grid.view(1, -1, 2)
        output[..., :2] = (output[..., :2] + grid) * stride_this_level
        output[..., 2:4] = torch.exp(output[..., 2:4]) * stride_this_level
        x_shifts.append(grid[:, :, 0])                                                           # :350-356
        y_shifts.append(grid[:, :, 1])
        expanded_strides.append(torch.zeros(1, grid.shape[1]).fill_(stride_this_level).type_as(xin0))
        if use_l1:                                                                               # :357-366
            r = reg_output.view(batch_size, 1, 4, hsize, wsize)
            r = r.permute(0, 1, 3, 4, 2).reshape(batch_size, -1, 4)
            origin_preds.append(r.clone())
        outputs.append(output)
    return (torch.cat(outputs, 1), torch.cat(origin_preds, 1) if use_l1 else None, torch.cat(x_shifts, 1), torch.cat(y_shifts, 1),
            torch.cat(expanded_strides, 1), torch.cat(dynamic_params, 1) if controller_outputs is not None else None,
            torch.cat(fpn_levels, 1) if controller_outputs is not None else None)


def weighted(res, p, dtype, device="cpu"):
    """the scalar whose gradients the fixtures record: sum g_outputs x outputs + sum g_origin x origin_preds + sum g_params x dynamic_params"""
    s = (res[0] * p["g_outputs"].to(device=device, dtype=dtype)).sum() + (res[1] * p["g_origin"].to(device=device, dtype=dtype)).sum()
    if res[5] is not None:
        s = s + (res[5] * p["g_params"].to(device=device, dtype=dtype)).sum()
    return s


def leaves(p, dtype, device="cpu", memory_format=torch.contiguous_format):
    """the maps of a problem as leaf tensors that require a gradient: (reg, obj, cls, ctrl or None), lists over the levels"""
    def leaf(t):
        return t.to(device=device, dtype=dtype).clone(memory_format=memory_format).requires_grad_(True)
    return tuple(None if p[m] is None else [leaf(t) for t in p[m]] for m in MAPS)


def run(p, dtype, device="cpu"):
    """the restatement with its backward -> dict: the seven RESULTS and grad_<map>_<level>, detached"""
    reg, obj, cls, ctrl = leaves(p, dtype, device)
    res = assemble(reg, obj, cls, p["strides"], ctrl)
    weighted(res, p, dtype, device).backward()
    out = {k: (None if t is None else t.detach()) for k, t in zip(RESULTS, res)}
    for m, ts in zip(MAPS, (reg, obj, cls, ctrl)):
        for k, t in enumerate(ts or ()):
            out["grad_%s_%d" % (m, k)] = t.grad
    return out


def stored_names(p):
    """the quantities a fixture holds: every result and gradient, the P-wide ones in fp32 only (pass-through: the two runs agree bit for bit)"""
    names = ["outputs", "origin_preds", "x_shifts", "y_shifts", "expanded_strides"]
    names += ["grad_%s_%d" % (m, k) for m in MAPS[:3] for k in range(len(p["levels"]))]
    wide = (["dynamic_params", "fpn_levels"] + ["grad_ctrl_%d" % k for k in range(len(p["levels"]))]) if p["P"] else []
    return names, wide


def rel_err(got, want):
    """max |got - want| / max |want| in double (0 / 0 = 0)"""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want).detach().double().cpu()
    d, s = float((got - want).abs().max()) if want.numel() else 0.0, float(want.abs().max()) if want.numel() else 0.0
    return (0.0 if d == 0.0 else float("inf")) if s == 0.0 else d / s


def bits_equal(got, want):
    got, want = torch.as_tensor(got).detach().cpu().contiguous(), torch.as_tensor(want).detach().cpu().contiguous()
    return got.dtype == want.dtype and got.shape == want.shape and torch.equal(got.reshape(-1).view(torch.uint8), want.reshape(-1).view(torch.uint8))
