"""The kernels of csrc/pw_mlp.hip alone, through the C-ABI (uni_pw_mlp_act_fwd / _bwd and their _f64 twins): the one calling helper that
tests/test_pw_mlp_gpu.py and tests/test_pw_mlp_plans_gpu.py share, and the trace of their launches.  Needs a device when called, not when
imported."""
import ctypes as C

import torch

import variant_cases as vc

DEV = "cuda"
H_DTYPE = {torch.float32: 0, torch.float64: 0, torch.float16: 1, torch.bfloat16: 2}


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def act_calls(L, h, ga, gy=None, want=("a", "gh", "gb1"), inplace=False, ws=True):
    """uni_pw_mlp_act_fwd and _bwd on (M, Hd) device maps of one dtype -> {a_fwd, a, grad_h, g_b1, g_b2}"""
    lib = L.lib()
    f64 = h.dtype == torch.float64
    sfx = "_f64" if f64 else ""
    M, Hd = h.shape
    Co = gy.shape[1] if gy is not None else 4
    hd = H_DTYPE[h.dtype]
    sdt = torch.float64 if f64 else torch.float32
    s = L.stream_ptr()
    out = {}
    hf = h.clone()
    out["a_fwd"] = hf if inplace else torch.empty_like(h)
    L.check(getattr(lib, "uni_pw_mlp_act_fwd" + sfx)(P(hf), hd, M, Hd, P(out["a_fwd"]), s), "uni_pw_mlp_act_fwd" + sfx)
    hb, gb = h.clone(), ga.clone()
    out["a"] = (hb if inplace else torch.empty_like(h)) if "a" in want else None
    out["grad_h"] = (gb if inplace else torch.empty_like(h)) if "gh" in want else None
    out["g_b1"] = torch.empty(Hd, device=DEV, dtype=sdt) if "gb1" in want else None
    out["g_b2"] = torch.empty(Co, device=DEV, dtype=sdt) if gy is not None else None
    need = lib.uni_pw_mlp_workspace_bytes(M, Hd, Co) * (2 if f64 else 1)
    assert need == 4 * 256 * (Hd + Co) * (2 if f64 else 1)
    wsb = torch.empty(need, dtype=torch.uint8, device=DEV) if ws else None
    L.check(getattr(lib, "uni_pw_mlp_act_bwd" + sfx)(P(hb), hd, P(gb), M, Hd, P(out["a"]), P(out["grad_h"]), P(out["g_b1"]), P(gy), Co, P(out["g_b2"]),
                                                     P(wsb), need if ws else 0, s), "uni_pw_mlp_act_bwd" + sfx)
    torch.cuda.synchronize()
    return out


def traced(L, fn):
    """fn() with the variant trace on -> (its result, {tag: launches} of the `pw_mlp ` tags)"""
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        res = fn()
    finally:
        lib.uni_variant_trace(0)
    return res, {t: v for t, v in vc.read_trace(lib).items() if t.startswith("pw_mlp ")}
