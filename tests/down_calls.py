"""Calls of uni_down_train_* and uni_patch4_* through the C-ABI for the kernel-level tests: buffers are torch tensors or tests/guard.py
allocations, the shapes are those of include/unicorn_hip.h.  No GPU work at import."""
import ctypes as C

import torch

import guard as G

DT = {torch.float32: 0, torch.float64: 0, torch.float16: 1, torch.bfloat16: 2}


def P(x):
    return None if x is None else C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def sfx(f64):
    return "_f64" if f64 else ""


def cl_rows(t):
    """(N, C, H, W) -> the (N H W, C) rows of channels-last memory"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).contiguous()


def from_cl_rows(t, shape):
    N, Cc, H, W = shape
    return t.reshape(N, H, W, Cc).permute(0, 3, 1, 2)


def ws_bytes(L, f64, dims):
    return L.lib().uni_down_train_workspace_bytes(*dims) * (2 if f64 else 1)


def down_fwd(L, f64, x, xd, w, b, dims, rebuild, A, ad, stats, eps=1e-6):
    """dims = (B, H, W, C)"""
    name = "uni_down_train_fwd" + sfx(f64)
    L.check(getattr(L.lib(), name)(P(x), xd, P(w), P(b), eps, *dims, rebuild, P(A), ad, P(stats), L.stream_ptr()), name)


def down_bwd(L, f64, x, xd, w, stats, gA, ad, dims, gx, gw, gb, ws, nws):
    name = "uni_down_train_bwd" + sfx(f64)
    L.check(getattr(L.lib(), name)(P(x), xd, P(w), P(stats), P(gA), ad, *dims, P(gx), P(gw), P(gb), P(ws), nws, L.stream_ptr()), name)


def gather(L, f64, x, xd, dims, A, ad):
    """dims = (B, Cin, H, W)"""
    name = "uni_patch4_gather" + sfx(f64)
    L.check(getattr(L.lib(), name)(P(x), xd, *dims, P(A), ad, L.stream_ptr()), name)


def scatter(L, f64, gA, ad, dims, gx, xd):
    name = "uni_patch4_scatter" + sfx(f64)
    L.check(getattr(L.lib(), name)(P(gA), ad, *dims, P(gx), xd, L.stream_ptr()), name)


def run_down(L, x, w, b, gA, a_dtype, need_x=True, need_p=True):
    """x (N, C, H, W) device tensor of any admitted dtype, w, b (C,), gA (M, 4C) in a_dtype -> dict(A, stats, A2 (the rebuild), g_x (N, C, H, W),
    g_ln_weight, g_ln_bias); the math type is that of w"""
    N, Cc, H, W = x.shape
    f64 = w.dtype == torch.float64
    dims = (N, H, W, Cc)
    M = N * (H // 2) * (W // 2)
    xr = cl_rows(x)
    e = lambda dt, *s: torch.empty(*s, device=x.device, dtype=dt)       # noqa: E731
    A, A2, stats = e(a_dtype, M, 4 * Cc), e(a_dtype, M, 4 * Cc), e(w.dtype, N * H * W, 2)
    down_fwd(L, f64, xr, DT[x.dtype], w, b, dims, 0, A, DT[a_dtype], stats)
    down_fwd(L, f64, xr, DT[x.dtype], w, b, dims, 1, A2, DT[a_dtype], stats)
    gx = e(x.dtype, N * H * W, Cc) if need_x else None
    gw, gb = (e(w.dtype, Cc), e(w.dtype, Cc)) if need_p else (None, None)
    nws = ws_bytes(L, f64, dims)
    ws = e(torch.uint8, nws) if need_p else None
    down_bwd(L, f64, xr, DT[x.dtype], w, stats, gA.contiguous(), DT[a_dtype], dims, gx, gw, gb, ws, nws if need_p else 0)
    torch.cuda.synchronize()
    return dict(A=A, A2=A2, stats=stats, g_x=None if gx is None else from_cl_rows(gx, x.shape), g_ln_weight=gw, g_ln_bias=gb)
