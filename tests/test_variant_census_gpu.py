"""Which kernel does a test run?  The variant trace of the library (uni_variant_trace) makes the launchers say it, and this module turns the
answer into checks:
  1. the trace itself (off by default, one tag per launch, split-K = partial + reduce tags, restart clears);
  2. a census of the tags the engine dispatches on the headline step (unicorn_track_large, f16x2, 800x1280, 16 frames and one frame) and on the
     tiny mask model (f16x2 352x608 x 3 frames, fp32 320x320), one forward pass each, written to variant_census.json in the suite's results directory
     (tests/guard.py results_dir, where parity_metrics.json goes);
  3. one kernel-level parity case per tag (tests/variant_cases.py CASES): the traced call must emit the tag -- the shape really reaches the
     variant -- and match its fp64 CPU reference under the bound restated from the existing parity tables;
  4. closure: every census tag has a case or is one of the context-only launchers of CTX_ONLY."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import guard
import variant_cases as vc

pytestmark = pytest.mark.gpu

ACTS = {0: lambda x: x, 1: F.relu, 2: F.gelu, 3: F.silu, 4: torch.sigmoid}
H2_FILL = 0x47004700      # int32 pre-fill of f16x2 buffers (two f16 7.0)


def _lib():
    from unicorn_amd import _lib as L
    L.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return L


@pytest.fixture(scope="module")
def L():
    return _lib()


def traced(L, fn):
    """run fn with the trace on -> (result, {tag: count})"""
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        r = fn()
        torch.cuda.synchronize()
    finally:
        lib.uni_variant_trace(0)
    return r, vc.read_trace(lib)


# ------------------------------------------------------------------------------------------------ buffers in the three operand formats
def op_buffer(rows, ld, fmt):
    """pre-filled (rows, ld) operand buffer: bf16 / fp32 elements or f16x2 groups (int32 storage, 4 B per element)"""
    if fmt == 0:
        return torch.full((rows, ld), 7.0, device="cuda", dtype=torch.bfloat16)
    if fmt == 1:
        return torch.full((rows, ld), 7.0, device="cuda", dtype=torch.float32)
    return torch.full((rows, ld), H2_FILL, device="cuda", dtype=torch.int32)


def op_decode(buf, fmt):
    """-> fp64 CPU values, f16x2 as hi + lo ([8 hi][8 lo] per 8 elements)"""
    if fmt == 2:
        rows, ld = buf.shape
        h = buf.view(torch.float16).reshape(rows, ld // 8, 2, 8).cpu().double()
        return (h[:, :, 0] + h[:, :, 1]).reshape(rows, ld)
    return buf.cpu().double()


def op_untouched(buf, fmt, rows, C_):
    """columns >= C_ of the first `rows` rows and every row behind them still hold the pre-fill"""
    fill = H2_FILL if fmt == 2 else 7.0
    b = buf.cpu()
    return bool((b[:rows, C_:] == fill).all()) and bool((b[rows:] == fill).all())


# ------------------------------------------------------------------------------------------------ runners: case args -> list of checks
# a check = (what, got fp64, reference fp64, absolute tolerance); runners also assert that nothing outside the outputs was written
def run_dwconv7_ln_ex(L, a, bound):
    C_, B, H, W, fmt = a["C"], a["B"], a["H"], a["W"], a["fmt"]
    g = torch.Generator().manual_seed(C_ + H + B)
    x = torch.randn(B, C_, H, W, generator=g)
    w = torch.randn(C_, 1, 7, 7, generator=g) / 7
    b, ga, be = torch.randn(C_, generator=g) * 0.1, 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    y = F.conv2d(x.double(), w.double(), b.double(), padding=3, groups=C_).permute(0, 2, 3, 1)
    exp = F.layer_norm(y, (C_,), ga.double(), be.double(), 1e-6).reshape(-1, C_)
    xn = x.permute(0, 2, 3, 1).contiguous().cuda()
    wt = w.reshape(C_, 49).t().contiguous().cuda()
    bd, gd, bed = b.cuda(), ga.cuda(), be.cuda()
    M = B * H * W
    out = op_buffer(M + 1, C_, fmt)
    L.check(L.lib().uni_dwconv7_ln_ex(L.ptr(xn), L.ptr(wt), L.ptr(bd), L.ptr(gd), L.ptr(bed), 1e-6, B, H, W, C_, L.ptr(out), fmt, L.stream_ptr()), "dwln_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, fmt, M, C_), "dwconv7_ln_ex wrote behind its output"
    return [("out", op_decode(out, fmt)[:M], exp, bound * max(1.0, exp.abs().max().item()))]


def run_layernorm_ex(L, a, bound):
    C_, fmt, mode = a["C"], a["fmt"], a["mode"]
    B = a.get("B", 1)
    if mode == "ps":
        M = B * a["h"] * a["w"]
    elif mode == "pair":
        M = B * 2 * a["pair_hw"]
    else:
        M = a["M"]
    g = torch.Generator().manual_seed(C_ + fmt + M)
    ldx = C_ + 8
    x = torch.randn(M, ldx, generator=g) * 3 + 1.5
    ga, be = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    exp = F.layer_norm(x[:, :C_].double(), (C_,), ga.double(), be.double(), 1e-6)
    big = exp.abs().max().item()
    rows_f = B * a["pair_hw"] if mode == "pair" else M
    ldf, ldb = C_ + 4, C_ + 8
    outF = torch.full((rows_f + 1, ldf), 7.0, device="cuda") if a["outF"] else None
    outF2 = torch.full((rows_f + 1, ldf), 7.0, device="cuda") if mode == "pair" else None
    outB = None
    if a["outB"]:
        outB = op_buffer(4 * M + 8, C_ // 4, fmt) if mode == "ps" else op_buffer(M + 1, ldb, fmt)
    xd, gd, bd = x.cuda(), ga.cuda(), be.cuda()
    L.check(L.lib().uni_layernorm_ex(L.ptr(xd), ldx, L.ptr(gd), L.ptr(bd), 1e-6, M, C_, L.ptr(outF), ldf, L.ptr(outF2), a.get("pair_hw", 0),
                                     L.ptr(outB), ldb, a["h"] if mode == "ps" else 0, a["w"] if mode == "ps" else 0, fmt, L.stream_ptr()), "layernorm_ex")
    torch.cuda.synchronize()
    checks = []
    if mode == "pair":
        e = exp.reshape(B, 2, a["pair_hw"], C_)
        for name, buf, t in (("outF (even frames)", outF, 0), ("outF2 (odd frames)", outF2, 1)):
            assert op_untouched(buf, 1, rows_f, C_), name + ": complement written"
            checks.append((name, buf.cpu().double()[:rows_f, :C_], e[:, t].reshape(rows_f, C_), vc.B_LN_F32 * big))
    elif outF is not None:
        assert op_untouched(outF, 1, M, C_), "outF: complement written"
        checks.append(("outF", outF.cpu().double()[:M, :C_], exp, vc.B_LN_F32 * big))
    if outB is not None:
        tol = bound * (max(1.0, big) if fmt == 2 else big)
        if mode == "ps":
            h, w = B * a["h"], a["w"]
            e = F.pixel_shuffle(exp.reshape(1, h, w, C_).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(4 * M, C_ // 4)
            assert op_untouched(outB, fmt, 4 * M, C_ // 4), "outB (PixelShuffle): written behind the map"
            checks.append(("outB (PixelShuffle)", op_decode(outB, fmt)[:4 * M], e, tol))
        else:
            assert op_untouched(outB, fmt, M, C_), "outB: complement written"
            checks.append(("outB", op_decode(outB, fmt)[:M, :C_], exp, tol))
    return checks


def run_groupnorm_act_ex(L, a, bound):
    C_, G, act, B, M, fmt = a["C"], a["G"], a["act"], a["B"], a["M"], a["fmt"]
    g = torch.Generator().manual_seed(C_ + G + M)
    ldx = C_ + 8
    x = torch.randn(B, M, ldx, generator=g) * (1.0 + torch.arange(B).float().reshape(B, 1, 1)) + 0.5 * torch.arange(B).float().reshape(B, 1, 1)
    ga, be = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    eps = 1e-3
    xs = x[:, :, :C_].double()
    grp = xs.reshape(B, M, G, C_ // G)
    stats = torch.zeros(B, 64, dtype=torch.float64)                    # slot b at stats + 64 b: [G][2] = sum, sum of squares
    stats[:, 0:2 * G:2] = grp.sum((1, 3))
    stats[:, 1:2 * G:2] = (grp ** 2).sum((1, 3))
    exp = ACTS[act](F.group_norm(xs.permute(0, 2, 1).unsqueeze(-1), G, ga.double(), be.double(), eps)).squeeze(-1).permute(0, 2, 1)   # per sample
    prior = prior_beta = None
    if a["prior"]:
        prior, prior_beta = torch.rand(B * M, generator=g), torch.randn(C_, generator=g)
        exp = exp + prior.double().reshape(B, M, 1) * prior_beta.double()
    exp = exp.reshape(B * M, C_)
    big = max(1.0, exp.abs().max().item())
    ldf, ldb = C_ + 4, C_ + 8
    W = a["up_w"]
    ldu = a["ldu"] or C_
    outF = torch.full((B * M + 1, ldf), 7.0, device="cuda") if a["outF"] else None
    outB = op_buffer(B * M + 1, ldb, fmt) if a["outB"] else None
    outUp = op_buffer(4 * B * M + 1, ldu, fmt) if W else None
    xd, sd, gd, bd = x.reshape(B * M, ldx).cuda(), stats.cuda(), ga.cuda(), be.cuda()
    pd, pbd = (prior.cuda(), prior_beta.cuda()) if a["prior"] else (None, None)
    L.check(L.lib().uni_groupnorm_act_ex(L.ptr(xd), ldx, L.ptr(sd), L.ptr(gd), L.ptr(bd), eps, B, M, C_, G, act, L.ptr(pd), L.ptr(pbd), L.ptr(outF), ldf,
                                         L.ptr(outB), ldb, L.ptr(outUp), ldu, W, fmt, L.stream_ptr()), "groupnorm_act_ex")
    torch.cuda.synchronize()
    checks = []
    if outF is not None:
        assert op_untouched(outF, 1, B * M, C_), "outF: complement written"
        checks.append(("outF", outF.cpu().double()[:B * M, :C_], exp, vc.B_GN_F32 * big))
    if outB is not None:
        assert op_untouched(outB, fmt, B * M, C_), "outB: complement written"
        checks.append(("outB", op_decode(outB, fmt)[:B * M, :C_], exp, bound * big))
    if outUp is not None:
        H = M // W
        e = exp.reshape(B, H, W, C_).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(4 * B * M, C_)
        assert op_untouched(outUp, fmt, 4 * B * M, C_), "outUp: complement written"
        checks.append(("outUp", op_decode(outUp, fmt)[:4 * B * M, :C_], e, bound * big))
    return checks


def _cast_h2(L, x):
    M, C_ = x.shape
    out = torch.zeros((M, C_), device="cuda", dtype=torch.int32)
    L.check(L.lib().uni_cast_h2(L.ptr(x), C_, L.ptr(out), C_, M, C_, L.stream_ptr()), "cast_h2")
    return out


def _pack_h2(L, w):
    import ctypes as C
    import numpy as np
    N, Cin, KH, KW = w.shape
    K = Cin * KH * KW
    out = np.zeros(((N + 255) // 256 * 256, (K + 63) // 64 * 64), dtype=np.uint32)
    sc = C.c_float(0)
    L.check(L.lib().uni_pack_weight_h2(np.ascontiguousarray(w.float().numpy()).ctypes.data_as(C.c_void_p), N, Cin, KH, KW, out.ctypes.data_as(C.c_void_p),
                                       C.byref(sc)), "pack_h2")
    return torch.from_numpy(out.view(np.int32)).cuda(), sc.value


def run_gemm(L, a, bound):
    """uni_gemm_h2 / uni_gemm_ex as an implicit GEMM against fp64 on the unrounded operands (test_gemm_h2's statement and bound)"""
    Hin, Win, Cin, N, k, stride, pad = a["geo"]
    act, G, h2 = a["act"], a["G"], a["fam"] == "h2"
    g = torch.Generator().manual_seed(Hin * 7 + N + a["cfg"] % 1000 + act)
    x = torch.randn(1, Cin, Hin, Win, generator=g) * 3.0
    w = torch.randn(N, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(N, generator=g) * 0.1 if a["bias"] else None
    ref = F.conv2d(x.double(), w.double(), bias.double() if a["bias"] else None, stride=stride, padding=pad)
    mag = F.conv2d(x.abs().double(), w.abs().double(), None, stride=stride, padding=pad)
    M = ref.shape[2] * ref.shape[3]
    raw, mag = ref.permute(0, 2, 3, 1).reshape(M, N), mag.permute(0, 2, 3, 1).reshape(M, N)
    res = torch.randn(M, N, generator=g) if a["res"] else None
    c0 = a.get("act_col0", 0)
    exp = torch.cat([raw[:, :c0], ACTS[act](raw[:, c0:])], 1) + (res.double() if a["res"] else 0)      # the activation on columns >= c0
    rows = x.permute(0, 2, 3, 1).reshape(Hin * Win, Cin).contiguous().cuda()
    outF = torch.full((M, N), float("nan"), device="cuda") if a["outF"] else None
    stats = torch.zeros(64, device="cuda", dtype=torch.float64) if G else None
    bias_d, res_d = (bias.cuda() if a["bias"] else None), (res.cuda() if a["res"] else None)
    if h2:
        A = _cast_h2(L, rows)
        Wp, wscale = _pack_h2(L, w)
        outB = torch.zeros((M, N), device="cuda", dtype=torch.int32) if a["outB"] else None
        if c0:
            L.check(L.lib().uni_gemm_ex(L.ptr(A), Cin, L.ptr(Wp), wscale, 2, M, N, Hin, Win, Cin, k, k, stride, pad, L.ptr(bias_d), act, c0, L.ptr(res_d), N,
                                        L.ptr(outF), N, L.ptr(outB), N, L.ptr(stats), (N // G) if G else 0, a["cfg"], L.stream_ptr()), "gemm_ex")
        else:
            L.check(L.lib().uni_gemm_h2(L.ptr(A), Cin, L.ptr(Wp), wscale, M, N, Hin, Win, Cin, k, k, stride, pad, L.ptr(bias_d), act, L.ptr(res_d), N,
                                        L.ptr(outF), N, L.ptr(outB), N, L.ptr(stats), (N // G) if G else 0, a["cfg"], L.stream_ptr()), "gemm_h2")
    else:
        K = Cin * k * k
        Wp = torch.zeros(((N + 255) // 256 * 256, (K + 63) // 64 * 64))
        Wp[:N, :K] = w.permute(0, 2, 3, 1).reshape(N, K)              # k = (ky * KW + kx) * Cin + c
        Wp = Wp.cuda()
        outB = torch.full((M, N), float("nan"), device="cuda") if a["outB"] else None
        L.check(L.lib().uni_gemm_ex(L.ptr(rows), Cin, L.ptr(Wp), 1.0, 1, M, N, Hin, Win, Cin, k, k, stride, pad, L.ptr(bias_d), act, c0, L.ptr(res_d), N,
                                    L.ptr(outF), N, L.ptr(outB), N, L.ptr(stats), (N // G) if G else 0, a["cfg"], L.stream_ptr()), "gemm_ex")
    torch.cuda.synchronize()
    tol = (mag * bound + 1e-6) * 1.2
    checks = []
    if outF is not None:
        checks.append(("outF", outF.cpu().double(), exp, tol))
    if outB is not None:
        checks.append(("outB", op_decode(outB, 2 if h2 else 1), exp, tol + (exp.abs() * 2.0 ** -21 if h2 else 0)))
    if G:
        grp = raw.reshape(M, G, N // G)
        s_ref = torch.stack([grp.sum((0, 2)), (grp ** 2).sum((0, 2))], 1)
        s_got = stats.cpu()[:2 * G].reshape(G, 2)
        assert torch.allclose(s_got, s_ref, rtol=2e-5, atol=2e-2), (s_got - s_ref).abs().max()       # test_gemm_h2
    return checks


def run_gemm_stacked(L, a, bound):
    """uni_gemm_stacked: B stacked samples and / or the outF row remap against the batched fp64 conv (vc.gemm_stacked_problem); every buffer is
    pre-filled, and what the kernel must not write -- the gaps between the remapped images, the columns >= N, the rows behind, the unused part
    of every statistics slot -- must still hold the fill"""
    Hin, Win, Cin, N, k, stride, pad = a["geo"]
    B, act, G, c0, h2 = a["B"], a["act"], a["G"], a["act_col0"], a["fam"] == "h2"
    P = vc.gemm_stacked_problem(a, bound)
    M, exp, tol = P["M"], P["exp"], P["tol"]
    rows = P["x"].permute(0, 2, 3, 1).reshape(B * Hin * Win, Cin).contiguous().cuda()
    FILL = -777.0
    ldf, ldb, ldr = a["ldf"], N + 8, N + 4
    outF = torch.full((a["outF_rows"], ldf), FILL, device="cuda") if a["outF"] else None
    stats = torch.zeros(64 * (B + 1), device="cuda", dtype=torch.float64) if G else None      # one slot more than the launch may touch
    bias_d, res_d = (P["bias"].cuda() if a["bias"] else None), (P["res"].cuda() if a["res"] else None)
    if h2:
        A = _cast_h2(L, rows)
        Wp, wscale = _pack_h2(L, P["w"])
    else:
        K = Cin * k * k
        Wp = torch.zeros(((N + 255) // 256 * 256, (K + 63) // 64 * 64))
        Wp[:N, :K] = P["w"].permute(0, 2, 3, 1).reshape(N, K)
        A, Wp, wscale = rows, Wp.cuda(), 1.0
    ofmt = 2 if h2 else 1
    outB = op_buffer(M + 1, ldb, ofmt) if a["outB"] else None
    L.check(L.lib().uni_gemm_stacked(L.ptr(A), Cin, L.ptr(Wp), wscale, ofmt, B, M, N, Hin, Win, Cin, k, k, stride, pad, L.ptr(bias_d), act, c0, L.ptr(res_d), ldr,
                                     L.ptr(outF), ldf, a["out_hw"], a["out_stride"], a["out_off"], a["outF_rows"], L.ptr(outB), ldb, L.ptr(stats),
                                     (N // G) if G else 0, a["splitk"], a["cfg"], L.stream_ptr()), "gemm_stacked")
    torch.cuda.synchronize()
    checks = []
    if outF is not None:
        got = outF.cpu().double()
        written = torch.zeros(a["outF_rows"], ldf, dtype=torch.bool)
        written[P["orow"], :N] = True
        assert bool((got[~written] == FILL).all()), "outF: written outside the (remapped) rows x N columns"
        checks.append(("outF", got[P["orow"], :N], exp, tol))
    if outB is not None:
        assert op_untouched(outB, ofmt, M, N), "outB: complement written"
        checks.append(("outB", op_decode(outB, ofmt)[:M, :N], exp, tol + (exp.abs() * 2.0 ** -21 if h2 else 0)))
    if G:
        st = stats.cpu().reshape(B + 1, 64)
        assert bool((st[:B, 2 * G:] == 0).all()) and bool((st[B] == 0).all()), "statistics: written outside the [G][2] sums of the B slots"
        checks.append(("stats", st[:B, :2 * G].reshape(B, G, 2), P["stats_ref"], P["stats_tol"]))
    return checks


def run_corr(L, a, bound):
    from unicorn_amd.ops import corr_softmax_pv, corr_softmax_pv_batched
    B, R, Q, K, prec = a["B"], a["R"], a["Q"], a["K"], a["prec"]
    g = torch.Generator().manual_seed(R + Q + B)
    nb = max(B, 1)
    er, ec = torch.randn(nb, 128, R, generator=g) * 0.6, torch.randn(nb, 128, Q, generator=g) * 0.6
    v = torch.rand(K, R, generator=g)
    exp = torch.stack([v.double() @ torch.softmax(er[b].double().t() @ ec[b].double(), 0) for b in range(nb)])
    if B:
        out = corr_softmax_pv_batched(er.cuda(), ec.cuda(), v.cuda(), precision=prec)
    else:
        out = corr_softmax_pv(er[0].cuda(), ec[0].cuda(), v.cuda(), precision=prec)[None]
    return [("out", out.cpu().double(), exp, bound)]


def run_cast(L, a, bound):
    M, C_, fmt = a["M"], a["C"], a["fmt"]
    g = torch.Generator().manual_seed(M)
    x = torch.randn(M, C_ + 8, generator=g)
    x[1] *= 1e-3
    x[2] *= 300.0
    xd = x.cuda()
    out = op_buffer(M + 1, C_ + 8, fmt)
    fn = L.lib().uni_cast_h2 if fmt == 2 else L.lib().uni_cast_f32
    L.check(fn(L.ptr(xd), C_ + 8, L.ptr(out), C_ + 8, M, C_, L.stream_ptr()), "cast")
    torch.cuda.synchronize()
    assert op_untouched(out, fmt, M, C_), "cast: complement written"
    e = x[:, :C_].double()
    return [("out", op_decode(out, fmt)[:M, :C_], e, (e.abs() * bound + 2.0 ** -25) if fmt == 2 else torch.zeros_like(e))]


def run_stem(L, a, bound):
    import unicorn_oracle as uo
    C_, B, H, W = a["C"], a["B"], a["H"], a["W"]
    g = torch.Generator().manual_seed(C_ + B)
    img = torch.rand(B, 3, H, W, generator=g) * 255
    w = torch.randn(C_, 3, 4, 4, generator=g) / 48 ** 0.5
    b, ga, be = torch.randn(C_, generator=g) * 0.1, 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    exp = uo.ln_channels_first(F.conv2d(img.double(), w.double(), b.double(), stride=4), ga.double(), be.double()).permute(0, 2, 3, 1).reshape(-1, C_)
    wt = w.reshape(C_, 48).t().contiguous().cuda()
    rows = B * (H // 4) * (W // 4)
    out = torch.full((rows + 1, C_), 7.0, device="cuda")
    imd, bd, gd, bed = img.cuda(), b.cuda(), ga.cuda(), be.cuda()
    L.check(L.lib().uni_stem_ex(L.ptr(imd), B, H, W, L.ptr(wt), L.ptr(bd), L.ptr(gd), L.ptr(bed), C_, L.ptr(out), L.stream_ptr()), "stem_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, 1, rows, C_)
    return [("out", out.cpu().double()[:rows], exp, bound * max(1.0, exp.abs().max().item()))]


def run_mlp(L, a, bound):
    import ctypes as C
    import numpy as np
    C_, M, layout = a["C"], a["M"], a["layout"]
    g = torch.Generator().manual_seed(C_ + M)
    x = torch.randn(M, C_, generator=g) * 1.5
    w1, b1 = torch.randn(4 * C_, C_, generator=g) * 0.05, torch.randn(4 * C_, generator=g) * 0.2
    w2, b2 = torch.randn(C_, 4 * C_, generator=g) * 0.05, torch.randn(C_, generator=g) * 0.2
    gamma = torch.rand(C_, generator=g) + 0.5
    res = torch.randn(M, C_, generator=g) * 3.0
    A = _cast_h2(L, x.cuda())
    a_dec = op_decode(A, 2)
    ref = res.double() + gamma.double() * (F.gelu(a_dec @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double())
    blob = np.zeros(L.lib().uni_mlp_blob_bytes(C_) // 2, dtype=np.uint16)
    s1, s2 = C.c_float(0), C.c_float(0)
    w1c, w2c, gc = (np.ascontiguousarray(t.float().numpy()) for t in (w1, w2, gamma))
    L.check(L.lib().uni_mlp_pack(w1c.ctypes.data_as(C.c_void_p), w2c.ctypes.data_as(C.c_void_p), gc.ctypes.data_as(C.c_void_p), C_, layout,
                                 blob.ctypes.data_as(C.c_void_p), C.byref(s1), C.byref(s2)), "mlp_pack")
    blob_d = torch.from_numpy(blob.view(np.int16)).cuda()
    out = torch.full((M + 64, C_), 777.0, device="cuda")
    out[:M] = res.cuda()
    outb = torch.zeros((M + 64, C_), device="cuda", dtype=torch.int32) if a["outB"] else None
    b1d, b2d = b1.cuda(), (gamma * b2).cuda()
    L.check(L.lib().uni_mlp_fused(L.ptr(A), C_, L.ptr(blob_d), L.ptr(b1d), L.ptr(b2d), s1.value, s2.value, L.ptr(out), C_, L.ptr(out), C_, L.ptr(outb), C_, M, C_,
                                  layout, L.stream_ptr()), "mlp_fused")
    torch.cuda.synchronize()
    assert (out[M:] == 777.0).all() and (outb is None or (outb[M:] == 0).all())
    scale = max(1.0, ref.abs().max().item())
    checks = [("out", out[:M].cpu().double(), ref, bound * scale)]
    if outb is not None:
        checks.append(("out_h2", op_decode(outb[:M], 2), out[:M].cpu().double(), 1e-6 * scale))      # test_mlp_fused: the copy against the fp32 output
    return checks


def _msda_problem(a):
    """-> value (B, Lq, 256), offaw (B Lq, 192), fp64 reference (B Lq, 256) of the fused sampler"""
    import unicorn_oracle as uo
    B, h, w = a["B"], a["h"], a["w"]
    g = torch.Generator().manual_seed(B * 100 + h)
    Lq = 2 * h * w
    value = torch.randn(B, Lq, 256, generator=g)
    off = torch.randn(B, Lq, 8, 2, 4, 2, generator=g) * 6.0
    off[:, :5] *= 30.0
    logits = torch.randn(B, Lq, 8, 8, generator=g) * 2.0
    offaw = torch.cat([off.reshape(B * Lq, 128), logits.reshape(B * Lq, 64)], 1).contiguous()
    ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ref = torch.stack([(jj.reshape(-1) + 0.5) / w, (ii.reshape(-1) + 0.5) / h], -1).repeat(2, 1).double()
    loc = ref[None, :, None, None, None, :] + off.double() / torch.tensor([w, h], dtype=torch.float64)
    attn = torch.softmax(logits.double(), -1).view(B, Lq, 8, 2, 4)
    want = uo.msda_core(value.double().view(B, Lq, 8, 32), [(h, w), (h, w)], loc, attn).reshape(B * Lq, 256)
    return value, offaw, want


def run_msda_tokens(L, a, bound):
    B, h, w = a["B"], a["h"], a["w"]
    value, offaw, want = _msda_problem(a)
    out = torch.empty(B * 2 * h * w, 256, device="cuda")
    vd, od = value.cuda(), offaw.cuda()
    L.check(L.lib().uni_msda_tokens(L.ptr(vd), L.ptr(od), 192, B, h, w, L.ptr(out), L.stream_ptr()), "uni_msda_tokens")
    torch.cuda.synchronize()
    return [("out", out.cpu().double(), want, bound + 1e-4 * want.abs())]          # allclose(rtol 1e-4, atol 2e-5)


# ------------------------------------------------------------------------------------------------ the glue launchers between context buffers
def _op_tol(e, fmt, bound):
    """operand rows against the fp64 value they store: the restated row bound of the format, exact for fp32 (as run_cast)"""
    return torch.zeros_like(e) if fmt == 1 else bound * max(1.0, e.abs().max().item())


def run_msda_tokens_ex(L, a, bound):
    B, h, w, fmt = a["B"], a["h"], a["w"], a["fmt"]
    value, offaw, want = _msda_problem(a)
    M = B * 2 * h * w
    out = op_buffer(M + 1, 256, fmt)
    vd, od = value.cuda(), offaw.cuda()
    L.check(L.lib().uni_msda_tokens_ex(L.ptr(vd), L.ptr(od), 192, B, h, w, L.ptr(out), fmt, L.stream_ptr()), "uni_msda_tokens_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, fmt, M, 256), "msda_tokens_ex wrote behind its output"
    return [("out", op_decode(out, fmt)[:M], want, bound * max(1.0, want.abs().max().item()))]


def run_cast_pair(L, a, bound):
    B, hw, C_, fmt = a["B"], a["h"] * a["w"], a["C"], a["fmt"]
    g = torch.Generator().manual_seed(B + C_)
    x = torch.randn(2, B, hw, C_, generator=g) * (1.0 + torch.arange(2 * B).float().reshape(2, B, 1, 1))      # every (frame, sample) on its own scale
    e = x.permute(1, 0, 2, 3).reshape(2 * B * hw, C_).double()                                                # [B][2][hw][C]
    x0, x1 = x[0].contiguous().cuda(), x[1].contiguous().cuda()
    out = op_buffer(2 * B * hw + 1, C_, fmt)
    L.check(L.lib().uni_cast_operand_pair_ex(L.ptr(x0), L.ptr(x1), L.ptr(out), B, hw, C_, fmt, L.stream_ptr()), "cast_operand_pair_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, fmt, 2 * B * hw, C_), "cast_operand_pair_ex wrote behind its output"
    return [("out", op_decode(out, fmt)[:2 * B * hw], e, _op_tol(e, fmt, bound))]


def run_pixel_shuffle(L, a, bound):
    B, h, w, C_, fmt = a["B"], a["h"], a["w"], a["C"], a["fmt"]
    g = torch.Generator().manual_seed(B + C_ + 1)
    x = torch.randn(B, C_, h, w, generator=g) * (1.0 + torch.arange(B).float().reshape(B, 1, 1, 1))
    e = F.pixel_shuffle(x.double(), 2).permute(0, 2, 3, 1).reshape(4 * B * h * w, C_ // 4)
    xd = x.permute(0, 2, 3, 1).contiguous().cuda()
    out = op_buffer(4 * B * h * w + 8, C_ // 4, fmt)
    L.check(L.lib().uni_pixel_shuffle_ex(L.ptr(xd), L.ptr(out), B, h, w, C_, fmt, L.stream_ptr()), "pixel_shuffle_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, fmt, 4 * B * h * w, C_ // 4), "pixel_shuffle_ex wrote behind its output"
    return [("out", op_decode(out, fmt)[:4 * B * h * w], e, _op_tol(e, fmt, bound))]


def run_add_pos(L, a, bound):
    B, hw, C_, fmt = a["B"], a["h"] * a["w"], a["C"], a["fmt"]
    g = torch.Generator().manual_seed(B + C_ + 2)
    src = torch.randn(B, 2, hw, C_, generator=g) * (1.0 + torch.arange(B).float().reshape(B, 1, 1, 1))
    pos = torch.randn(2, hw, C_, generator=g)                  # frame 0 / 1, shared by the batch
    lvl = torch.randn(2, C_, generator=g)
    e = (src.double() + pos.double()[None] + lvl.double()[None, :, None, :]).reshape(2 * B * hw, C_)
    sd, p0, p1, ld = src.cuda(), pos[0].contiguous().cuda(), pos[1].contiguous().cuda(), lvl.cuda()
    out = op_buffer(2 * B * hw + 1, C_, fmt)
    L.check(L.lib().uni_add_pos_ex(L.ptr(sd), L.ptr(p0), L.ptr(p1), L.ptr(ld), L.ptr(out), B, hw, C_, fmt, L.stream_ptr()), "add_pos_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, fmt, 2 * B * hw, C_), "add_pos_ex wrote behind its output"
    got = op_decode(out, fmt)[:2 * B * hw]
    if fmt != 1:
        return [("out", got, e, _op_tol(e, fmt, bound))]
    # fp32 rows: the sum itself is rounded, so "exact" is the fp32 evaluation in the kernel's association src + (pos + lvl) -- correctly rounded
    # additions, the same bits on any IEEE machine -- and that evaluation lies within two roundings, 2^-23 (|src| + |pos| + |lvl|), of fp64
    e32 = (src + (pos[None] + lvl[None, :, None, :])).reshape(2 * B * hw, C_).double()
    mag = (src.abs().double() + pos.abs().double()[None] + lvl.abs().double()[None, :, None, :]).reshape(2 * B * hw, C_)
    return [("out (fp64 sum)", got, e, 2.0 ** -23 * mag + 1e-30), ("out (fp32 sum, exact)", got, e32, torch.zeros_like(e32))]


def _fp32_yardstick(what, r32, r64, cap):
    """the project's yardstick for fp32 results of fp32 arithmetic: 4 x the distance of the oracle's own fp32 evaluation from its fp64
    evaluation of the same inputs (CPU), capped by the case's restated bound (relative to max(1, max |reference|))"""
    d = (r32.double() - r64).abs().max().item()
    tol = min(4.0 * d, cap * max(1.0, r64.abs().max().item()))
    print("%s: oracle fp32 - fp64 %.3e -> tolerance %.3e" % (what, d, tol))
    return tol


def run_add_aligned_bilinear(L, a, bound):
    import unicorn_oracle as uo
    B, h, w, C_, f = a["B"], a["h"], a["w"], a["C"], a["factor"]
    g = torch.Generator().manual_seed(B + C_ + f)
    src = torch.randn(B, C_, h, w, generator=g) * (1.0 + torch.arange(B).float().reshape(B, 1, 1, 1))
    dst = torch.randn(B, C_, f * h, f * w, generator=g)
    r64 = dst.double() + uo.aligned_bilinear(src.double(), f)                # per sample: the oracle pads / interpolates every (h, w) map on its own
    r32 = dst + uo.aligned_bilinear(src, f)
    rows = B * f * h * f * w
    buf = torch.full((rows + 1, C_), 7.0, device="cuda")
    buf[:rows] = dst.permute(0, 2, 3, 1).reshape(rows, C_).cuda()
    sd = src.permute(0, 2, 3, 1).contiguous().cuda()
    L.check(L.lib().uni_add_aligned_bilinear_ex(L.ptr(sd), B, h, w, C_, f, L.ptr(buf), L.stream_ptr()), "add_aligned_bilinear_ex")
    torch.cuda.synchronize()
    assert op_untouched(buf, 1, rows, C_), "add_aligned_bilinear_ex wrote behind its output"
    flat = lambda t: t.permute(0, 2, 3, 1).reshape(rows, C_)
    return [("dst", buf.cpu().double()[:rows], flat(r64), _fp32_yardstick("add_aligned_bilinear", flat(r32), flat(r64), bound))]


def run_pos_embed(L, a, bound):
    import unicorn_oracle as uo
    h, w, sz, nf = a["h"], a["w"], a["sz"], a["nf"]
    g = torch.Generator().manual_seed(sz + nf)
    P = {"pos_emb.row_embed.weight": torch.rand(sz, nf, generator=g), "pos_emb.col_embed.weight": torch.rand(sz, nf, generator=g)}      # nn.init.uniform_
    flat = lambda t: t[0].permute(1, 2, 0).reshape(h * w, 2 * nf)
    r64, r32 = flat(uo.pos_embed({k: v.double() for k, v in P.items()}, h, w)), flat(uo.pos_embed(P, h, w))
    out = torch.full((h * w + 1, 2 * nf), 7.0, device="cuda")
    rd, cd = P["pos_emb.row_embed.weight"].cuda(), P["pos_emb.col_embed.weight"].cuda()
    L.check(L.lib().uni_pos_embed_ex(L.ptr(rd), L.ptr(cd), sz, nf, h, w, L.ptr(out), L.stream_ptr()), "pos_embed_ex")
    torch.cuda.synchronize()
    assert op_untouched(out, 1, h * w, 2 * nf), "pos_embed_ex wrote behind its output"
    return [("out", out.cpu().double()[:h * w], r64, _fp32_yardstick("pos_embed", r32, r64, bound))]


def run_prior_pyramid(L, a, bound):
    import unicorn_oracle as uo
    from unicorn_amd.ops import prior_pyramid
    c = torch.rand(1, a["K"], a["H8"], a["W8"], generator=torch.Generator().manual_seed(9))
    got, ref = prior_pyramid(c.cuda()), uo.prior_pyramid(c.double())
    return [("level %d" % i, x.cpu().double(), y, bound) for i, (x, y) in enumerate(zip(got, ref))]


def run_decode(L, a, bound):
    import unicorn_oracle as uo
    B, H, W, nch = a["B"], a["H"], a["W"], a["nch"]
    g = torch.Generator().manual_seed(2)
    levels = [torch.randn(B, nch, H // s_, W // s_, generator=g) for s_ in (8, 16, 32)]
    exp, _ = uo.decode_outputs([t.double() for t in levels])
    d = torch.cat([t.flatten(2) for t in levels], 2).permute(0, 2, 1).contiguous().cuda()
    L.check(L.lib().uni_decode_outputs(L.ptr(d), B, H, W, nch, L.stream_ptr()), "decode")
    torch.cuda.synchronize()
    return [("out", d.cpu().double(), exp.double(), bound + 1e-6 * exp.double().abs())]          # allclose(rtol 1e-6, atol 1e-5)


def run_condinst(L, a, bound):
    import unicorn_oracle as uo
    from unicorn_amd.ops import condinst_masks
    n, H8, W8 = a["n"], a["H8"], a["W8"]
    g = torch.Generator().manual_seed(8)
    cfg = uo.CONFIGS["unicorn_track_tiny_mask"]
    mf, um = torch.randn(1, 8, H8, W8, generator=g), torch.randn(1, 144, H8, W8, generator=g)
    params = torch.randn(n, 169, generator=g) * 0.5
    loc = torch.rand(n, 2, generator=g) * torch.tensor([W8 * 8.0, H8 * 8.0])
    lvl = torch.arange(n) % 3
    ref = uo.aligned_bilinear(uo.dynamic_mask_head(cfg, mf.double(), params.double(), loc.double(), lvl, um.double()), 2)
    got = condinst_masks(mf.cuda(), um.cuda(), params.cuda(), loc.cuda(), lvl, 4, 2)
    return [("masks", got.cpu().double(), ref.double(), bound)]


RUNNERS = {"uni_dwconv7_ln_ex": run_dwconv7_ln_ex, "uni_layernorm_ex": run_layernorm_ex, "uni_groupnorm_act_ex": run_groupnorm_act_ex,
           "uni_gemm_h2": run_gemm, "uni_gemm_ex": run_gemm, "uni_gemm_stacked": run_gemm_stacked, "uni_corr_softmax_pv": run_corr, "uni_corr_softmax_pv_batched": run_corr,
           "uni_cast_h2": run_cast, "uni_cast_f32": run_cast, "uni_stem_ex": run_stem, "uni_mlp_fused": run_mlp, "uni_msda_tokens": run_msda_tokens,
           "uni_msda_tokens_ex": run_msda_tokens_ex, "uni_cast_operand_pair_ex": run_cast_pair, "uni_pixel_shuffle_ex": run_pixel_shuffle,
           "uni_add_pos_ex": run_add_pos, "uni_add_aligned_bilinear_ex": run_add_aligned_bilinear, "uni_pos_embed_ex": run_pos_embed,
           "uni_prior_pyramid": run_prior_pyramid, "uni_decode_outputs": run_decode, "uni_condinst_masks": run_condinst}


def run_case(L, tag):
    """the case of `tag`: traced call, tag assertion, parity checks; returns the printed report"""
    case = vc.CASES[tag]
    checks, tags = traced(L, lambda: RUNNERS[case["entry"]](L, case["args"], case["bound"]))
    assert tag in tags, "the case does not reach its variant: launcher emitted %s" % sorted(tags)
    lines = []
    for what, got, exp, tol in checks:
        assert torch.isfinite(got).all(), what
        err = (got - exp).abs()
        if torch.is_tensor(tol):            # element-wise tolerance (sum |a||w| scale of a GEMM, allclose-style bounds)
            if bool((tol > 0).all()):
                lines.append("%s: %s max err / tolerance %.3f" % (tag, what, (err / tol).max().item()))
            else:                           # exact where the tolerance is 0
                lines.append("%s: %s max err %.3e (held to the exact value)" % (tag, what, err.max().item()))
            ok = bool((err <= tol).all())
        else:
            lines.append("%s: %s max err %.3e (tolerance %.3e)" % (tag, what, err.max().item(), tol))
            ok = err.max().item() < tol
        print(lines[-1])
        assert ok, lines[-1]
    return lines


# ------------------------------------------------------------------------------------------------ 1. the trace itself
def _dwln_call(L):
    C_, H, W = 96, 6, 8
    x = torch.randn(H, W, C_, device="cuda")
    w = torch.randn(49, C_, device="cuda")
    v = torch.randn(C_, device="cuda")
    out = torch.empty(H * W, C_, device="cuda")
    L.check(L.lib().uni_dwconv7_ln_ex(L.ptr(x), L.ptr(w), L.ptr(v), L.ptr(v), L.ptr(v), 1e-6, 1, H, W, C_, L.ptr(out), 1, L.stream_ptr()), "dwln_ex")
    torch.cuda.synchronize()


def test_trace_is_off_by_default_and_counts_one_tag_per_launch(L):
    lib = L.lib()
    lib.uni_variant_trace(1)              # (an earlier test of the process may have left tags behind: start from an empty, stopped trace)
    lib.uni_variant_trace(0)
    _dwln_call(L)
    assert vc.read_trace(lib) == {}, "a launch with the trace off left a tag"
    _, tags = traced(L, lambda: _dwln_call(L))
    assert tags == {"dwconv7_ln ln<PX=4> CG=24 S=10 fmt=f32 batched=0": 1}, tags
    assert vc.read_trace(lib) == tags, "stopping the trace must keep the tags readable"
    _, tags = traced(L, lambda: (_dwln_call(L), _dwln_call(L)))
    assert list(tags.values()) == [2], tags
    lib.uni_variant_trace(1)
    assert vc.read_trace(lib) == {}, "uni_variant_trace(1) must clear the trace"
    lib.uni_variant_trace(0)
    assert lib.uni_variant_trace_read(None, 0) == 1      # the empty text: its NUL


def test_trace_split_k_gives_partial_and_reduce_tags(L):
    import ctypes as C
    import numpy as np
    M, N, K = 256, 256, 1024
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).cuda()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).reshape(N, K, 1, 1)
    A = torch.zeros((M, K), device="cuda", dtype=torch.int32)
    L.check(L.lib().uni_cast_h2(L.ptr(x), K, L.ptr(A), K, M, K, L.stream_ptr()), "cast_h2")
    Wp = np.zeros((256, K), dtype=np.uint32)
    sc = C.c_float(0)
    L.check(L.lib().uni_pack_weight_h2(np.ascontiguousarray(w.numpy()).ctypes.data_as(C.c_void_p), N, K, 1, 1, Wp.ctypes.data_as(C.c_void_p), C.byref(sc)), "pack_h2")
    Wd = torch.from_numpy(Wp.view(np.int32)).cuda()
    out = torch.full((M, N), float("nan"), device="cuda")
    call = lambda: L.check(L.lib().uni_gemm_h2(L.ptr(A), K, L.ptr(Wd), sc.value, M, N, M, 1, K, 1, 1, 1, 0, None, 0, None, N, L.ptr(out), N, None, N, None, 0,
                                               4 * 1000000 + 22, L.stream_ptr()), "gemm_h2 split-K")
    _, tags = traced(L, call)
    part = [t for t in tags if t.startswith("gemm:h2 cfg=2222 ") and " splitk=1 " in t]
    red = [t for t in tags if t.startswith("gemm:splitk_reduce ")]
    assert len(tags) == 2 and len(part) == 1 and len(red) == 1 and set(tags.values()) == {1}, tags
    exp = x.double() @ w.reshape(N, K).double().cuda().t()
    assert (out.double() - exp).abs().max().item() < 1e-4 * exp.abs().max().item()


def test_gemm_stacked_rejects_bad_arguments_before_any_launch(L):
    """uni_gemm_stacked checks every argument before it launches: a bad sample count, remap or split-K request is an error code with a
    message, no tag is traced and no output element changes.  (Every buffer here is large enough for any reading of the arguments.)  The
    tightest valid remap -- the last remapped row is the last row of out_f32 -- is accepted."""
    lib = L.lib()
    B, Hin, Win, Cin, N = 5, 7, 9, 128, 192
    M, rows, ldf = B * Hin * Win, 1000, N + 4
    A = torch.zeros(M, Cin, device="cuda")
    Wp = torch.zeros(256, 128, device="cuda")
    outF = torch.full((rows, ldf), -777.0, device="cuda")
    stats = torch.zeros(64 * B, device="cuda", dtype=torch.float64)
    ok = dict(fmt=1, B=B, M=M, out_hw=0, out_stride=0, out_off=0, outF_rows=rows, act=0, stats=None, cpg=0, splitk=0)
    remap = dict(out_hw=63, out_stride=200, out_off=10)             # last row: 4 * 200 + 10 + 63 = 873 rows needed

    def call(**kw):
        a = dict(ok, **kw)
        return lib.uni_gemm_stacked(L.ptr(A), Cin, L.ptr(Wp), 1.0, a["fmt"], a["B"], a["M"], N, Hin, Win, Cin, 1, 1, 1, 0, None, a["act"], 0, None, 0, L.ptr(outF), ldf,
                                    a["out_hw"], a["out_stride"], a["out_off"], a["outF_rows"], None, 0, L.ptr(a["stats"]), a["cpg"], a["splitk"], 0, L.stream_ptr())

    bad = {"B = 0": dict(B=0), "B = -1": dict(B=-1), "B = 128": dict(B=128), "M one short": dict(M=M - 1), "B = 3 does not match the map": dict(B=3),
           "remap one row behind outF_rows": dict(remap, outF_rows=872), "out_hw does not divide M": dict(remap, out_hw=64),
           "out_stride < out_hw": dict(remap, out_stride=62), "out_off < 0": dict(remap, out_off=-1), "outF_rows < M": dict(outF_rows=M - 1),
           "split-K in fp32": dict(splitk=2), "split-K with an activation": dict(fmt=2, splitk=2, act=1), "split-K 65": dict(fmt=2, splitk=65),
           "split-K with a remap": dict(remap, fmt=2, splitk=2), "statistics without cpg": dict(stats=stats), "cpg does not divide N": dict(stats=stats, cpg=5),
           "48 groups": dict(stats=stats, cpg=4), "statistics with an activation": dict(stats=stats, cpg=12, act=1)}

    def all_bad():
        for what, kw in bad.items():
            assert call(**kw) != 0, "accepted: " + what
            assert lib.uni_last_error(), what
    _, tags = traced(L, all_bad)
    assert tags == {}, tags
    assert bool((outF == -777.0).all()) and bool((stats == 0).all())
    L.check(call(**dict(remap, outF_rows=873)), "gemm_stacked (tightest valid remap)")
    torch.cuda.synchronize()
    written = torch.zeros(rows, dtype=torch.bool)
    written[vc.gemm_stacked_problem(dict(geo=(Hin, Win, Cin, N, 1, 1, 0), B=B, act=0, G=0, act_col0=0, cfg=0, bias=False, res=False, **remap))["orow"]] = True
    got = outF.cpu()
    assert bool((got[written][:, :N] == 0).all()) and bool((got[written][:, N:] == -777.0).all()) and bool((got[~written] == -777.0).all())


# ------------------------------------------------------------------------------------------------ 2. census
def _sot_step(m, cfg, d_pre, lbs, cur, corr_prec):
    from unicorn_amd.ops import condinst_masks, corr_softmax_pv, corr_softmax_pv_batched, prior_pyramid
    B = cur.shape[0]
    fpn, d_cur = m(imgs=cur, mode="backbone")
    f_pre, f_cur = m(seq_dict0=d_pre, seq_dict1=d_cur, mode="interaction")
    e_pre, e_cur = m(feat=f_pre, mode="upsample"), m(feat=f_cur, mode="upsample")
    if B > 1:
        pred = corr_softmax_pv_batched(e_pre, e_cur, lbs, precision=corr_prec)
    else:
        pred = corr_softmax_pv(e_pre[0].flatten(-2), e_cur[0].flatten(-2), lbs, precision=corr_prec)
    coarse = pred.view(1, B, d_cur["h"] * 2, d_cur["w"] * 2)
    pri = tuple(t.transpose(0, 1).contiguous() for t in prior_pyramid(coarse))
    head = m.head(fpn, pri, mode="sot")
    outs = [coarse, head[0] if cfg.mask else head]
    if cfg.mask:                         # CondInst masks of four anchors of the first frame
        idx = torch.arange(0, 2000, 500)
        outs.append(condinst_masks(head[4][:1], head[5][:1], head[2][0][idx.cuda()], head[1][idx.cuda()], head[3][0][idx], cfg.up_rate, cfg.d_rate))
    return outs


@pytest.fixture(scope="module")
def census(L):
    """workload -> {tag: count}; synthetic weights, no CPU oracle: dispatch depends on shapes only"""
    import synth
    import unicorn_oracle as uo
    from unicorn_amd.models import Unicorn
    from unicorn_amd.ops import label_map_s8
    out = {}
    for name, prec, H, W, Bs in (("unicorn_track_large", "f16x2", 800, 1280, (16, 1)), ("unicorn_track_tiny_mask", "f16x2", 352, 608, (3,)),
                                 ("unicorn_track_tiny_mask", "fp32", 320, 320, (1,))):
        cfg = uo.CONFIGS[name]
        m = Unicorn(name, precision=prec).cuda()
        missing, _ = m.load_state_dict(synth.synth_state_dict(cfg), strict=False)
        assert not missing, missing[:5]
        m.eval()
        frames, box = synth.synth_clip(H, W, 3, seed=1)
        with torch.no_grad():
            _, d_pre = m(imgs=frames[0].cuda(), mode="backbone")
            lbs = label_map_s8(box, H, W, "cuda")
            for B in Bs:
                cur = torch.cat([frames[1 + b % 2] for b in range(B)], 0).cuda()
                outs, tags = traced(L, lambda: _sot_step(m, cfg, d_pre, lbs, cur, 0 if prec == "fp32" else 2))
                for o in outs:
                    assert torch.isfinite(o).all()
                out["%s %s %dx%d B=%d" % (name, prec, H, W, B)] = tags
        del m
        torch.cuda.empty_cache()
    return out


def _write_census(census, uncovered, not_dispatched):
    out = guard.results_dir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "variant_census.json"), "w") as f:
        json.dump({"workloads": census, "uncovered": uncovered, "not_dispatched": not_dispatched}, f, indent=1, sort_keys=True)


def test_census_closure_every_dispatched_variant_has_a_parity_case(census):
    """Every tag the engine dispatched on the census workloads is a key of CASES or one of the context-only launchers of CTX_ONLY.  The reverse
    direction is a report: cases whose variant no census workload dispatched are listed under not_dispatched in the JSON."""
    seen = set()
    for tags in census.values():
        assert tags, "a census workload recorded no launch"
        seen |= set(tags)
    uncovered = sorted(t for t in seen if t not in vc.CASES and not vc.ctx_only_match(t))
    # a context-only GEMM tag parks only the row-remap / stacked-sample switch: the instantiation it names must have a one-sample case
    uncovered += sorted({"%s   <- one-sample twin of the context-only %s" % (vc.gemm_twin(t), t) for t in seen
                         if vc.ctx_only_match(t) and t.startswith("gemm:") and vc.gemm_twin(t) not in vc.CASES})
    not_dispatched = sorted(t for t in vc.CASES if t not in seen)
    _write_census(census, uncovered, not_dispatched)
    assert not uncovered, "%d dispatched variants without a parity case:\n%s" % (len(uncovered), "\n".join(uncovered))


# ------------------------------------------------------------------------------------------------ 3. one parity case per tag
@pytest.mark.parametrize("tag", sorted(vc.CASES))
def test_case_reaches_its_variant_and_matches_fp64(L, tag):
    run_case(L, tag)
