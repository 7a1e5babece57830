"""Guard-band tests: every context-free C-ABI kernel stays inside its buffers at ragged shapes and padded leading dimensions.

Each buffer handed to a kernel is a tests/guard.py allocation [front guard | payload with row pitch ld > cols | back guard]: inputs are
poisoned (NaN / illegal bytes) around the payload, outputs and workspaces are filled with 0xA5 and must come back with guards and pitch
padding untouched, completely written where the header says so, equal to the plain call (contiguous exact-size tensors) and inside the
bound of the entry point's existing parity test (tests/test_kernels_gpu.py, test_msda_backward_gpu.py, test_corr_backward_gpu.py -- the
case tables and bounds are restated from there, no tolerance is new).  Workspaces are exactly what the uni_*_workspace_bytes function
returns.  Guard widths: guard.guard_bytes = max(64 KiB, 256 rows of the pitch) -- the tallest tile of the GEMM family is 256 rows; flat
buffers take the 64 KiB floor (the largest flat tile, a 32 x 128 fp32 correlation tile, is 16 KiB).

The comparison with the plain call is BITWISE except where listed here (every record of guard_report.json in the results directory says which):
  * gn_stats of uni_gemm_bf16 / uni_gemm_h2: fp64 atomics (or per-tile fp32 partial sums) arrive in another order -> the existing bound
    against the fp64 sums;
  * grad_value of uni_msda_bwd / uni_msda_bwd_f64: hardware float atomics, documented as run-to-run different in the last bits -> both
    calls are held to the reference bound;
  * fp32 outputs of GEMMs with N = 5 / 169 keep the same scalar epilogue in both calls and are still compared bitwise; nothing else differs.

Not covered: the context entry points (uni_backbone_fpn, uni_interaction, uni_upsample, uni_head*, uni_pos_embed) keep their buffers
inside the engine's workspace, out of reach of this method; the model-level tests (tests/test_model_gpu.py) hold them to the reference.
What the method cannot see at all (a stray read whose value is discarded, a stray write beyond the guard width) is stated in guard.py."""
import ctypes as C
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import guard as G  # noqa: E402
import unicorn_oracle as uo  # noqa: E402
import mask_oracle as mo  # noqa: E402
from planted import planted_pred  # noqa: E402

DEV = "cuda"
ACTS = {0: lambda x: x, 1: F.relu, 2: F.gelu, 3: F.silu, 4: torch.sigmoid}


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    t0 = time.time()
    yield _lib
    G.record("module", "wall time", "tests/test_kernel_bounds_gpu.py", {}, [], note="%.1f s" % (time.time() - t0))
    G.dump()


def P(x):
    """device pointer of a tensor / guarded buffer / None"""
    if x is None:
        return None
    return C.c_void_p(x.ptr if isinstance(x, G.Guarded) else x.data_ptr())


def gin(name, t, ld=None, poison=None):
    t2 = t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])
    pitch = t2.shape[1] if ld is None else ld
    return G.guard_in(name, t2, ld=ld, guard=G.guard_bytes(pitch, t.element_size()), poison=poison)


def gout(name, rows, cols, dtype, ld=None, init=None):
    es = torch.empty((), dtype=dtype).element_size()
    return G.guard_out(name, rows, cols, dtype, DEV, ld=ld, guard=G.guard_bytes(cols if ld is None else ld, es), init=init)


def gws(name, nbytes):
    return G.guard_ws(name, nbytes, DEV, guard=64 * 1024)


def sync_check(*bufs):
    torch.cuda.synchronize()
    G.check_all(*bufs)


def relmax(got, ref):
    return float((got.detach().double().cpu() - ref.double().cpu()).abs().max() / ref.double().abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# GEMM family
# ------------------------------------------------------------------------------------------------------------------------------
def pack_weight(L, w, h2):
    N, Cin, KH, KW = w.shape
    K = Cin * KH * KW
    Npad, Kpad = (N + 255) // 256 * 256, (K + 63) // 64 * 64
    wc = np.ascontiguousarray(w.float().cpu().numpy())
    if h2:
        out = np.zeros((Npad, Kpad), dtype=np.uint32)
        sc = C.c_float(0)
        L.check(L.lib().uni_pack_weight_h2(wc.ctypes.data_as(C.c_void_p), N, Cin, KH, KW, out.ctypes.data_as(C.c_void_p), C.byref(sc)), "pack_h2")
        return torch.from_numpy(out.view(np.int32)).cuda(), sc.value
    out = np.zeros((Npad, Kpad), dtype=np.uint16)
    L.check(L.lib().uni_pack_weight(wc.ctypes.data_as(C.c_void_p), N, Cin, KH, KW, out.ctypes.data_as(C.c_void_p)), "pack")
    return torch.from_numpy(out.view(np.int16)).cuda().view(torch.bfloat16), 1.0


def cast_h2(L, x):
    M, C_ = x.shape
    out = torch.zeros((M, C_), device=DEV, dtype=torch.int32)
    L.check(L.lib().uni_cast_h2(L.ptr(x), C_, L.ptr(out), C_, M, C_, L.stream_ptr()), "cast_h2")
    return out


def h2_decode(buf, M, C_):
    h = buf.contiguous().view(torch.float16).reshape(M, C_ // 8, 2, 8).float()
    return (h[:, :, 0] + h[:, :, 1]).reshape(M, C_)


def pad_ld(n, mult=8):
    """a leading dimension > n that keeps the launchers' divisibility (16-byte rows) when n has it; N = 5 / 169 rows stay unaligned"""
    return n + mult if n % mult == 0 else n + 1 if n % 2 else n + 2


def gemm_problem(L, fam, case, bound):
    """case = (Hin, Win, Cin, N, k, stride, pad, act, bias, res, G, outF, outB, splitk); res: False / True / "inplace" (aliases outF)"""
    Hin, Win, Cin, N, k, stride, pad, act, use_bias, use_res, Gn, use_F, use_B, sk = case
    g = torch.Generator().manual_seed((Hin * 7 + Win * 3 + Cin + N + k) & 0xffff)
    h2 = fam == "h2"
    x = torch.randn(1, Cin, Hin, Win, generator=g) * (2.0 if h2 and bound != "splitk" else 1.0)
    w = torch.randn(N, Cin, k, k, generator=g) * (0.05 if bound == "splitk" else 1.0 / (Cin * k * k) ** 0.5)
    bias = torch.randn(N, generator=g) * (1.0 if bound == "splitk" else 0.1) if use_bias else None
    if not h2:
        x, w = x.bfloat16().float(), w.bfloat16().float()          # bf16 kernels: fp64 reference on the same bf16-rounded operands
    xr = x[0].permute(1, 2, 0).reshape(Hin * Win, Cin).contiguous().cuda()
    A = cast_h2(L, xr) if h2 else xr.bfloat16()
    xd = x.double().cuda()
    if bound == "splitk":                                          # that test's reference: fp64 on the f16x2-DECODED operand
        xd = h2_decode(A, Hin * Win, Cin).double().reshape(Hin, Win, Cin).permute(2, 0, 1)[None]
    wd = w.double().cuda()
    ref = F.conv2d(xd, wd, bias.double().cuda() if use_bias else None, stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wd.abs(), None, stride=stride, padding=pad)
    M = ref.shape[2] * ref.shape[3]
    raw = ref[0].permute(1, 2, 0).reshape(M, N)
    mag = mag[0].permute(1, 2, 0).reshape(M, N)
    res = torch.randn(M, N, generator=g).cuda() if use_res else None
    exp = ACTS[act](raw) + (res.double() if use_res else 0)
    Wp, wscale = pack_weight(L, w, h2)
    return dict(A=A, Wp=Wp, wscale=wscale, bias=bias.cuda() if use_bias else None, res=res, raw=raw, mag=mag, exp=exp, M=M, K=Cin * k * k)


def gemm_call(L, fam, case, p, cfg, A, lda, Wp, bias, res, ldr, outF, ldf, outB, ldb, stats):
    Hin, Win, Cin, N, k, stride, pad, act, _, _, Gn, _, _, sk = case
    force = cfg + (1000000 * sk if sk > 1 else 0)
    cpg = (N // Gn) if Gn else 0
    if fam == "h2":
        rc = L.lib().uni_gemm_h2(P(A), lda, P(Wp), p["wscale"], p["M"], N, Hin, Win, Cin, k, k, stride, pad, P(bias), act, P(res), ldr,
                                 P(outF), ldf, P(outB), ldb, P(stats), cpg, force, L.stream_ptr())
    else:
        rc = L.lib().uni_gemm_bf16(P(A), lda, P(Wp), p["M"], N, Hin, Win, Cin, k, k, stride, pad, P(bias), act, P(res), ldr,
                                   P(outF), ldf, P(outB), ldb, P(stats), cpg, force, L.stream_ptr())
    L.check(rc, "gemm %s cfg %d" % (fam, cfg))


def gemm_bounds(fam, case, p, cfg, bound, outF, outB, stats, stats_atol):
    """the existing tests' bounds, against fp64 (see the docstrings of test_gemm_conv / test_gemm_h2 / test_gemm_h2_deep / test_gemm_h2_splitk)"""
    N, Gn, M = case[3], case[10], p["M"]
    exp, mag = p["exp"], p["mag"]
    scale = max(1.0, exp.abs().max().item())
    if fam == "bf16":
        if outF is not None:
            assert torch.isfinite(outF).all(), cfg
            assert (outF.double() - exp).abs().max().item() < 2e-3 * scale, cfg
        if outB is not None:
            assert (outB.double() - exp).abs().max().item() < 1e-2 * scale, cfg
        if Gn:
            grp = p["raw"].reshape(M, Gn, N // Gn)
            s_ref = torch.stack([grp.sum((0, 2)), (grp ** 2).sum((0, 2))], 1)
            assert torch.allclose(stats[:2 * Gn].reshape(Gn, 2), s_ref, rtol=1e-3, atol=stats_atol), cfg
        return
    if bound == "splitk":
        tol = (4e-6 if p["K"] <= 4096 else 1e-5) * scale
        assert (outF.double() - exp).abs().max().item() < tol, cfg
    else:
        tol = mag * 2.0 ** -20 + 1e-6
        if outF is not None:
            assert torch.isfinite(outF).all(), cfg
            assert ((outF.double() - exp).abs() <= tol * 1.2).all(), (cfg, ((outF.double() - exp).abs() / tol).max().item())
        if outB is not None:
            dec = h2_decode(outB, M, N).double()
            assert ((dec - exp).abs() <= tol * 1.2 + exp.abs() * 2.0 ** -21).all(), cfg
    if Gn:
        grp = p["raw"].reshape(M, Gn, N // Gn)
        s_ref = torch.stack([grp.sum((0, 2)), (grp ** 2).sum((0, 2))], 1)
        if bound == "splitk":                 # test_gemm_h2_splitk holds the statistics to the UNSPLIT launch at 1e-5 of their maximum
            s1 = p["stats_unsplit"][:2 * Gn]
            assert (stats[:2 * Gn] - s1).abs().max().item() < 1e-5 * s1.abs().max().item(), cfg
        else:
            assert torch.allclose(stats[:2 * Gn].reshape(Gn, 2), s_ref, rtol=2e-5, atol=stats_atol), cfg


def run_gemm(L, fam, case, cfgs, bound="mag", stats_atol=None, table=""):
    Hin, Win, Cin, N, k, stride, pad, act, use_bias, use_res, Gn, use_F, use_B, sk = case
    h2 = fam == "h2"
    p = gemm_problem(L, fam, case, bound)
    M = p["M"]
    if stats_atol is None:
        stats_atol = 2e-2 if h2 else 1e-2
    odt = torch.int32 if h2 else torch.bfloat16
    lda, ldf, ldb, ldr = Cin + 8, pad_ld(N, 8), pad_ld(N, 8), pad_ld(N, 4)
    inplace = use_res == "inplace"
    if inplace:
        ldr = ldf
    if bound == "splitk" and Gn:                 # the unsplit launch of the same problem: yardstick of the split statistics
        o1, s1 = torch.zeros((M, N), device=DEV), torch.zeros(64, device=DEV, dtype=torch.float64)
        gemm_call(L, fam, case[:13] + (1,), p, cfgs[0], p["A"], Cin, p["Wp"], p["bias"], None, N, o1, N, None, N, s1)
        torch.cuda.synchronize()
        p["stats_unsplit"] = s1
    for cfg in cfgs:
        # the plain call: contiguous exact-size tensors
        oF = (p["res"].clone() if inplace else torch.full((M, N), float("nan"), device=DEV)) if use_F else None
        oB = torch.zeros((M, N), device=DEV, dtype=odt) if use_B else None
        st = torch.zeros(64, device=DEV, dtype=torch.float64) if Gn else None
        gemm_call(L, fam, case, p, cfg, p["A"], Cin, p["Wp"], p["bias"], oF if inplace else p["res"], N, oF, N, oB, N, st)
        torch.cuda.synchronize()
        # the guarded call
        gA = gin("A", p["A"], ld=lda, poison="nan16" if h2 else None)
        gW = gin("w_packed", p["Wp"], poison="nan16" if h2 else None)
        gb = gin("bias", p["bias"]) if use_bias else None
        gF = gout("outF", M, N, torch.float32, ld=ldf, init=p["res"] if inplace else None) if use_F else None
        gr = None if (not use_res or inplace) else gin("residual", p["res"], ld=ldr)
        gB = gout("outB", M, N, odt, ld=ldb) if use_B else None
        gs = gout("gn_stats", 1, 64, torch.float64, init=torch.zeros(64, dtype=torch.float64)) if Gn else None
        gemm_call(L, fam, case, p, cfg, gA, lda, gW, gb, gF if inplace else gr, ldr, gF, ldf, gB, ldb, gs)
        torch.cuda.synchronize()
        for b in (gA, gW, gb, gr, gF, gB):
            if b is not None:
                b.check()
        if gs is not None:
            gs.check(complete=False)             # 2 G of the 64 doubles are accumulated into, the rest of the slot is not written
            assert (gs.view[0, 2 * Gn:] == 0).all(), cfg
        if gF is not None:
            gF.check_equal(oF, "the plain call (cfg %d)" % cfg)
        if gB is not None:
            gB.check_equal(oB, "the plain call (cfg %d)" % cfg)
        gemm_bounds(fam, case, p, cfg, bound, gF.payload() if gF else None,
                    (gB.payload() if h2 else gB.payload().float()) if gB else None, gs.view[0] if gs else None, stats_atol)
        G.record("uni_gemm_" + fam, "%sforce_cfg %d%s" % (table + " " if table else "", cfg, " split-K %d" % sk if sk > 1 else ""),
                 "M=%d N=%d K=%d conv %dx%d/s%d act %d" % (M, N, p["K"], k, k, stride, act),
                 {"lda": lda, "ldr": ldr if use_res else 0, "ldf": ldf if use_F else 0, "ldb": ldb if use_B else 0},
                 [gA, gW, gb, gr, gF, gB, gs], bitwise=not Gn,
                 note="outF / outB bitwise; gn_stats (fp64 atomics) is held to the existing bound against the fp64 sums, not to the plain call" if Gn else "")


# (Hin, Win, Cin, N, k, stride, pad, act, bias, res, G, outF, outB, splitk)
SMALL_CONV = [
    (20, 24, 96, 384, 1, 1, 0, 2, True, False, 0, True, True, 1),        # pwconv1 + GELU, K = 96 (K tail)
    (20, 24, 384, 96, 1, 1, 0, 0, True, True, 0, True, True, 1),         # pwconv2 + residual
    (25, 40, 256, 256, 3, 1, 1, 0, False, False, 16, True, True, 1),     # 3x3 + GN sums, M = 1000 (ragged)
    (26, 34, 192, 192, 3, 2, 1, 0, False, False, 16, True, True, 1),     # 3x3 stride 2, M = 221
    (20, 20, 96, 192, 2, 2, 0, 0, True, False, 0, True, True, 1),        # 2x2 / s2
    (10, 10, 48, 48, 3, 1, 1, 0, False, False, 16, True, True, 1),       # cpg = 3
    (13, 17, 256, 5, 1, 1, 0, 4, True, False, 0, True, True, 1),         # N = 5 (ldf 6 like the head buffer)
    (13, 17, 256, 169, 3, 1, 1, 0, True, False, 0, True, True, 1),       # N = 169
    (16, 16, 64, 256, 3, 1, 1, 1, True, False, 0, True, True, 1),        # ReLU
    (37, 29, 136, 264, 1, 1, 0, 3, True, False, 0, True, True, 1),       # K tail 136, N = 256 + 8, SiLU
]


@pytest.mark.parametrize("case", SMALL_CONV)
def test_gemm_bf16_tiles(L, case):
    """heuristic, 2-wave / 4-wave tiles and the persistent variants at one-tile problems (test_gemm_conv's cfg list)"""
    run_gemm(L, "bf16", case, [0, 22, 12, 21, 11, 122, 42, 24, 44, 444, 445, 224], table="tiles")


@pytest.mark.parametrize("case", SMALL_CONV)
def test_gemm_h2_tiles(L, case):
    """test_gemm_h2's cfg list; the operand-format output needs N % 8 == 0"""
    if case[3] % 8:
        case = case[:12] + (False,) + case[13:]
    run_gemm(L, "h2", case, [0, 44, 22, 12, 21, 11], table="tiles")


LARGE_PLAIN = [
    (35003, 1, 136, 512, 1, 1, 0, 0, True, True, 0, True, True, 1),      # K tail 136, residual + fp32 + operand out, ragged M past the persistent grid
    (9001, 1, 320, 384, 1, 1, 0, 2, True, False, 0, False, True, 1),     # K = 320, GELU, operand-format out only
    (5000, 1, 256, 136, 1, 1, 0, 3, True, False, 0, True, True, 1),      # N = 128 + 8, SiLU
]
PINGPONG_PLAIN = [                                                        # what cfg 188 covers: K a multiple of the step, none / ReLU / GELU
    (35003, 1, 192, 512, 1, 1, 0, 0, True, True, 0, True, True, 1),      # odd step count, residual + fp32 + operand out, ragged M
    (9001, 1, 320, 384, 1, 1, 0, 2, True, False, 0, False, True, 1),     # GELU, operand-format out only
    (5000, 1, 256, 136, 1, 1, 0, 1, True, False, 0, True, True, 1),      # N = 128 + 8, ReLU
]


@pytest.mark.parametrize("case", LARGE_PLAIN)
def test_gemm_bf16_persistent(L, case):
    """more tiles than persistent blocks: the row-descriptor walkers (test_gemm_large's cfg list)"""
    run_gemm(L, "bf16", case, [144, 44, 444, 445, 224, 0], table="persistent")


@pytest.mark.parametrize("case", LARGE_PLAIN)
def test_gemm_h2_persistent(L, case):
    run_gemm(L, "h2", case, [44, 0, 22], table="persistent")


@pytest.mark.parametrize("case", PINGPONG_PLAIN)
def test_gemm_pingpong_plain(L, case):
    """cfg 188 (gemm_h2q.hip) on plain GEMMs with several tiles per persistent block, both families"""
    run_gemm(L, "bf16", case, [188], table="ping-pong")
    run_gemm(L, "h2", case, [188], table="ping-pong")


PINGPONG_CONV = [
    (200, 320, 64, 512, 3, 1, 1, 0, False, False, 16, True, False, 1),     # 3x3 + GroupNorm sums
    (101, 163, 128, 384, 3, 2, 1, 0, True, False, 16, True, False, 1),     # 3x3 stride 2, odd map
    (120, 160, 64, 256, 2, 2, 0, 0, True, False, 0, True, False, 1),       # 2x2 / s2
    (160, 200, 128, 256, 1, 1, 0, 0, False, False, 16, True, False, 1),    # 1x1 + GroupNorm sums
    (96, 96, 64, 256, 3, 1, 1, 1, True, False, 0, False, True, 1),         # 3x3 + ReLU, operand-format output only
]


@pytest.mark.parametrize("case", PINGPONG_CONV)
def test_gemm_pingpong_conv(L, case):
    """cfg 188 as an implicit GEMM, both families (test_gemm_bf16_pingpong / test_gemm_h2q_conv_and_stats and their statistics bounds)"""
    run_gemm(L, "bf16", case, [188], stats_atol=1.0, table="ping-pong conv")
    run_gemm(L, "h2", case, [188], stats_atol=0.5, table="ping-pong conv")


DEEP = [
    (4000, 1, 3072, 768, 1, 1, 0, 0, True, "inplace", 0, True, False, 1),     # pwconv2 + in-place residual
    (1003, 1, 768, 3072, 1, 1, 0, 2, True, False, 0, False, True, 1),         # pwconv1 + GELU -> operand-format out, ragged M
    (50, 80, 384, 384, 3, 1, 1, 0, True, False, 16, True, False, 1),          # 3x3 + GroupNorm sums
    (26, 34, 192, 192, 3, 2, 1, 0, True, False, 16, True, False, 1),          # 3x3 stride 2, ragged M
    (20, 20, 96, 200, 2, 2, 0, 1, True, False, 0, False, True, 1),            # 2x2 / s2, N = 200
    (130, 1, 64, 96, 1, 1, 0, 0, True, False, 0, True, False, 1),             # K = 64
    (25, 40, 256, 256, 3, 1, 1, 0, True, False, 16, True, False, 4),          # split-K 4, statistics from the reduce kernel
    (1000, 1, 3072, 768, 1, 1, 0, 0, True, "inplace", 0, True, False, 5),     # split-K 5, unequal ranges, in-place residual
]


@pytest.mark.parametrize("case", DEEP)
def test_gemm_h2_deep(L, case):
    run_gemm(L, "h2", case, [322, 323, 332, 331, 346, 422, 423], stats_atol=5e-2, table="deep")


SPLITK = [
    # (case, cfg) of test_gemm_h2_splitk: bias, no activation, fp32 output
    ((25, 40, 256, 256, 3, 1, 1, 0, True, False, 16, True, False, 4), 0),
    ((50, 80, 384, 384, 3, 1, 1, 0, True, False, 16, True, False, 2), 22),
    ((1000, 1, 3072, 768, 1, 1, 0, 0, True, "inplace", 0, True, False, 3), 0),
    ((130, 1, 1536, 64, 1, 1, 0, 0, True, False, 0, True, False, 8), 0),
    ((4000, 1, 3072, 768, 1, 1, 0, 0, True, "inplace", 0, True, False, 4), 188),
    ((100, 160, 256, 256, 3, 1, 1, 0, True, False, 16, True, False, 4), 188),
    ((25, 40, 768, 768, 3, 1, 1, 0, True, False, 16, True, False, 6), 0),
    ((50, 80, 384, 384, 3, 1, 1, 0, True, False, 16, True, False, 3), 188),
]


@pytest.mark.parametrize("case,cfg", SPLITK)
def test_gemm_h2_splitk(L, case, cfg):
    """K ranges -> partial-tile slab -> reduce kernel.  The slab is not a caller buffer: uni_gemm_h2 keeps one grow-only allocation per
    device for it (at least split x M x N floats, larger after a larger earlier case), so it cannot be guarded or sized from here; every
    caller-visible buffer is."""
    run_gemm(L, "h2", case, [cfg], bound="splitk", stats_atol=0.0, table="split-K")


# ------------------------------------------------------------------------------------------------------------------------------
# casts, norms, the fused MLP
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C_", [(257, 64), (1, 96), (1003, 136)])
def test_casts(L, M, C_):
    """uni_cast_bf16 / uni_cast_h2 with ldx > C and ldo > C (ldx % 4, ldo % 8): bound of test_h2_cast_and_pack_formats / bf16 RNE"""
    g = torch.Generator().manual_seed(M + C_)
    x = (torch.randn(M, C_, generator=g) * 3).cuda()
    ldx, ldo = C_ + 4, C_ + 8
    for name, dt in (("uni_cast_bf16", torch.bfloat16), ("uni_cast_h2", torch.int32)):
        fn = getattr(L.lib(), name)
        plain = torch.zeros((M, C_), device=DEV, dtype=dt)
        L.check(fn(P(x), C_, P(plain), C_, M, C_, L.stream_ptr()), name)
        gx, go = gin("x", x, ld=ldx), gout("out", M, C_, dt, ld=ldo)
        L.check(fn(P(gx), ldx, P(go), ldo, M, C_, L.stream_ptr()), name)
        sync_check(gx, go)
        go.check_equal(plain)
        if dt == torch.bfloat16:
            assert torch.equal(go.payload(), x.bfloat16())
        else:
            dec = h2_decode(go.payload(), M, C_)
            assert ((dec - x).abs() <= x.abs() * 2.0 ** -21 + 2.0 ** -25).all()
        G.record(name, "-", "M=%d C=%d" % (M, C_), {"ldx": ldx, "ldo": ldo}, [gx, go])


@pytest.mark.parametrize("C_", [96, 192, 768, 1536])
def test_layernorm(L, C_):
    g = torch.Generator().manual_seed(C_)
    M, ldx = 777, C_ + 4
    x = torch.randn(M, C_, generator=g) * 3 + 1.5
    ga, be = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    exp = F.layer_norm(x.double(), (C_,), ga.double(), be.double(), 1e-6)
    xd, gd, bd = x.cuda(), ga.cuda(), be.cuda()
    pF, pB = torch.empty((M, C_), device=DEV), torch.empty((M, C_), device=DEV, dtype=torch.bfloat16)
    L.check(L.lib().uni_layernorm(P(xd), C_, P(gd), P(bd), 1e-6, M, C_, P(pF), P(pB), L.stream_ptr()), "ln")
    gx, gg, gb = gin("x", xd, ld=ldx), gin("gamma", gd), gin("beta", bd)
    oF, oB = gout("outF", M, C_, torch.float32), gout("outB", M, C_, torch.bfloat16)
    L.check(L.lib().uni_layernorm(P(gx), ldx, P(gg), P(gb), 1e-6, M, C_, P(oF), P(oB), L.stream_ptr()), "ln")
    sync_check(gx, gg, gb, oF, oB)
    oF.check_equal(pF)
    oB.check_equal(pB)
    assert (oF.payload().cpu().double() - exp).abs().max() < 2e-5 * exp.abs().max()
    assert (oB.payload().cpu().double() - exp).abs().max() < 8e-3 * exp.abs().max()
    G.record("uni_layernorm", "-", "M=%d C=%d" % (M, C_), {"ldx": ldx}, [gx, gg, gb, oF, oB])


def _dw_problem(C_, B, H, W):
    g = torch.Generator().manual_seed(C_ + H + B)
    x = torch.randn(B, C_, H, W, generator=g)
    w = torch.randn(C_, 1, 7, 7, generator=g) / 7
    b, ga, be = torch.randn(C_, generator=g) * 0.1, 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    y = F.conv2d(x, w, b, padding=3, groups=C_).permute(0, 2, 3, 1)               # the existing tests' reference: torch fp32 on the CPU
    exp = F.layer_norm(y, (C_,), ga, be, 1e-6).reshape(-1, C_).cuda().double()
    xn = x.permute(0, 2, 3, 1).contiguous().cuda().reshape(B * H * W, C_)
    return xn, w.reshape(C_, 49).t().contiguous().cuda(), b.cuda(), ga.cuda(), be.cuda(), exp


def _dw_decode(out, fmt, M, C_):
    return h2_decode(out, M, C_).double() if fmt == 2 else out.double()


DW_VARIANTS = [
    # (C, B, H, W, variant of the existing tables)
    (96, 3, 20, 24, "small map"),
    (192, 1, 101, 163, "8-px strips"),
    (768, 1, 49, 83, "one frame with 275 strips: past the row-split kernel's limit, 8-px strips"),
    (768, 1, 50, 80, "row-split one-frame kernel"),
    (768, 2, 31, 45, "row-split, two samples, odd H"),
    (768, 1, 127, 163, "persistent LDS-weight variant"),
    (256, 1, 207, 323, "persistent LDS-weight variant, LDS reduction"),
    (192, 3, 150, 323, "packed-lane strip groups, ragged last group"),
    (192, 2, 201, 320, "packed-lane strip groups, full rows"),
    (512, 5, 33, 70, "non-persistent 2-row kernel, batched, ragged W"),
]


@pytest.mark.parametrize("C_,B,H,W,variant", DW_VARIANTS)
def test_dwconv7_ln(L, C_, B, H, W, variant):
    """uni_dwconv7_ln_ex in all three formats (+ uni_dwconv7_ln for one map); x ends after its last pixel, the 7x7 halo must come from
    the zero padding and never from the NaN guards; bounds of test_dwconv7_ln / test_dwconv7_ln_batched_all_formats"""
    xn, wt, b, ga, be, exp = _dw_problem(C_, B, H, W)
    M = B * H * W
    scale = max(1.0, exp.abs().max().item())
    runs = [("uni_dwconv7_ln_ex", f) for f in (2, 1, 0)] + ([("uni_dwconv7_ln", 0)] if B == 1 else [])
    for name, fmt in runs:
        dt = torch.bfloat16 if fmt == 0 else (torch.int32 if fmt == 2 else torch.float32)

        def call(x_, w_, b_, g_, be_, o_):
            if name == "uni_dwconv7_ln":
                return L.lib().uni_dwconv7_ln(P(x_), P(w_), P(b_), P(g_), P(be_), 1e-6, H, W, C_, P(o_), L.stream_ptr())
            return L.lib().uni_dwconv7_ln_ex(P(x_), P(w_), P(b_), P(g_), P(be_), 1e-6, B, H, W, C_, P(o_), fmt, L.stream_ptr())
        plain = torch.zeros((M, C_), device=DEV, dtype=dt)
        L.check(call(xn, wt, b, ga, be, plain), name)
        # x_nhwc: the 7x7 halo reaches 3 image rows above and below the map, 4 for the 2-row / 4-row kernels, plus up to 8 pixels of a
        # strip: the guard is sized for (4 W + 8) pixels of C fp32 channels, so an unclamped halo row would land in NaN
        gx = G.guard_in("x_nhwc", xn, guard=max(G.guard_bytes(C_, 4), (4 * W + 8) * C_ * 4))
        gw_, gb, gg, gbe = gin("w49c", wt), gin("bias", b), gin("gamma", ga), gin("beta", be)
        go = gout("out", M, C_, dt)
        L.check(call(gx, gw_, gb, gg, gbe, go), name)
        sync_check(gx, gw_, gb, gg, gbe, go)
        go.check_equal(plain)
        err = (_dw_decode(go.payload(), fmt, M, C_) - exp).abs().max().item()
        tol = (8e-3 if name == "uni_dwconv7_ln" else 1.6e-2) if fmt == 0 else 2e-5
        assert err < tol * scale, (name, fmt, err)
        G.record(name, "%s, fmt %d" % (variant, fmt), "B=%d H=%d W=%d C=%d" % (B, H, W, C_), {}, [gx, gw_, gb, gg, gbe, go])


@pytest.mark.parametrize("C_,Gn,act", [(256, 16, 3), (192, 16, 3), (48, 16, 3), (256, 32, 0), (128, 16, 1)])
def test_groupnorm_act(L, C_, Gn, act):
    g = torch.Generator().manual_seed(C_ + Gn)
    M, eps = 1000, 1e-3
    x = torch.randn(M, C_, generator=g) * 2 + 0.5
    ga, be = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    exp = ACTS[act](F.group_norm(x.t().reshape(1, C_, M, 1).double(), Gn, ga.double(), be.double(), eps)).reshape(C_, M).t()
    grp = x.reshape(M, Gn, C_ // Gn).double()
    stats = torch.stack([grp.sum((0, 2)), (grp ** 2).sum((0, 2))], 1).reshape(-1).cuda()
    xd, gd, bd = x.cuda(), ga.cuda(), be.cuda()
    pF, pB = torch.empty((M, C_), device=DEV), torch.empty((M, C_), device=DEV, dtype=torch.bfloat16)
    L.check(L.lib().uni_groupnorm_act(P(xd), P(stats), P(gd), P(bd), eps, M, C_, Gn, act, P(pF), P(pB), L.stream_ptr()), "gn")
    gx, gs, gg, gb = gin("x", xd), gin("stats", stats), gin("gamma", gd), gin("beta", bd)
    oF, oB = gout("outF", M, C_, torch.float32), gout("outB", M, C_, torch.bfloat16)
    L.check(L.lib().uni_groupnorm_act(P(gx), P(gs), P(gg), P(gb), eps, M, C_, Gn, act, P(oF), P(oB), L.stream_ptr()), "gn")
    sync_check(gx, gs, gg, gb, oF, oB)
    oF.check_equal(pF)
    oB.check_equal(pB)
    scale = max(1.0, exp.abs().max().item())
    assert (oF.payload().cpu().double() - exp).abs().max() < 1e-4 * scale
    # bf16 output (no existing test, no tolerance): the kernel stores the SAME fp32 value to both outputs, the bf16 one rounded to nearest even
    assert torch.equal(oB.payload(), oF.payload().bfloat16())
    G.record("uni_groupnorm_act", "act %d, fp32 + bf16 outputs" % act, "M=%d C=%d G=%d" % (M, C_, Gn), {}, [gx, gs, gg, gb, oF, oB])


def _op_dtype(fmt):
    return torch.bfloat16 if fmt == 0 else (torch.int32 if fmt == 2 else torch.float32)


def _op_decode(buf, fmt):
    return h2_decode(buf, buf.shape[0], buf.shape[1]).double() if fmt == 2 else buf.double()


@pytest.mark.parametrize("mode,C_,fmt", [("ps", 192, 2), ("ps", 768, 0), ("pair", 256, 2), ("pair", 256, 1)])
def test_layernorm_ex(L, mode, C_, fmt):
    """uni_layernorm_ex: the PixelShuffle scatter of the operand rows (three stacked (7, 5) maps -> a dense (42, 10, C / 4) map) and the
    frame-pair remap of the fp32 rows (tokens [3][2][35]: even frames -> out_f32, odd frames -> out_f32_2, operand rows unremapped), padded
    pitches on every strided buffer; bounds of test_layernorm (fp32 2e-5, bf16 8e-3) and format 2 of test_dwconv7_ln_batched_all_formats"""
    B, h, w, hw = 3, 7, 5, 35
    M = B * h * w if mode == "ps" else B * 2 * hw
    g = torch.Generator().manual_seed(C_ + fmt)
    ldx, ldf, ldb = C_ + 4, C_ + 4, C_ + 8
    x = torch.randn(M, C_, generator=g) * 3 + 1.5
    ga, be = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    exp = F.layer_norm(x.double(), (C_,), ga.double(), be.double(), 1e-6)
    big = exp.abs().max().item()
    xd, gd, bd = x.cuda(), ga.cuda(), be.cuda()
    dt = _op_dtype(fmt)
    rows_f = B * hw
    rows_b, cols_b = (4 * M, C_ // 4) if mode == "ps" else (M, C_)

    def call(x_, ldx_, g_, b_, oF, ldf_, oF2, oB, ldb_):
        return L.lib().uni_layernorm_ex(P(x_), ldx_, P(g_), P(b_), 1e-6, M, C_, P(oF), ldf_, P(oF2), hw if mode == "pair" else 0, P(oB), ldb_,
                                        h if mode == "ps" else 0, w if mode == "ps" else 0, fmt, L.stream_ptr())
    pF = torch.zeros((rows_f, C_), device=DEV) if mode == "pair" else None
    pF2 = torch.zeros((rows_f, C_), device=DEV) if mode == "pair" else None
    pB = torch.zeros((rows_b, cols_b), device=DEV, dtype=dt)
    L.check(call(xd, C_, gd, bd, pF, C_, pF2, pB, C_), "layernorm_ex")
    gx, gg, gb = gin("x", xd, ld=ldx), gin("gamma", gd), gin("beta", bd)
    oF = gout("out_f32", rows_f, C_, torch.float32, ld=ldf) if mode == "pair" else None
    oF2 = gout("out_f32_2", rows_f, C_, torch.float32, ld=ldf) if mode == "pair" else None
    oB = gout("out_op", rows_b, cols_b, dt) if mode == "ps" else gout("out_op", rows_b, cols_b, dt, ld=ldb)      # the shuffled map is dense
    L.check(call(gx, ldx, gg, gb, oF, ldf, oF2, oB, ldb), "layernorm_ex")
    sync_check(gx, gg, gb, oF, oF2, oB)
    oB.check_equal(pB)
    if mode == "pair":
        oF.check_equal(pF)
        oF2.check_equal(pF2)
        e = exp.reshape(B, 2, hw, C_)
        assert (oF.payload().cpu().double() - e[:, 0].reshape(rows_f, C_)).abs().max() < 2e-5 * big
        assert (oF2.payload().cpu().double() - e[:, 1].reshape(rows_f, C_)).abs().max() < 2e-5 * big
        eb = exp
    else:
        eb = F.pixel_shuffle(exp.reshape(1, B * h, w, C_).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).reshape(rows_b, cols_b)
    tol = 8e-3 * big if fmt == 0 else 2e-5 * max(1.0, big)
    assert (_op_decode(oB.payload(), fmt).cpu() - eb).abs().max() < tol
    G.record("uni_layernorm_ex", "%s, fmt %d" % (mode, fmt), "M=%d C=%d" % (M, C_), {"ldx": ldx, "ldf": ldf, "ldb": ldb}, [gx, gg, gb, oF, oF2, oB])


@pytest.mark.parametrize("fmt", [2, 0])
def test_groupnorm_act_ex_upsampled_copy(L, fmt):
    """uni_groupnorm_act_ex: three samples with their own statistics slots, the prior fusion, fp32 + operand rows + the 2x nearest copy of
    every (47, 13) map into a (94, 26) map whose pitch is wider than C; bounds of test_groupnorm_act (fp32 1e-4), test_layernorm (bf16 8e-3)
    and format 2 of test_dwconv7_ln_batched_all_formats"""
    C_, Gn, act, B, W, H = 96, 16, 3, 3, 13, 47
    M, eps = H * W, 1e-3
    g = torch.Generator().manual_seed(C_ + fmt)
    x = torch.randn(B, M, C_, generator=g) * (1.0 + torch.arange(B).float().reshape(B, 1, 1)) + 0.5
    ga, be = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    prior, pbeta = torch.rand(B * M, generator=g), torch.randn(C_, generator=g)
    xs = x.double()
    grp = xs.reshape(B, M, Gn, C_ // Gn)
    stats = torch.zeros(B, 64, dtype=torch.float64)
    stats[:, 0:2 * Gn:2], stats[:, 1:2 * Gn:2] = grp.sum((1, 3)), (grp ** 2).sum((1, 3))
    exp = ACTS[act](F.group_norm(xs.permute(0, 2, 1).unsqueeze(-1), Gn, ga.double(), be.double(), eps)).squeeze(-1).permute(0, 2, 1)
    exp = (exp + prior.double().reshape(B, M, 1) * pbeta.double()).reshape(B * M, C_)
    eup = exp.reshape(B, H, W, C_).repeat_interleave(2, 1).repeat_interleave(2, 2).reshape(4 * B * M, C_)
    scale = max(1.0, exp.abs().max().item())
    xd, sd, gd, bd, pd, pbd = x.reshape(B * M, C_).cuda(), stats.cuda(), ga.cuda(), be.cuda(), prior.cuda(), pbeta.cuda()
    dt = _op_dtype(fmt)
    ldx, ldf, ldb, ldu = C_ + 4, C_ + 4, C_ + 8, C_ + 32

    def call(x_, ldx_, s_, g_, b_, p_, pb_, oF, ldf_, oB, ldb_, oU, ldu_):
        return L.lib().uni_groupnorm_act_ex(P(x_), ldx_, P(s_), P(g_), P(b_), eps, B, M, C_, Gn, act, P(p_), P(pb_), P(oF), ldf_, P(oB), ldb_, P(oU), ldu_,
                                            W, fmt, L.stream_ptr())
    pF = torch.zeros((B * M, C_), device=DEV)
    pB, pU = torch.zeros((B * M, C_), device=DEV, dtype=dt), torch.zeros((4 * B * M, C_), device=DEV, dtype=dt)
    L.check(call(xd, C_, sd, gd, bd, pd, pbd, pF, C_, pB, C_, pU, C_), "groupnorm_act_ex")
    gx, gs, gg, gb, gp, gpb = gin("x", xd, ld=ldx), gin("stats", sd), gin("gamma", gd), gin("beta", bd), gin("prior", pd), gin("prior_beta", pbd)
    oF, oB, oU = gout("out_f32", B * M, C_, torch.float32, ld=ldf), gout("out_op", B * M, C_, dt, ld=ldb), gout("out_up", 4 * B * M, C_, dt, ld=ldu)
    L.check(call(gx, ldx, gs, gg, gb, gp, gpb, oF, ldf, oB, ldb, oU, ldu), "groupnorm_act_ex")
    sync_check(gx, gs, gg, gb, gp, gpb, oF, oB, oU)
    oF.check_equal(pF)
    oB.check_equal(pB)
    oU.check_equal(pU)
    tol = (8e-3 if fmt == 0 else 2e-5) * scale
    assert (oF.payload().cpu().double() - exp).abs().max() < 1e-4 * scale
    assert (_op_decode(oB.payload(), fmt).cpu() - exp).abs().max() < tol
    assert (_op_decode(oU.payload(), fmt).cpu() - eup).abs().max() < tol
    G.record("uni_groupnorm_act_ex", "prior + outUp, fmt %d" % fmt, "B=%d M=%d C=%d G=%d W=%d" % (B, M, C_, Gn, W),
             {"ldx": ldx, "ldf": ldf, "ldb": ldb, "ldu": ldu}, [gx, gs, gg, gb, gp, gpb, oF, oB, oU])


@pytest.mark.parametrize("W", [96, 100])          # W % 16 == 0: 4-pixel kernel, otherwise the 1-pixel fallback
@pytest.mark.parametrize("C_", [96, 192])
def test_stem(L, C_, W):
    g = torch.Generator().manual_seed(C_)
    H = 64
    img = torch.rand(1, 3, H, W, generator=g) * 255
    w = torch.randn(C_, 3, 4, 4, generator=g) / 48 ** 0.5
    b, ga, be = torch.randn(C_, generator=g) * 0.1, 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    exp = uo.ln_channels_first(F.conv2d(img, w, b, stride=4), ga, be).permute(0, 2, 3, 1).reshape(-1, C_)
    wt = w.reshape(C_, 48).t().contiguous().cuda()
    M = H // 4 * W // 4
    imd, bd, gd, bed = img.cuda(), b.cuda(), ga.cuda(), be.cuda()
    plain = torch.empty((M, C_), device=DEV)
    L.check(L.lib().uni_stem(P(imd), H, W, P(wt), P(bd), P(gd), P(bed), C_, P(plain), L.stream_ptr()), "stem")
    gi, gw_, gb, gg, gbe = gin("img", imd.reshape(3 * H, W)), gin("w48c", wt), gin("bias", bd), gin("gamma", gd), gin("beta", bed)
    go = gout("out_nhwc", M, C_, torch.float32)
    L.check(L.lib().uni_stem(P(gi), H, W, P(gw_), P(gb), P(gg), P(gbe), C_, P(go), L.stream_ptr()), "stem")
    sync_check(gi, gw_, gb, gg, gbe, go)
    go.check_equal(plain)
    assert (go.payload().cpu() - exp).abs().max() < 2e-4 * max(1.0, exp.abs().max().item())
    G.record("uni_stem", "W %% 16 %s 0" % ("==" if W % 16 == 0 else "!="), "H=%d W=%d C=%d" % (H, W, C_), {}, [gi, gw_, gb, gg, gbe, go])


def mlp_pack(L, w1, w2, gamma, layout):
    C_ = w1.shape[1]
    nb = L.lib().uni_mlp_blob_bytes(C_)
    blob = np.zeros(nb // 2, dtype=np.uint16)
    a, b = C.c_float(0), C.c_float(0)
    w1c, w2c, gc = (np.ascontiguousarray(t.float().numpy()) for t in (w1, w2, gamma))
    L.check(L.lib().uni_mlp_pack(w1c.ctypes.data_as(C.c_void_p), w2c.ctypes.data_as(C.c_void_p), gc.ctypes.data_as(C.c_void_p), C_, layout,
                                 blob.ctypes.data_as(C.c_void_p), C.byref(a), C.byref(b)), "mlp_pack")
    return torch.from_numpy(blob.view(np.int16)).cuda(), a.value, b.value


@pytest.mark.parametrize("with_outb", [False, True])
@pytest.mark.parametrize("C_,M,layout,alias", [(192, 1, 0, True), (96, 1000, 0, True), (256, 4000, 0, False), (192, 33000, 0, True),
                                               (192, 1, 1, True), (256, 4000, 1, True), (192, 128, 1, False), (192, 33000, 1, True)])
def test_mlp_fused(L, C_, M, layout, alias, with_outb):
    """both layouts; lda / ldr / ldo / ldb padded; M = 1, a ragged M past one 128-row tile, a ragged M past the persistent grid
    (> 128 x 256 rows); with and without the f16x2 copy; out aliasing residual (what the engine does) and separate buffers.
    Bound of test_mlp_fused (fp64 on the f16x2-decoded operand)."""
    g = torch.Generator().manual_seed(C_ + M)
    x = torch.randn(M, C_, generator=g) * 1.5
    w1, b1 = torch.randn(4 * C_, C_, generator=g) * 0.05, torch.randn(4 * C_, generator=g) * 0.2
    w2, b2 = torch.randn(C_, 4 * C_, generator=g) * 0.05, torch.randn(C_, generator=g) * 0.2
    gamma = torch.rand(C_, generator=g) + 0.5
    res = (torch.randn(M, C_, generator=g) * 3.0).cuda()
    A = cast_h2(L, x.cuda())
    a_dec = h2_decode(A, M, C_).double()
    hid = F.gelu(a_dec @ w1.double().cuda().t() + b1.double().cuda())
    ref = res.double() + gamma.double().cuda() * (hid @ w2.double().cuda().t() + b2.double().cuda())
    blob, ws1, ws2 = mlp_pack(L, w1, w2, gamma, layout)
    b1d, b2d = b1.cuda(), (gamma * b2).cuda()
    lda, ldr, ldo, ldb = C_ + 8, C_ + 4, C_ + 12, C_ + 16
    if alias:
        ldr = ldo
    pout = res.clone()
    poutb = torch.zeros((M, C_), device=DEV, dtype=torch.int32) if with_outb else None
    L.check(L.lib().uni_mlp_fused(P(A), C_, P(blob), P(b1d), P(b2d), ws1, ws2, P(pout), C_, P(pout), C_, P(poutb), C_, M, C_, layout,
                                  L.stream_ptr()), "mlp_fused")
    gA, gbl, gb1, gb2 = gin("a_h2", A, ld=lda, poison="nan16"), gin("blob", blob.view(torch.float16), poison="nan16"), gin("b1", b1d), gin("b2", b2d)
    go = gout("out", M, C_, torch.float32, ld=ldo, init=res if alias else None)
    gr = None if alias else gin("residual", res, ld=ldr)
    gob = gout("out_h2", M, C_, torch.int32, ld=ldb) if with_outb else None
    L.check(L.lib().uni_mlp_fused(P(gA), lda, P(gbl), P(gb1), P(gb2), ws1, ws2, P(go if alias else gr), ldr, P(go), ldo, P(gob), ldb, M, C_,
                                  layout, L.stream_ptr()), "mlp_fused")
    sync_check(gA, gbl, gb1, gb2, go, gr, gob)
    go.check_equal(pout)
    got = go.payload().double()
    scale = max(1.0, ref.abs().max().item())
    assert torch.isfinite(got).all() and (got - ref).abs().max() < 4e-6 * scale
    if with_outb:
        gob.check_equal(poutb)
        assert (h2_decode(gob.payload(), M, C_).double() - got).abs().max() < 1e-6 * scale
    G.record("uni_mlp_fused", "layout %d, %s, %s f16x2 copy" % (layout, "out aliases residual" if alias else "separate residual", "with" if with_outb else "no"),
             "M=%d C=%d" % (M, C_), {"lda": lda, "ldr": ldr, "ldo": ldo, "ldb": ldb if with_outb else 0}, [gA, gbl, gb1, gb2, go, gr, gob])


# ------------------------------------------------------------------------------------------------------------------------------
# deformable attention
# ------------------------------------------------------------------------------------------------------------------------------
MSDA_SHAPES = [(7, 5), (3, 4)]


def msda_problem(D, dtype, exact_borders):
    """Sampling points in pixel coordinates: integer part from -2 .. W+1 (H+1) in BOTH levels -- outside the map, straddling every border
    (one or two corners outside) and inside -- fraction in [0.05, 0.95], so no coordinate sits within 0.05 of the lattice where
    grad_sampling_loc is discontinuous (the lattice rule of test_msda_backward_gpu.py).  exact_borders (forward only, continuous there):
    the first queries sit exactly ON -1, 0, W-1 and W."""
    N, M, Lq, Pn = 2, 3, 50, 4
    Ln, S = len(MSDA_SHAPES), sum(h * w for h, w in MSDA_SHAPES)
    g = torch.Generator().manual_seed(D)
    value = torch.randn(N, S, M, D, generator=g, dtype=torch.float64)
    loc = torch.empty(N, Lq, M, Ln, Pn, 2, dtype=torch.float64)
    for l, (h, w) in enumerate(MSDA_SHAPES):
        for c, n in ((0, w), (1, h)):
            px = torch.randint(-2, n + 2, (N, Lq, M, Pn), generator=g).double() + 0.05 + 0.9 * torch.rand(N, Lq, M, Pn, generator=g, dtype=torch.float64)
            if exact_borders:
                for q, v in enumerate((-1.0, 0.0, n - 1.0, float(n), -0.5, n - 0.5)):
                    px[:, q] = v
            loc[:, :, :, l, :, c] = (px + 0.5) / n
    attn = torch.softmax(torch.randn(N, Lq, M, Ln * Pn, generator=g, dtype=torch.float64), -1).view(N, Lq, M, Ln, Pn)
    gout_ = torch.randn(N, Lq, M * D, generator=g, dtype=torch.float64)
    return tuple(t.to(dtype) for t in (value, loc, attn, gout_)), (N, S, M, D, Lq, Ln, Pn)


def msda_host_shapes():
    flat = [v for hw in MSDA_SHAPES for v in hw]
    starts = [0]
    for h, w in MSDA_SHAPES[:-1]:
        starts.append(starts[-1] + h * w)
    return (C.c_int64 * len(flat))(*flat), (C.c_int64 * len(starts))(*starts)


def oracle_grads(dtype, value, loc, attn, gout_):
    v, l, a = (t.to(dtype).clone().requires_grad_(True) for t in (value, loc, attn))
    out = uo.msda_core(v, MSDA_SHAPES, l, a)
    out.backward(gout_.to(dtype))
    return out.detach(), v.grad, l.grad, a.grad


@pytest.mark.parametrize("D", [30, 32, 64, 71])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_msda_forward(L, D, dtype):
    (value, loc, attn, _), (N, S, M, _, Lq, Ln, Pn) = msda_problem(D, dtype, True)
    shp, lsi = msda_host_shapes()
    fn = L.lib().uni_msda_fwd if dtype == torch.float32 else L.lib().uni_msda_fwd_f64
    ref = uo.msda_core(value.double(), MSDA_SHAPES, loc.double(), attn.double())
    vd, ld_, ad = value.cuda(), loc.cuda(), attn.cuda()
    plain = torch.empty((N * Lq, M * D), device=DEV, dtype=dtype)
    L.check(fn(P(vd), shp, lsi, P(ld_), P(ad), P(plain), N, S, M, D, Lq, Ln, Pn, L.stream_ptr()), "msda_fwd")
    gv, gl, ga = gin("value", vd.reshape(N * S, M * D)), gin("sampling_loc", ld_.reshape(N * Lq, -1)), gin("attn_weight", ad.reshape(N * Lq, -1))
    go = gout("out", N * Lq, M * D, dtype)
    L.check(fn(P(gv), shp, lsi, P(gl), P(ga), P(go), N, S, M, D, Lq, Ln, Pn, L.stream_ptr()), "msda_fwd")
    sync_check(gv, gl, ga, go)
    go.check_equal(plain)
    got = go.payload().cpu().reshape(N, Lq, M * D)
    if dtype == torch.float64:
        assert relmax(got, ref) <= 1e-12
    else:
        assert torch.allclose(got.double(), ref, rtol=1e-4, atol=1e-5), (got.double() - ref).abs().max()
    G.record("uni_msda_fwd" + ("_f64" if dtype == torch.float64 else ""), "D=%d" % D, "N=%d Lq=%d M=%d levels %s P=%d" % (N, Lq, M, MSDA_SHAPES, Pn),
             {}, [gv, gl, ga, go])


@pytest.mark.parametrize("D", [30, 32, 64, 71])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_msda_backward(L, D, dtype):
    """the three gradients guarded; grad_value is summed with float atomics (not bitwise against the plain call: both calls are held to the
    reference bound), grad_sampling_loc / grad_attn_weight have one writer per element and are bitwise.  Bounds of
    test_msda_backward_gpu.py: fp64 1e-12 x max, fp32 4 x msda_core's own fp32-vs-fp64 error."""
    (value, loc, attn, gout_), (N, S, M, _, Lq, Ln, Pn) = msda_problem(D, dtype, False)
    shp, lsi = msda_host_shapes()
    fn = L.lib().uni_msda_bwd if dtype == torch.float32 else L.lib().uni_msda_bwd_f64
    want64 = oracle_grads(torch.float64, value, loc, attn, gout_)[1:]
    want32 = oracle_grads(torch.float32, value, loc, attn, gout_)[1:]
    vd, ld_, ad, gd = value.cuda(), loc.cuda(), attn.cuda(), gout_.cuda()
    pv, pl, pa = torch.empty_like(vd), torch.empty_like(ld_), torch.empty_like(ad)
    L.check(fn(P(vd), shp, lsi, P(ld_), P(ad), P(gd), P(pv), P(pl), P(pa), N, S, M, D, Lq, Ln, Pn, L.stream_ptr()), "msda_bwd")
    gv, gl, ga = gin("value", vd.reshape(N * S, M * D)), gin("sampling_loc", ld_.reshape(N * Lq, -1)), gin("attn_weight", ad.reshape(N * Lq, -1))
    gg = gin("grad_output", gd.reshape(N * Lq, M * D))
    ov, ol, oa = gout("grad_value", N * S, M * D, dtype), gout("grad_sampling_loc", N * Lq, M * Ln * Pn * 2, dtype), gout("grad_attn_weight", N * Lq, M * Ln * Pn, dtype)
    L.check(fn(P(gv), shp, lsi, P(gl), P(ga), P(gg), P(ov), P(ol), P(oa), N, S, M, D, Lq, Ln, Pn, L.stream_ptr()), "msda_bwd")
    sync_check(gv, gl, ga, gg, ov, ol, oa)
    ol.check_equal(pl)
    oa.check_equal(pa)
    for name, got, plain, w64, w32 in zip(("grad_value", "grad_loc", "grad_attn"), (ov, ol, oa), (pv, pl, pa), want64, want32):
        bound = 1e-12 if dtype == torch.float64 else 4 * relmax(w32, w64)
        e, ep = relmax(got.payload().reshape(w64.shape), w64), relmax(plain.reshape(w64.shape), w64)
        print("msda bwd D=%d %s %s: guarded err %.3e plain err %.3e bound %.3e" % (D, dtype, name, e, ep, bound))
        assert e <= bound and ep <= bound, (name, e, ep, bound)
    G.record("uni_msda_bwd" + ("_f64" if dtype == torch.float64 else ""), "D=%d" % D, "N=%d Lq=%d M=%d levels %s P=%d" % (N, Lq, M, MSDA_SHAPES, Pn),
             {}, [gv, gl, ga, gg, ov, ol, oa], bitwise=False, note="grad_value: float atomics, both calls within the reference bound; the other two bitwise")


@pytest.mark.parametrize("B,h,w", [(2, 10, 13), (1, 7, 5), (1, 50, 80)])
def test_msda_tokens(L, B, h, w):
    """uni_msda_tokens with ldo = 200 > 192 (the engine's 192-wide offset / logit rows inside a wider buffer); test_msda_wave_kernel_tokens"""
    g = torch.Generator().manual_seed(B * 100 + h)
    hw, ldo = h * w, 200
    Lq = 2 * hw
    value = torch.randn(B, Lq, 256, generator=g)
    off = torch.randn(B, Lq, 8, 2, 4, 2, generator=g) * 6.0
    off[:, :5] *= 30.0
    logits = torch.randn(B, Lq, 8, 8, generator=g) * 2.0
    offaw = torch.cat([off.reshape(B * Lq, 128), logits.reshape(B * Lq, 64)], 1).contiguous().cuda()
    vd = value.cuda()
    plain = torch.empty(B * Lq, 256, device=DEV)
    L.check(L.lib().uni_msda_tokens(P(vd), P(offaw), 192, B, h, w, P(plain), L.stream_ptr()), "uni_msda_tokens")
    gv, go_ = gin("value", vd.reshape(B * Lq, 256)), gin("offaw", offaw, ld=ldo)
    out = gout("out", B * Lq, 256, torch.float32)
    L.check(L.lib().uni_msda_tokens(P(gv), P(go_), ldo, B, h, w, P(out), L.stream_ptr()), "uni_msda_tokens")
    sync_check(gv, go_, out)
    out.check_equal(plain)
    ii, jj = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    ref = torch.stack([(jj.reshape(-1) + 0.5) / w, (ii.reshape(-1) + 0.5) / h], -1).repeat(2, 1)
    loc = ref[None, :, None, None, None, :] + off / torch.tensor([w, h], dtype=torch.float32)
    attn = torch.softmax(logits, -1).view(B, Lq, 8, 2, 4)
    want = uo.msda_core(value.view(B, Lq, 8, 32), [(h, w), (h, w)], loc, attn).reshape(B * Lq, 256)
    assert torch.allclose(out.payload().cpu(), want, rtol=1e-4, atol=2e-5)
    G.record("uni_msda_tokens", "-", "B=%d h=%d w=%d" % (B, h, w), {"ldo": ldo}, [gv, go_, out])


# ------------------------------------------------------------------------------------------------------------------------------
# correlation
# ------------------------------------------------------------------------------------------------------------------------------
def corr_single(L, er, ec, v, out, ws, ws_bytes, R, Q, K, prec):
    L.check(L.lib().uni_corr_softmax_pv(P(er), P(ec), P(v), P(out), R, Q, 128, K, prec, P(ws), ws_bytes, L.stream_ptr()), "uni_corr_softmax_pv")


@pytest.mark.parametrize("R,Q,K", [(1, 33, 1), (7, 1, 3), (33, 7, 4), (333, 257, 5), (1000, 1300, 8), (333, 257, 9), (700, 900, 16), (257, 333, 17),
                                   (700, 900, 21), (1600, 1600, 1), (4000, 2000, 5)])
def test_corr_softmax_pv(L, R, Q, K):
    """precisions 0..3; K on both sides of every dispatch boundary (1 | 4 | 8 | 16 rows per pass, chunks of 8 / 16); R, Q that are no
    multiples of the 32 x 128 tiles down to 1; (4000, 2000): the reference axis is split and the merge kernel runs.  The workspace is
    exactly uni_corr_workspace_bytes.  Bounds of test_corr_softmax_pv (2e-5) and test_corr_fp16_single_pass_mode (precision 3)."""
    g = torch.Generator().manual_seed(R + Q)
    er, ec, v = torch.randn(128, R, generator=g) * 0.6, torch.randn(128, Q, generator=g) * 0.6, torch.rand(K, R, generator=g)
    ref = uo.correlation_propagate(er, ec, v)
    ref16 = uo.correlation_propagate(er, ec, v, half=True)
    erd, ecd, vd = er.t().contiguous().cuda(), ec.t().contiguous().cuda(), v.cuda()
    need = L.lib().uni_corr_workspace_bytes(R, Q, K)
    for prec in (0, 1, 2, 3):
        plain, pws = torch.empty((K, Q), device=DEV), torch.empty(need, device=DEV, dtype=torch.uint8)
        corr_single(L, erd, ecd, vd, plain, pws, need, R, Q, K, prec)
        ge, gc, gv = gin("e_ref", erd), gin("e_cur", ecd), gin("values", vd)
        go, gw_ = gout("out", K, Q, torch.float32), gws("workspace", need)
        corr_single(L, ge, gc, gv, go, gw_, need, R, Q, K, prec)
        sync_check(ge, gc, gv, go, gw_)
        go.check_equal(plain)
        got = go.payload().cpu()
        if prec == 3:
            e16 = (got - ref16).abs()
            assert e16.max() < 1e-3 and e16.mean() < 1.5e-4, (e16.max(), e16.mean())
        else:
            assert (got - ref).abs().max().item() < 2e-5, prec
        G.record("uni_corr_softmax_pv", "precision %d, K=%d" % (prec, K), "R=%d Q=%d" % (R, Q), {}, [ge, gc, gv, go, gw_], workspace_bytes=need)


@pytest.mark.parametrize("case", [
    # (B, R, Q, K, values per frame, precision): test_corr_softmax_pv_batched's table, plus small ragged problems
    (3, 1600, 1600, 1, False, 2),
    (4, 1000, 1300, 3, True, 2),
    (2, 4000, 3000, 1, False, 2),        # few blocks per frame: the reference axis is split (partial results + batched merge)
    (5, 700, 900, 16, True, 3),
    (2, 333, 257, 21, False, 2),         # more than 16 value rows: frame by frame
    (3, 333, 257, 2, True, 0),           # exact-fp32 kernel: frame by frame
    (3, 33, 7, 4, True, 2),
    (2, 1, 33, 1, False, 3),
])
def test_corr_softmax_pv_batched(L, case):
    B, R, Q, K, vpf, prec = case
    g = torch.Generator().manual_seed(B + R + Q)
    er, ec = torch.randn(B, 128, R, generator=g) * 0.6, torch.randn(B, 128, Q, generator=g) * 0.6
    v = torch.rand((B, K, R) if vpf else (K, R), generator=g)
    erd, ecd, vd = er.transpose(1, 2).contiguous().cuda(), ec.transpose(1, 2).contiguous().cuda(), v.cuda()
    need = L.lib().uni_corr_workspace_bytes_batched(B, R, Q, K)
    fn = L.lib().uni_corr_softmax_pv_batched
    plain, pws = torch.empty((B, K, Q), device=DEV), torch.empty(need, device=DEV, dtype=torch.uint8)
    L.check(fn(P(erd), P(ecd), P(vd), P(plain), B, R, Q, 128, K, int(vpf), prec, P(pws), need, L.stream_ptr()), "corr_batched")
    ge, gc, gv = gin("e_ref", erd.reshape(B * R, 128)), gin("e_cur", ecd.reshape(B * Q, 128)), gin("values", vd.reshape(-1, R))
    go, gw_ = gout("out", B * K, Q, torch.float32), gws("workspace", need)
    L.check(fn(P(ge), P(gc), P(gv), P(go), B, R, Q, 128, K, int(vpf), prec, P(gw_), need, L.stream_ptr()), "corr_batched")
    sync_check(ge, gc, gv, go, gw_)
    go.check_equal(plain)
    got = go.payload().reshape(B, K, Q)
    need1 = L.lib().uni_corr_workspace_bytes(R, Q, K)
    for b in range(B):
        vb = vd[b] if vpf else vd
        one, ws1 = torch.empty((K, Q), device=DEV), torch.empty(need1, device=DEV, dtype=torch.uint8)
        corr_single(L, erd[b], ecd[b], vb, one, ws1, need1, R, Q, K, prec)
        torch.cuda.synchronize()
        assert (got[b] - one).abs().max().item() < 5e-6
        if prec != 3:
            ref = uo.correlation_propagate(er[b], ec[b], v[b] if vpf else v)
            assert (got[b].cpu() - ref).abs().max().item() < 2e-5
    G.record("uni_corr_softmax_pv_batched", "precision %d, K=%d, %s values" % (prec, K, "per-frame" if vpf else "shared"),
             "B=%d R=%d Q=%d" % (B, R, Q), {}, [ge, gc, gv, go, gw_], workspace_bytes=need)


def three_lines_grads(dtype, er, ec, v, g_):
    """er (B,R,128), ec (B,Q,128), v (B,K,R), g_ (B,K,Q) on the CPU: out, lse and the three gradients of unicorn.py:321-326"""
    a, b, c = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (er, ec, v))
    s = a @ b.transpose(1, 2)
    o = c @ torch.softmax(s, dim=1)
    o.backward(g_.cpu().to(dtype))
    return o.detach(), torch.logsumexp(s.detach(), dim=1), a.grad, b.grad, c.grad


@pytest.mark.parametrize("B,R,Q,K,shared", [(1, 150, 140, 17, False), (1, 20, 300, 2, False), (1, 300, 11, 2, False), (3, 130, 70, 9, False),
                                            (2, 33, 7, 1, False), (1, 7, 33, 3, False), (3, 90, 75, 2, True), (2, 1500, 1300, 3, False)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_corr_lse_and_backward(L, B, R, Q, K, shared, dtype):
    """uni_corr_softmax_pv_lse / _bwd (+ the _f64 pair) with the workspace at exactly uni_corr_bwd_workspace_bytes; every NULL-output
    combination of test_partial_requires_grad_and_layouts; shared value rows (grad_values (K,R), summed over the frames).  Bounds of
    test_corr_backward_gpu.py: fp64 1e-12; fp32 4 x the CPU fp32 error of the same lines (out: its own, gradients: the largest of the
    three), lse 2e-5 x max(1, |lse|)."""
    f64 = dtype == torch.float64
    g = torch.Generator().manual_seed(100 + K + R)
    er = (0.4 * torch.randn(B, R, 128, generator=g)).to(dtype).cuda()
    ec = (0.4 * torch.randn(B, Q, 128, generator=g)).to(dtype).cuda()
    v = torch.rand((K, R) if shared else (B, K, R), generator=g).to(dtype).cuda()
    g_ = torch.randn(B, K, Q, generator=g).to(dtype).cuda()
    vfull = v.unsqueeze(0).expand(B, -1, -1) if shared else v
    r64 = three_lines_grads(torch.float64, er, ec, vfull, g_)
    r32 = three_lines_grads(torch.float32, er, ec, vfull, g_)
    if shared:
        r64, r32 = r64[:4] + (r64[4].sum(0),), r32[:4] + (r32[4].sum(0),)
    need = 0 if f64 else L.lib().uni_corr_bwd_workspace_bytes(B, R, Q, K)
    lib, vpf = L.lib(), 0 if shared else 1

    def fwd(e0, e1, vv, o, l, ws):
        if f64:
            return lib.uni_corr_softmax_pv_lse_f64(P(e0), P(e1), P(vv), P(o), P(l), B, R, Q, 128, K, vpf, L.stream_ptr())
        return lib.uni_corr_softmax_pv_lse(P(e0), P(e1), P(vv), P(o), P(l), B, R, Q, 128, K, vpf, 0, P(ws), need, L.stream_ptr())

    def bwd(e0, e1, vv, o, l, gg, a, b, c, ws):
        if f64:
            return lib.uni_corr_softmax_pv_bwd_f64(P(e0), P(e1), P(vv), P(o), P(l), P(gg), P(a), P(b), P(c), B, R, Q, 128, K, vpf, L.stream_ptr())
        return lib.uni_corr_softmax_pv_bwd(P(e0), P(e1), P(vv), P(o), P(l), P(gg), P(a), P(b), P(c), B, R, Q, 128, K, vpf, 0, P(ws), need, L.stream_ptr())
    pws = None if f64 else torch.empty(need, device=DEV, dtype=torch.uint8)
    po, pl = torch.empty((B, K, Q), device=DEV, dtype=dtype), torch.empty((B, Q), device=DEV, dtype=dtype)
    L.check(fwd(er, ec, v, po, pl, pws), "corr_lse")
    ge, gc, gv = gin("e_ref", er.reshape(B * R, 128)), gin("e_cur", ec.reshape(B * Q, 128)), gin("values", v.reshape(-1, R))
    go, gl = gout("out", B * K, Q, dtype), gout("lse", B, Q, dtype)
    gw_ = None if f64 else gws("workspace", need)
    L.check(fwd(ge, gc, gv, go, gl, gw_), "corr_lse")
    sync_check(ge, gc, gv, go, gl, gw_)
    go.check_equal(po)
    gl.check_equal(pl)
    own = [relmax(b_, a_) for a_, b_ in zip(r64, r32)]
    yard = [own[0], None] + [max(own[2:])] * 3
    if f64:
        assert relmax(go.payload().reshape(B, K, Q), r64[0]) <= 1e-12 and relmax(gl.payload(), r64[1]) <= 1e-12
    else:
        assert relmax(go.payload().reshape(B, K, Q), r64[0]) <= 4 * yard[0]
        assert float((gl.payload().double().cpu() - r64[1]).abs().max()) < 2e-5 * max(1.0, float(r64[1].abs().max()))
    G.record("uni_corr_softmax_pv_lse" + ("_f64" if f64 else ""), "precision 0, K=%d, %s values" % (K, "shared" if shared else "per-frame"),
             "B=%d R=%d Q=%d" % (B, R, Q), {}, [ge, gc, gv, go, gl, gw_], workspace_bytes=need)
    if not f64:                                  # the forward's other operand formats behind the same entry (the backward is precision 0 only);
        # precision 3 has no bar for this entry in the existing tests: it is held to the plain call and the guards
        for prec in (2, 3):
            po2, pl2 = torch.empty_like(po), torch.empty_like(pl)
            L.check(lib.uni_corr_softmax_pv_lse(P(er), P(ec), P(v), P(po2), P(pl2), B, R, Q, 128, K, vpf, prec, P(pws), need, L.stream_ptr()), "corr_lse")
            go2, gl2, gw2 = gout("out", B * K, Q, dtype), gout("lse", B, Q, dtype), gws("workspace", need)
            L.check(lib.uni_corr_softmax_pv_lse(P(ge), P(gc), P(gv), P(go2), P(gl2), B, R, Q, 128, K, vpf, prec, P(gw2), need, L.stream_ptr()), "corr_lse")
            sync_check(ge, gc, gv, go2, gl2, gw2)
            go2.check_equal(po2)
            gl2.check_equal(pl2)
            if prec == 2:                        # test_lse_forward_is_bitwise_the_existing_forward / test_corr_softmax_pv: 2e-5
                assert float((go2.payload().double().cpu().reshape(B, K, Q) - r64[0]).abs().max()) < 2e-5 * max(1.0, float(r64[0].abs().max()))
                assert float((gl2.payload().double().cpu() - r64[1]).abs().max()) < 2e-5 * max(1.0, float(r64[1].abs().max()))
            G.record("uni_corr_softmax_pv_lse", "precision %d, K=%d, %s values" % (prec, K, "shared" if shared else "per-frame"),
                     "B=%d R=%d Q=%d" % (B, R, Q), {}, [ge, gc, gv, go2, gl2, gw2], workspace_bytes=need)
    rows_v = K if shared else B * K
    full = None                                  # the plain outputs of the full combination: every partial one must equal them bit for bit
    for needs in ((True, True, True), (False, True, False), (True, True, False), (True, False, True), (False, False, True)):
        pa = torch.empty((B * R, 128), device=DEV, dtype=dtype) if needs[0] else None
        pb = torch.empty((B * Q, 128), device=DEV, dtype=dtype) if needs[1] else None
        pc = torch.empty((rows_v, R), device=DEV, dtype=dtype) if needs[2] else None
        L.check(bwd(er, ec, v, po, pl, g_, pa, pb, pc, pws), "corr_bwd")
        gi = [gin("e_ref", er.reshape(B * R, 128)), gin("e_cur", ec.reshape(B * Q, 128)), gin("values", v.reshape(-1, R)),
              gin("out", po.reshape(B * K, Q)), gin("lse", pl), gin("grad_out", g_.reshape(B * K, Q))]
        oa = gout("grad_e_ref", B * R, 128, dtype) if needs[0] else None
        ob = gout("grad_e_cur", B * Q, 128, dtype) if needs[1] else None
        oc = gout("grad_values", rows_v, R, dtype) if needs[2] else None
        gw2 = None if f64 else gws("workspace", need)
        L.check(bwd(gi[0], gi[1], gi[2], gi[3], gi[4], gi[5], oa, ob, oc, gw2), "corr_bwd")
        sync_check(*(gi + [oa, ob, oc, gw2]))
        if all(needs):
            full = (pa, pb, pc)
        for i, (o_, p_, w64, y) in enumerate(zip((oa, ob, oc), (pa, pb, pc), r64[2:], yard[2:])):
            if o_ is None:
                continue
            o_.check_equal(p_)
            if all(needs):
                e = relmax(o_.payload().reshape(w64.shape), w64)
                assert e <= (1e-12 if f64 else 4 * y), (o_.name, e, y)
            else:                                # test_partial_requires_grad_and_layouts: one writer per element, the same bits
                o_.check_equal(full[i], "the call with all three outputs")
        G.record("uni_corr_softmax_pv_bwd" + ("_f64" if f64 else ""), "outputs %s, K=%d, %s values" % (
            "".join("x" if n else "-" for n in needs), K, "shared" if shared else "per-frame"), "B=%d R=%d Q=%d" % (B, R, Q), {},
            gi + [oa, ob, oc, gw2], workspace_bytes=need)


# ------------------------------------------------------------------------------------------------------------------------------
# box, label and mask operators
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H8,W8", [(2, 44, 76), (1, 50, 42), (3, 100, 160)])
def test_prior_pyramid(L, K, H8, W8):
    """44 x 76 = the 352 x 608 geometry (W8 / 4 = 19 odd); 50 x 42: neither side a multiple of 4"""
    c = torch.rand(1, K, H8, W8, generator=torch.Generator().manual_seed(9))
    ref = uo.prior_pyramid(c)
    cd = c.cuda()
    p16, p32 = torch.empty((K * (H8 // 2), W8 // 2), device=DEV), torch.empty((K * (H8 // 4), W8 // 4), device=DEV)
    L.check(L.lib().uni_prior_pyramid(P(cd), P(p16), P(p32), K, H8, W8, L.stream_ptr()), "prior_pyramid")
    gi = gin("p8", cd.reshape(K * H8, W8))
    o16, o32 = gout("p16", K * (H8 // 2), W8 // 2, torch.float32), gout("p32", K * (H8 // 4), W8 // 4, torch.float32)
    L.check(L.lib().uni_prior_pyramid(P(gi), P(o16), P(o32), K, H8, W8, L.stream_ptr()), "prior_pyramid")
    sync_check(gi, o16, o32)
    o16.check_equal(p16)
    o32.check_equal(p32)
    assert torch.allclose(o16.payload().cpu().reshape(ref[1].shape), ref[1], atol=1e-6)
    assert torch.allclose(o32.payload().cpu().reshape(ref[2].shape), ref[2], atol=1e-6)
    G.record("uni_prior_pyramid", "-", "K=%d H8=%d W8=%d" % (K, H8, W8), {}, [gi, o16, o32])


@pytest.mark.parametrize("H,W", [(352, 608), (800, 1280)])
def test_label_map_s8(L, H, W):
    for box in ([320.0, 200.0, 640.0, 400.0], [3.4, 7.5, W - 0.4, H - 99.5], [-20.0, -5.0, 50.5, 2000.0], [100.5, 100.5, 100.5, 300.0]):
        ref = uo.label_map_s8(torch.tensor(box), H, W)
        bd = torch.tensor(box).cuda()
        n = (H // 8) * (W // 8)
        plain = torch.empty((1, n), device=DEV)
        L.check(L.lib().uni_label_map_s8(P(bd), P(plain), H, W, L.stream_ptr()), "label_map")
        gb, go = gin("box_xyxy", bd), gout("out", H // 8, W // 8, torch.float32)
        L.check(L.lib().uni_label_map_s8(P(gb), P(go), H, W, L.stream_ptr()), "label_map")
        sync_check(gb, go)
        go.check_equal(plain)
        assert torch.equal(go.payload().cpu().reshape(ref.shape), ref), box
    G.record("uni_label_map_s8", "-", "H=%d W=%d" % (H, W), {}, [gb, go])


def test_sample_embeddings(L):
    """ld_boxes = 7 (the (n, 7) detection rows) with NaN in the three trailing columns; boxes whose centre the border padding clips"""
    g = torch.Generator().manual_seed(4)
    H8, W8, Cc, n = 40, 64, 128, 50
    emb = torch.randn(1, Cc, H8, W8, generator=g)
    boxes = torch.rand(n, 4, generator=g) * torch.tensor([512, 320, 512, 320.0])
    boxes[0] = torch.tensor([-30.0, -10.0, 5.0, 6.0])
    boxes[1] = torch.tensor([500.0, 300.0, 530.0, 345.0])
    boxes[2] = torch.tensor([0.0, 0.0, 0.0, 0.0])
    boxes[3] = torch.tensor([511.0, 319.0, 512.0, 320.0])
    ref = uo.sample_instance_embeddings(emb, boxes)
    ed, bd = emb.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, Cc), boxes.cuda()
    plain = torch.empty((n, Cc), device=DEV)
    L.check(L.lib().uni_sample_embeddings(P(ed), H8, W8, Cc, P(bd), 4, n, 8.0, P(plain), L.stream_ptr()), "sample_embeddings")
    ge, gb, go = gin("embed_nhwc", ed), gin("boxes_xyxy", bd, ld=7), gout("out", n, Cc, torch.float32)
    L.check(L.lib().uni_sample_embeddings(P(ge), H8, W8, Cc, P(gb), 7, n, 8.0, P(go), L.stream_ptr()), "sample_embeddings")
    sync_check(ge, gb, go)
    go.check_equal(plain)
    assert torch.allclose(go.payload().cpu(), ref, atol=1e-5)
    G.record("uni_sample_embeddings", "-", "n=%d H8=%d W8=%d C=%d" % (n, H8, W8, Cc), {"ld_boxes": 7}, [ge, gb, go])


def _condinst_inputs(n, H8, W8, seed):
    g = torch.Generator().manual_seed(seed)
    mf = torch.randn(1, 8, H8, W8, generator=g)
    um = torch.randn(1, 144, H8, W8, generator=g)
    params = torch.randn(n, 169, generator=g) * 0.5
    loc = torch.rand(n, 2, generator=g) * torch.tensor([W8 * 8.0, H8 * 8.0])
    lvl = (torch.arange(n) % 5).to(torch.int32)
    return mf, um, params, loc, lvl


@pytest.mark.parametrize("n", [0, 1, 11])
def test_condinst_masks(L, n):
    """ldp = 176 > 169, the workspace at exactly the documented n*H8*W8*(1+r*r)*4 bytes, n = 0 (nothing may be touched), 1, and 11 (the
    8-instance chunk has a ragged last group of 3)"""
    H8, W8, r, d_rate, ldp = 20, 28, 4, 2, 176
    mf, um, params, loc, lvl = _condinst_inputs(max(n, 1), H8, W8, 8)
    mfd = mf.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, 8)
    umd = um.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, 144)
    pd, ld_, lv = params.cuda(), loc.cuda(), lvl.cuda()
    Ho, Wo = d_rate * r * H8, d_rate * r * W8
    rows = max(n, 1)
    need = n * H8 * W8 * (1 + r * r) * 4
    plain, pws = torch.zeros((rows * Ho, Wo), device=DEV), torch.empty(max(need, 16), device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_condinst_masks(P(mfd), P(umd), P(pd), 169, P(ld_), P(lv), n, H8, W8, r, d_rate, P(plain), P(pws), need, L.stream_ptr()), "condinst")
    gi = [gin("mask_feats", mfd), gin("up_masks", umd), gin("params", pd, ld=ldp), gin("inst_loc", ld_), gin("inst_lvl", lv, poison=0x7F)]
    go, gw_ = gout("out", rows * Ho, Wo, torch.float32), gws("workspace", max(need, 16))
    L.check(L.lib().uni_condinst_masks(P(gi[0]), P(gi[1]), P(gi[2]), ldp, P(gi[3]), P(gi[4]), n, H8, W8, r, d_rate, P(go), P(gw_), need,
                                       L.stream_ptr()), "condinst")
    torch.cuda.synchronize()
    G.check_all(*gi)
    gw_.check()
    if n == 0:
        go.check(complete=False)
        assert bool((go.base == G.FILL).all()) and bool((gw_.base == G.FILL).all())          # n == 0: neither buffer is touched
    else:
        go.check()
        go.check_equal(plain)
        cfg = uo.CONFIGS["unicorn_track_tiny_mask"]
        ref = uo.aligned_bilinear(uo.dynamic_mask_head(cfg, mf, params, loc, lvl.long(), um), 2)
        assert torch.allclose(go.payload().cpu().reshape(ref.shape), ref, atol=2e-5)
    G.record("uni_condinst_masks", "n=%d" % n, "H8=%d W8=%d r=%d d_rate=%d" % (H8, W8, r, d_rate), {"ldp": ldp}, gi + [go, gw_], workspace_bytes=need)


@pytest.mark.parametrize("H8,W8,rr,H,W", [(25, 40, 0.8333333, 250, 390), (40, 64, 1.4988, 214, 342), (40, 64, 2.7, 118, 189)])
@pytest.mark.parametrize("n", [0, 1, 11])
def test_condinst_masks_u8(L, n, H8, W8, rr, H, W):
    """the fused CondInst -> resize -> threshold call (staged-LDS and sample-per-tap variants) with both outputs guarded; bit-identical to
    the plain call and to uni_condinst_masks + uni_mask_resize (test_condinst_resized_fused_equals_two_pass); n = 0 touches nothing"""
    r, d_rate, ldp, thr = 4, 2, 172, 0.3
    if n == 0:
        mf, um, params, loc, lvl = _condinst_inputs(1, H8, W8, H8 * 7 + W)
        gi = [gin("mask_feats", mf.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, 8)),
              gin("up_masks", um.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, 144)), gin("params", params.cuda(), ld=ldp),
              gin("inst_loc", loc.cuda()), gin("inst_lvl", lvl.cuda(), poison=0x7F)]
        op, ob, gw_ = gout("out_prob", H, W, torch.float32), gout("out_bin", H, W, torch.uint8), gws("workspace", 16)
        L.check(L.lib().uni_condinst_masks_u8(P(gi[0]), P(gi[1]), P(gi[2]), ldp, P(gi[3]), P(gi[4]), 0, H8, W8, r, d_rate, rr, H, W, thr, P(op), P(ob),
                                              P(gw_), 0, L.stream_ptr()), "condinst_u8")
        torch.cuda.synchronize()
        G.check_all(*gi)
        for b in (op, ob, gw_):
            b.check(complete=False)
            assert bool((b.base == G.FILL).all()), b.name          # n == 0: neither output nor the workspace is touched
        G.record("uni_condinst_masks_u8", "n=0 r=%.4f" % rr, "H8=%d W8=%d -> %dx%d" % (H8, W8, H, W), {"ldp": ldp}, gi + [op, ob, gw_])
        return
    mf, um, params, loc, lvl = _condinst_inputs(n, H8, W8, H8 * 7 + W)
    mfd = mf.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, 8)
    umd = um.permute(0, 2, 3, 1).contiguous().cuda().reshape(H8 * W8, 144)
    pd, ld_, lv = params.cuda(), loc.cuda(), lvl.cuda()
    need = n * H8 * W8 * (1 + r * r) * 4
    Hn, Wn = d_rate * r * H8, d_rate * r * W8
    pws = torch.empty(need, device=DEV, dtype=torch.uint8)
    pp, pb = torch.full((n * H, W), -1.0, device=DEV), torch.full((n * H, W), 9, device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_condinst_masks_u8(P(mfd), P(umd), P(pd), 169, P(ld_), P(lv), n, H8, W8, r, d_rate, rr, H, W, thr, P(pp), P(pb), P(pws), need,
                                          L.stream_ptr()), "condinst_u8")
    full = torch.empty((n * Hn, Wn), device=DEV)
    L.check(L.lib().uni_condinst_masks(P(mfd), P(umd), P(pd), 169, P(ld_), P(lv), n, H8, W8, r, d_rate, P(full), P(pws), need, L.stream_ptr()), "condinst")
    tp, tb = torch.empty((n * H, W), device=DEV), torch.empty((n * H, W), device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_mask_resize(P(full), n, Hn, Wn, rr, H, W, thr, P(tp), P(tb), L.stream_ptr()), "mask_resize")
    gi = [gin("mask_feats", mfd), gin("up_masks", umd), gin("params", pd, ld=ldp), gin("inst_loc", ld_), gin("inst_lvl", lv, poison=0x7F)]
    op, ob, gw_ = gout("out_prob", n * H, W, torch.float32), gout("out_bin", n * H, W, torch.uint8), gws("workspace", need)
    L.check(L.lib().uni_condinst_masks_u8(P(gi[0]), P(gi[1]), P(gi[2]), ldp, P(gi[3]), P(gi[4]), n, H8, W8, r, d_rate, rr, H, W, thr, P(op), P(ob),
                                          P(gw_), need, L.stream_ptr()), "condinst_u8")
    sync_check(*(gi + [op, ob, gw_]))
    op.check_equal(pp).check_equal(tp, "uni_condinst_masks + uni_mask_resize")
    ob.check_equal(pb).check_equal(tb, "uni_condinst_masks + uni_mask_resize")
    G.record("uni_condinst_masks_u8", "n=%d r=%.4f" % (n, rr), "H8=%d W8=%d -> %dx%d" % (H8, W8, H, W), {"ldp": ldp}, gi + [op, ob, gw_], workspace_bytes=need)


@pytest.mark.parametrize("shape,size,swap", [((1080, 1920), (800, 1280), True), ((480, 640), (800, 1280), True),
                                             ((375, 1242), (800, 1280), False), ((97, 61), (320, 320), True),
                                             ((800, 1280), (800, 1280), False), ((2160, 3840), (800, 1280), True)])      # test_letterbox_device's six
def test_letterbox(L, shape, size, swap):
    """a guarded uint8 image: every byte is a legal pixel, so the image stays below 200 and the guards hold 0xFF -- a stray tap changes the
    bit-exact comparison with the oracle"""
    import letterbox_oracle as lo
    img = np.random.default_rng(shape[0] + shape[1]).integers(0, 200, shape + (3,), dtype=np.uint8)
    ref, r_ref = lo.letterbox(img, size, swap)
    h, w = shape
    H, W = size
    imd = torch.from_numpy(img).cuda()
    plain, r1, r2 = torch.empty((3 * H, W), device=DEV), C.c_double(0), C.c_double(0)
    L.check(L.lib().uni_letterbox(P(imd), h, w, int(swap), H, W, P(plain), C.byref(r1), L.stream_ptr()), "letterbox")
    gi, go = gin("img_hwc", imd.reshape(h, w * 3), poison=0xFF), gout("out_chw", 3 * H, W, torch.float32)
    L.check(L.lib().uni_letterbox(P(gi), h, w, int(swap), H, W, P(go), C.byref(r2), L.stream_ptr()), "letterbox")
    sync_check(gi, go)
    go.check_equal(plain)
    assert r1.value == r_ref and r2.value == r_ref
    assert np.array_equal(go.payload().cpu().numpy().reshape(3, H, W), ref)
    G.record("uni_letterbox", "swap_rb %d" % swap, "%dx%d -> %dx%d" % (h, w, H, W), {}, [gi, go])


@pytest.mark.parametrize("nch", [6, 13])
def test_decode_outputs(L, nch):
    g = torch.Generator().manual_seed(2)
    H, W, B = 320, 352, 2
    levels = [torch.randn(B, nch, H // s_, W // s_, generator=g) for s_ in (8, 16, 32)]
    exp, _ = uo.decode_outputs([t.clone() for t in levels])
    raw = torch.cat([t.flatten(2) for t in levels], 2).permute(0, 2, 1).contiguous().cuda()
    A = raw.shape[1]
    plain = raw.clone()
    L.check(L.lib().uni_decode_outputs(P(plain), B, H, W, nch, L.stream_ptr()), "decode")
    go = gout("outputs", B * A, nch, torch.float32, init=raw)
    L.check(L.lib().uni_decode_outputs(P(go), B, H, W, nch, L.stream_ptr()), "decode")
    sync_check(go)
    go.check_equal(plain)
    assert torch.allclose(go.payload().cpu().reshape(exp.shape), exp, rtol=1e-6, atol=1e-5)
    G.record("uni_decode_outputs", "nch=%d" % nch, "B=%d H=%d W=%d A=%d" % (B, H, W, A), {}, [go])


def test_nms(L):
    g = torch.Generator().manual_seed(4)
    n = 700
    xy = torch.rand(n, 2, generator=g) * 300
    boxes = torch.cat([xy, xy + torch.rand(n, 2, generator=g) * 80 + 5], 1)
    scores = torch.rand(n, generator=g)
    ref = uo.nms(boxes, scores, 0.5)
    need = L.lib().uni_nms_workspace_bytes(n)
    bd, sd = boxes.cuda(), scores.cuda()
    pk, pn, pws = torch.full((n,), -1, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV, dtype=torch.int32), torch.empty(need, device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_nms(P(bd), P(sd), n, 0.5, P(pk), P(pn), P(pws), need, L.stream_ptr()), "nms")
    gb, gs = gin("boxes_xyxy", bd), gin("scores", sd)
    ok, on, gw_ = gout("keep_idx", 1, n, torch.int32), gout("n_out", 1, 1, torch.int32), gws("workspace", need)
    L.check(L.lib().uni_nms(P(gb), P(gs), n, 0.5, P(ok), P(on), P(gw_), need, L.stream_ptr()), "nms")
    torch.cuda.synchronize()
    G.check_all(gb, gs, on, gw_)
    ok.check(complete=False)                     # only the first n_out entries are written
    m = int(on.view[0, 0])
    assert m == int(pn[0]) == ref.numel() and 0 < m < n
    assert torch.equal(ok.view[0, :m], pk[:m]) and torch.equal(ok.view[0, :m].cpu().long(), ref)
    assert bool((ok.view[0, m:].view(torch.uint8) == G.FILL).all())
    G.record("uni_nms", "-", "n=%d kept=%d" % (n, m), {}, [gb, gs, ok, on, gw_], workspace_bytes=need)


@pytest.mark.parametrize("A,nc,agnostic,max_det", [(2100, 1, False, 2100), (2100, 1, False, 20), (21000, 8, True, 33), (333, 3, False, 5), (21000, 8, False, 21000)])
def test_postprocess(L, A, nc, agnostic, max_det):
    """ld = 5 + nc + 3 with NaN in the trailing columns, the workspace at exactly uni_postprocess_workspace_bytes(A), max_det below the
    number of survivors (the clamp: det_out / keep_idx hold max_det rows and not one more); test_postprocess_device's equalities"""
    pred = planted_pred(A, nc, seed=A + nc)
    ref_in = pred.clone()
    ref_det, ref_idx = uo.postprocess(ref_in, nc, 0.2, 0.45, class_agnostic=agnostic, return_index=True)[0]
    ld, need = 5 + nc + 3, L.lib().uni_postprocess_workspace_bytes(A)
    kept = min(max_det, ref_det.shape[0])
    assert ref_det.shape[0] > 10 and (max_det >= A or max_det < ref_det.shape[0])
    pp, pdet = pred[0].clone().cuda(), torch.full((max_det, 7), -1.0, device=DEV)
    pk, pn, pws = torch.full((max_det,), -1, device=DEV, dtype=torch.int32), torch.zeros(1, device=DEV, dtype=torch.int32), torch.empty(need, device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_postprocess(P(pp), A, 5 + nc, nc, 0.2, 0.45, int(agnostic), max_det, P(pdet), P(pk), P(pn), P(pws), need, L.stream_ptr()), "post")
    gp = gin("pred", pred[0].cuda(), ld=ld)          # in-place input / output: NaN around the rows and in the trailing columns
    od, ok, on = gout("det_out", max_det, 7, torch.float32), gout("keep_idx", 1, max_det, torch.int32), gout("n_out", 1, 1, torch.int32)
    gw_ = gws("workspace", need)
    L.check(L.lib().uni_postprocess(P(gp), A, ld, nc, 0.2, 0.45, int(agnostic), max_det, P(od), P(ok), P(on), P(gw_), need, L.stream_ptr()), "post")
    torch.cuda.synchronize()
    gp.check(complete=False)
    G.check_all(on, gw_)
    od.check(complete=False)
    ok.check(complete=False)
    assert int(on.view[0, 0]) == int(pn[0]) == kept
    assert torch.equal(od.view[:kept], pdet[:kept]) and torch.equal(ok.view[0, :kept], pk[:kept])
    assert torch.equal(od.view[:kept].cpu(), ref_det[:kept]) and torch.equal(ok.view[0, :kept].cpu().long(), ref_idx[:kept])
    assert bool((od.view[kept:].contiguous().view(torch.uint8) == G.FILL).all()) and bool((ok.view[0, kept:].view(torch.uint8) == G.FILL).all())
    gp.check_equal(pp)
    assert torch.equal(gp.payload().cpu()[:, :4], ref_in[0, :, :4])          # corners written back in place
    G.record("uni_postprocess", "nc=%d agnostic=%d max_det=%d" % (nc, agnostic, max_det), "A=%d survivors=%d" % (A, ref_det.shape[0]), {"ld": ld},
             [gp, od, ok, on, gw_], workspace_bytes=need)


@pytest.mark.parametrize("geo", [(96, 160, 0.8333333, 110, 190), (100, 160, 1.37, 70, 100), (50, 64, 0.7, 90, 40), (80, 128, 0.5, 160, 256)])
def test_mask_resize(L, geo):
    Hn, Wn, r, H, W = geo
    N, thr = 4, 0.3
    m = torch.rand(N, Hn, Wn, generator=torch.Generator().manual_seed(Hn + W))
    ref = mo.resize_bilinear(m.numpy(), r, H, W)
    md = m.cuda()
    pp, pb = torch.empty((N * H, W), device=DEV), torch.empty((N * H, W), device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_mask_resize(P(md), N, Hn, Wn, r, H, W, thr, P(pp), P(pb), L.stream_ptr()), "mask_resize")
    gi, op, ob = gin("masks", md.reshape(N * Hn, Wn)), gout("out_prob", N * H, W, torch.float32), gout("out_bin", N * H, W, torch.uint8)
    L.check(L.lib().uni_mask_resize(P(gi), N, Hn, Wn, r, H, W, thr, P(op), P(ob), L.stream_ptr()), "mask_resize")
    sync_check(gi, op, ob)
    op.check_equal(pp)
    ob.check_equal(pb)
    assert np.array_equal(op.payload().cpu().numpy().reshape(N, H, W), ref)
    assert np.array_equal(ob.payload().cpu().numpy().reshape(N, H, W), (ref > np.float32(thr)).astype(np.uint8))
    G.record("uni_mask_resize", "r=%.4f" % r, "%dx%d -> %dx%d" % (Hn, Wn, H, W), {}, [gi, op, ob])


def test_vos_merge(L):
    g = np.random.default_rng(3)
    Hn, Wn, r, H, W = 100, 160, 0.75, 130, 200
    probs = g.random((4, Hn, Wn), dtype=np.float32)
    probs[0, :20] = 0.0
    probs[1, 20:40] = 1.0
    probs[2] = probs[3]
    ids, init_ids = [4, 2, 9, 6], [11, 1]
    init = (g.random((2, H, W)) > 0.8).astype(np.uint8)
    ref = mo.soft_aggregate(mo.resize_bilinear(probs, r, H, W), [str(i) for i in ids], init, [str(i) for i in init_ids])
    pd, idd = torch.from_numpy(probs).cuda(), torch.tensor(ids, dtype=torch.int32).cuda()
    imd, iid = torch.from_numpy(init).cuda(), torch.tensor(init_ids, dtype=torch.int32).cuda()
    plain = torch.empty((H, W), device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_vos_merge(P(pd), P(idd), 4, Hn, Wn, r, P(imd), P(iid), 2, H, W, P(plain), L.stream_ptr()), "vos_merge")
    gi = [gin("probs", pd.reshape(4 * Hn, Wn)), gin("prob_ids", idd, poison=0x7F), gin("init_masks", imd.reshape(2 * H, W), poison=0x7F),
          gin("init_ids", iid, poison=0x7F)]
    go = gout("out", H, W, torch.uint8)
    L.check(L.lib().uni_vos_merge(P(gi[0]), P(gi[1]), 4, Hn, Wn, r, P(gi[2]), P(gi[3]), 2, H, W, P(go), L.stream_ptr()), "vos_merge")
    sync_check(*(gi + [go]))
    go.check_equal(plain)
    assert np.array_equal(go.payload().cpu().numpy(), ref)
    G.record("uni_vos_merge", "-", "%dx%d -> %dx%d, K1=4 K2=2" % (Hn, Wn, H, W), {}, gi + [go])


def _mots_masks():
    g = np.random.default_rng(4)
    H, W = 135, 241
    masks = np.zeros((6, H, W), dtype=np.uint8)
    for n in range(5):
        y0, x0 = g.integers(0, H - 40), g.integers(0, W - 60)
        masks[n, y0:y0 + g.integers(10, 40), x0:x0 + g.integers(10, 60)] = 1
    masks[3] |= (g.random((H, W)) < 0.05).astype(np.uint8)
    masks[4, 0, 0] = 1
    return masks, H, W


def test_mots_overlap_free(L):
    masks, H, W = _mots_masks()
    md = torch.from_numpy(masks).cuda()
    plain = torch.empty_like(md)
    L.check(L.lib().uni_mots_overlap_free(P(md), 6, H, W, P(plain), L.stream_ptr()), "overlap_free")
    gi, go = gin("masks", md.reshape(6 * H, W), poison=0x7F), gout("out", 6 * H, W, torch.uint8)
    L.check(L.lib().uni_mots_overlap_free(P(gi), 6, H, W, P(go), L.stream_ptr()), "overlap_free")
    sync_check(gi, go)
    go.check_equal(plain.reshape(6 * H, W))
    assert np.array_equal(go.payload().cpu().numpy().reshape(6, H, W), mo.overlap_free(masks))
    G.record("uni_mots_overlap_free", "-", "N=6 H=%d W=%d" % (H, W), {}, [gi, go])


@pytest.mark.parametrize("kind", ["normal", "max_runs overflow", "max_chars binding"])
def test_rle_encode(L, kind):
    """a normal case; a dense mask with far more runs than max_runs (out_len must be -1); max_chars as the binding limit.  In all three
    nothing outside the payloads of out_chars, out_len, counts, n_runs and the EXACT-size workspace may change -- the overflowed attempt of
    test_mots_overlap_free_and_rle_device's retry included."""
    if kind == "max_runs overflow":
        masks = (np.random.default_rng(4).random((2, 64, 96)) < 0.5).astype(np.uint8)
        max_runs, max_chars = 64, 6 * 65
    else:
        masks = mo.overlap_free(_mots_masks()[0])
        max_runs = 1 << 14
        max_chars = 6 * (max_runs + 1) if kind == "normal" else 40
    N, H, W = masks.shape
    exp = [mo.mask_to_rle_string(m) for m in masks]
    true_runs = [len(mo.rle_from_string(s)) for s in exp]
    need = L.lib().uni_rle_workspace_bytes(N, H, W, max_runs)
    md = torch.from_numpy(masks).cuda()
    pc, pl = torch.zeros((N, max_chars), device=DEV, dtype=torch.uint8), torch.zeros(N, device=DEV, dtype=torch.int32)
    pcnt, pnr = torch.zeros((N, max_runs + 1), device=DEV, dtype=torch.int32), torch.zeros(N, device=DEV, dtype=torch.int32)
    pws = torch.empty(need, device=DEV, dtype=torch.uint8)
    L.check(L.lib().uni_rle_encode(P(md), N, H, W, max_runs, max_chars, P(pc), P(pl), P(pcnt), P(pnr), P(pws), need, L.stream_ptr()), "rle")
    gi = gin("masks", md.reshape(N * H, W), poison=0x7F)
    oc, ol = gout("out_chars", N, max_chars, torch.uint8), gout("out_len", 1, N, torch.int32)
    ocnt, onr, gw_ = gout("counts", N, max_runs + 1, torch.int32), gout("n_runs", 1, N, torch.int32), gws("workspace", need)
    L.check(L.lib().uni_rle_encode(P(gi), N, H, W, max_runs, max_chars, P(oc), P(ol), P(ocnt), P(onr), P(gw_), need, L.stream_ptr()), "rle")
    torch.cuda.synchronize()
    G.check_all(gi, ol, onr, gw_)
    oc.check(complete=False)
    ocnt.check(complete=False)
    ol.check_equal(pl)
    onr.check_equal(pnr)
    lens = ol.view[0].cpu().tolist()
    for i in range(N):
        fits = len(exp[i]) <= max_chars and true_runs[i] <= max_runs + 1
        if kind == "max_runs overflow":
            assert lens[i] == -1
        elif fits or kind == "normal":
            assert lens[i] == len(exp[i]) and oc.view[i, :lens[i]].cpu().numpy().tobytes() == exp[i]
            assert torch.equal(oc.view[i, :lens[i]], pc[i, :lens[i]])
            nr = int(onr.view[0, i])
            assert torch.equal(ocnt.view[i, :nr], pcnt[i, :nr])
        else:
            assert lens[i] == -1
    if kind == "max_chars binding":
        assert -1 in lens and max(lens) > 0          # the limit binds for some masks and not for others
    G.record("uni_rle_encode", kind, "N=%d H=%d W=%d max_runs=%d max_chars=%d" % (N, H, W, max_runs, max_chars), {}, [gi, oc, ol, ocnt, onr, gw_],
             workspace_bytes=need)
