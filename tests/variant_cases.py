"""The executable map "what the engine dispatches -> which kernel-level parity case covers it".

Every launcher of libunicorn_hip.so reports the kernel instantiation it launches as a tag (uni_variant_trace, include/unicorn_hip.h).
CASES maps a tag to ONE parity case: a context-free entry point, the smallest arguments that make the launcher emit the tag (derived from
the dispatcher; tests/test_variant_census_gpu.py asserts the tag, so a retuned crossover that moves the shape elsewhere fails there), the fp64
CPU reference, the bound and the existing test the bound is restated from.  CTX_ONLY lists the tag patterns that have no context-free entry
point and names the model-level test that runs them.  Data and small helpers only: no GPU work at import."""
import ctypes
import re


def parse_trace(text):
    """'tag\\tcount\\n' lines -> {tag: count}"""
    out = {}
    for line in text.splitlines():
        if line:
            tag, n = line.rsplit("\t", 1)
            out[tag] = int(n)
    return out


def read_trace(lib):
    need = lib.uni_variant_trace_read(None, 0)
    buf = ctypes.create_string_buffer(need)
    lib.uni_variant_trace_read(buf, need)
    return parse_trace(buf.value.decode())


# ---- bounds, restated from the existing parity tables (relative to max(1, max |reference|) unless the runner says otherwise) ----
B_DWLN = {0: 1.6e-2, 1: 2e-5, 2: 2e-5}            # test_dwconv7_ln_batched_all_formats
B_LN_F32, B_LN_BF16 = 2e-5, 8e-3                    # test_layernorm (relative to max |reference|)
B_GN_F32 = 1e-4                                     # test_groupnorm_act
B_H2_ROWS = 2e-5                                    # f16x2 operand rows decoded hi + lo: format 2 of test_dwconv7_ln_batched_all_formats (same act_store* helpers)
B_BF16_ROWS = 8e-3                                  # bf16 operand rows: test_layernorm


def _dw(kernel, C, B, H, W, fmt):
    f = ("bf16", "f32", "h2")[fmt]
    return dict(tag="dwconv7_ln %s fmt=%s batched=%d" % (kernel, f, B > 1), entry="uni_dwconv7_ln_ex", args=dict(C=C, B=B, H=H, W=W, fmt=fmt),
                ref="torch fp64: F.conv2d(groups=C, padding=3) + F.layer_norm", bound=B_DWLN[fmt],
                bound_from="test_dwconv7_ln_batched_all_formats")


def _lnb(C, rows, nw, pack):
    return "lnb<C=%d,ROWS=%d,NW=%d,PACK=%d>" % (C, rows, nw, pack)


def _ln(mode, C, fmt, outF, outB, **kw):
    f = ("bf16", "f32", "h2")[fmt]
    ni = (C // 4 + 63) // 64
    ni = ni if ni <= 4 else 6
    tag = "layernorm NI=%d fmt=%s ps=%d pair=%d outF=%d outB=%d" % (ni, f, mode == "ps", mode == "pair", outF, outB)
    ref = {"rows": "torch fp64: F.layer_norm", "ps": "torch fp64: F.pixel_shuffle(F.layer_norm, 2)",
           "pair": "torch fp64: F.layer_norm, odd frames of [B][2][hw] tokens -> second output"}[mode]
    return dict(tag=tag, entry="uni_layernorm_ex", args=dict(mode=mode, C=C, fmt=fmt, outF=outF, outB=outB, **kw), ref=ref,
                bound={0: B_BF16_ROWS, 1: B_LN_F32, 2: B_H2_ROWS}[fmt], bound_from="test_layernorm" if fmt != 2 else "test_dwconv7_ln_batched_all_formats")


def _gn(C, G, act, B, M, fmt, prior=False, up_w=0, outF=False, outB=False, ldu=0, bound=None):
    f = ("bf16", "f32", "h2")[fmt]
    act_t = act if act in (0, 1, 3) else -1
    tag = "gn_apply ACT=%d FAST=%d fmt=%s batched=%d prior=%d outUp=%d outF=%d outB=%d" % (
        act_t, fmt != 1 and act_t >= 0, f, B > 1, prior, up_w > 0, outF, outB)
    return dict(tag=tag, entry="uni_groupnorm_act_ex", args=dict(C=C, G=G, act=act, B=B, M=M, fmt=fmt, prior=prior, up_w=up_w, outF=outF, outB=outB, ldu=ldu),
                ref="torch fp64: per-sample F.group_norm + activation (+ prior[m] * prior_beta[c])",
                bound=bound if bound is not None else {0: B_BF16_ROWS, 1: B_GN_F32, 2: B_H2_ROWS}[fmt],
                bound_from={0: "test_layernorm", 1: "test_groupnorm_act", 2: "test_dwconv7_ln_batched_all_formats"}[fmt])


CASE_LIST = []

# ---------------------------------------------------------------------------------------------------------------- depthwise 7x7 + LayerNorm
# launch_dwconv7_ln (csrc/norm.hip): n8 = cdiv(W, 8) * H * B * C / 4 picks 4 px (< 70k) / 8 px (< 150k) / 2 rows x 8 px; the LDS-weight
# kernels need C in {192, 256, 384, 512, 768} and cdiv(strips, strips per block) >= 384
CASE_LIST += [
    # C = 1536 is not in the LDS-weight list: ln2 with CG = 384, S = 1 (the 16-frame stride-32 map is 25 x 40; B = 4 is the smallest B with n8 >= 150k)
    _dw("ln2 CG=384 S=1", 1536, 4, 25, 40, 2),
    _dw("ln2 CG=384 S=1", 1536, 4, 25, 40, 1),
    _dw("ln2 CG=384 S=1", 1536, 4, 25, 40, 0),
]

# ---------------------------------------------------------------------------------------------------------------- LayerNorm modes
CASE_LIST += [
    # PixelShuffle(2) scatter of the operand rows (upsample stage): C = 192 (NI = 1) and 768 (NI = 3), one (7, 5) map and three stacked ones
    _ln("ps", 192, 2, False, True, B=1, h=7, w=5),
    _ln("ps", 192, 1, False, True, B=3, h=7, w=5),
    _ln("ps", 192, 0, False, True, B=3, h=7, w=5),
    _ln("ps", 768, 2, False, True, B=3, h=7, w=5),
    _ln("ps", 768, 1, False, True, B=1, h=7, w=5),
    _ln("ps", 768, 0, False, True, B=1, h=7, w=5),
    # frame-pair remap of the fp32 rows (interaction stage): tokens [3][2][35], odd frames -> the second output
    _ln("pair", 256, 2, True, True, B=3, pair_hw=35),
    _ln("pair", 256, 1, True, True, B=3, pair_hw=35),
    _ln("pair", 256, 0, True, True, B=3, pair_hw=35),
    _ln("pair", 256, 1, True, False, B=3, pair_hw=35),
]

# ---------------------------------------------------------------------------------------------------------------- GroupNorm apply modes
# launch_gn_apply: rows per grid stride = gridDim.x * 256 / (C / 8); M = 5501 (C = 256, 683 blocks -> 5464 rows) and M = 30001 (C = 48:
# C / 8 = 6 does not divide 256, the grid is rounded 683 -> 684 blocks -> 29184 rows) are no multiples of it, so both loops of the kernel run.
# The bf16 / f16x2 formats take the reciprocal-based activations (FAST): against the exact fp64 reference the f16x2 rows measured at most
# 2.8e-6 of the largest value, inside the restated 2e-5, so no bound of their own is derived for them.  The bf16 rows of the same cases
# measured 1.9e-3 .. 3.1e-3 of the largest value (bound 8e-3): that is the bf16 rounding of the stored value (half an ulp of values in
# [8, 16) is 3.1e-2, the largest outputs are 9.8 .. 16.4), three orders above the activation's own error, which the fp32 output of the bf16
# case shows directly: 2.0e-6 absolute at a largest value of 16 (bound 1e-4).
CASE_LIST += [
    _gn(256, 16, 3, 3, 5501, 1, prior=True, outF=True),
    _gn(256, 16, 3, 3, 5501, 2, prior=True, outF=True, outB=True),
    _gn(256, 16, 3, 3, 5501, 0, prior=True, outF=True, outB=True),
    _gn(48, 16, 3, 3, 30001, 1, outF=True),
    _gn(48, 16, 3, 3, 30001, 2, outB=True),
    _gn(48, 16, 3, 3, 30001, 0, outB=True),
    _gn(96, 16, 3, 3, 13 * 47, 2, up_w=13, outB=True, ldu=128),
    _gn(96, 16, 3, 3, 13 * 47, 0, up_w=13, outB=True, ldu=128),
    _gn(96, 16, 3, 3, 13 * 47, 1, up_w=13, outB=True, ldu=128),
]


# ================================================================================================================ what the census dispatches
# (variant_census.json in the suite's results directory: unicorn_track_large f16x2 800x1280 at 16 frames and one frame, unicorn_track_tiny_mask f16x2 352x608 x 3 and
# fp32 320x320).  Shapes: the smallest that reach the variant; where the dispatcher asks for a minimum amount of work (strips per round of 256
# blocks) the inputs are as large as that minimum, not larger.
CASE_LIST += [
    # 4-px strips: n8 < 70k
    _dw("ln<PX=4> CG=24 S=10", 96, 1, 20, 24, 1),
    _dw("ln<PX=4> CG=384 S=1", 1536, 1, 7, 11, 2),
    _dw("ln<PX=4> CG=48 S=5", 192, 1, 13, 10, 1),
    _dw("ln<PX=4> CG=48 S=5", 192, 3, 13, 10, 2),
    _dw("ln<PX=4> CG=64 S=4", 256, 1, 9, 11, 1),
    _dw("ln<PX=4> CG=64 S=4", 256, 1, 9, 11, 2),
    _dw("ln<PX=4> CG=64 S=4", 256, 2, 9, 11, 2),
    _dw("ln<PX=4> CG=96 S=2", 384, 1, 9, 16, 1),
    _dw("ln<PX=4> CG=96 S=2", 384, 2, 9, 16, 2),
    # 8-px strips: 70k <= n8 < 150k (13 strips x 77 rows x 3 x 24 = 72072; 13 x 87 x 64 = 72384; 13 x 45 x 2 x 64 = 74880)
    _dw("ln<PX=8> CG=24 S=10", 96, 3, 77, 101, 2),
    _dw("ln<PX=8> CG=64 S=4", 256, 1, 87, 101, 2),
    _dw("ln<PX=8> CG=64 S=4", 256, 2, 45, 101, 2),
    # 2 rows x 8 px without LDS weights: C = 384, one frame: n8 = 20 x 79 x 96 = 151680, 800 strips < 384 x 4
    _dw("ln2 CG=96 S=2", 384, 1, 79, 157, 2),
    # LDS-weight kernels: cdiv(strips, strips per block) >= 384
    _dw(_lnb(192, 2, 12, 1), 192, 3, 171, 163, 2),      # packed lanes: 6 groups x 86 x 3 = 1548 groups >= 384 x 4
    _dw(_lnb(192, 2, 8, 0), 192, 1, 159, 317, 2),       # one frame: 3200 strips >= 384 x 8, but 800 groups < 384 x 4 -> unpacked 8 waves
    _dw(_lnb(256, 2, 8, 0), 256, 3, 99, 163, 2),        # 1575 4-row strips < 3065 <= 3150 2-row strips
    _dw(_lnb(256, 4, 8, 0), 256, 6, 99, 163, 2),        # 3150 4-row strips
    _dw(_lnb(384, 2, 12, 1), 384, 3, 93, 163, 2),       # 11 groups x 47 x 3 = 1551 groups
    _dw(_lnb(768, 2, 12, 0), 768, 3, 49, 83, 2),        # 825 strips >= 384 x 2, more than the 256 of the row-split kernel
    # row-split one-frame kernel: C = 768, at most 256 strips
    _dw("lns<768>", 768, 1, 10, 10, 1),
    _dw("lns<768>", 768, 1, 10, 10, 2),
    _dw("lns<768>", 768, 2, 31, 45, 2),
]

_LN_C = {1: 192, 2: 384, 3: 768, 6: 1536}


def _ln_rows(ni, fmt, outF, outB):
    return _ln("rows", _LN_C[ni], fmt, bool(outF), bool(outB), M=333)


CASE_LIST += [_ln_rows(ni, fmt, f, b) for ni, fmt, f, b in (
    (1, 1, 0, 1), (1, 1, 1, 1), (1, 2, 0, 1), (1, 2, 1, 1), (2, 1, 0, 1), (2, 1, 1, 1), (2, 2, 0, 1), (2, 2, 1, 1), (3, 1, 0, 1), (3, 2, 0, 1), (3, 2, 1, 1),
    (6, 2, 0, 1))]
CASE_LIST += [_ln("pair", 256, 2, True, False, B=3, pair_hw=35)]

# GroupNorm apply: (act, fmt, batched, prior, outUp, outF, outB) as dispatched; one sample: M = 1000 rows, three samples: 611 = 47 x 13 rows each
CASE_LIST += [_gn(96, 16, act, 3 if bat else 1, 611 if (bat or up) else 1000, fmt, prior=bool(pr), up_w=13 if up else 0, outF=bool(f), outB=bool(b), ldu=128 if up else 0)
              for act, fmt, bat, pr, up, f, b in (
    (0, 1, 1, 0, 0, 1, 1), (0, 2, 1, 0, 0, 1, 1), (1, 1, 0, 0, 0, 0, 1), (1, 1, 0, 0, 0, 1, 0), (1, 2, 1, 0, 0, 0, 1), (1, 2, 1, 0, 0, 1, 0),
    (3, 1, 0, 0, 0, 0, 1), (3, 1, 0, 0, 0, 1, 0), (3, 1, 0, 0, 0, 1, 1), (3, 1, 0, 0, 1, 0, 1), (3, 1, 0, 1, 0, 1, 0),
    (3, 2, 0, 0, 0, 0, 1), (3, 2, 0, 0, 0, 1, 0), (3, 2, 0, 0, 0, 1, 1), (3, 2, 0, 0, 1, 0, 1), (3, 2, 0, 1, 0, 1, 0),
    (3, 2, 1, 0, 0, 1, 0), (3, 2, 1, 0, 0, 1, 1), (3, 2, 1, 1, 0, 1, 0))]

# ---------------------------------------------------------------------------------------------------------------- GEMM
# tag fields as uni_note_gemm (csrc/kernels.h) writes them.  The tag does not depend on how the variant was chosen, so the small shapes force
# the tile configuration (force_cfg) the heuristic takes at the census shapes.  Bound: |err| <= 1.2 (2^-20 sum |a||w| + 1e-6) as test_gemm_h2
# (operand-format output: + 2^-21 |reference|); the exact-fp32 kernel is held to the same fp32-equivalent bound.
B_GEMM = 2.0 ** -20
PLAIN = (300, 1, 128, 192, 1, 1, 0)      # (Hin, Win, Cin, N, k, stride, pad): 300 rows, K = 128
CONV3 = (20, 24, 64, 192, 3, 1, 1)       # 3x3 implicit GEMM, K = 576, ragged M = 480
PLAIN384, CONV384 = (300, 1, 128, 384, 1, 1, 0), (20, 24, 64, 384, 3, 1, 1)      # N = 2 x 192 for the 256 x 192 tile (cpg = 24)
HEAD5 = (13, 17, 256, 5, 1, 1, 0)        # reg / obj predictions: N = 5, ld 5 -> the direct (unstaged) epilogue
CTRL169 = (13, 17, 64, 169, 3, 1, 1)     # controller conv: N = 169 -> the direct epilogue of an implicit GEMM


def _gemm(fam, kernel, code, force, conv, stats, splitk, outF, outB, res, act, bias=True, geo=None, win=0):
    """win: the activation applies to the columns >= win only (the head's sigmoid window; uni_gemm_ex)"""
    fmt = "f32" if fam == "f32" else "h2"
    geo = geo or (CONV3 if conv else PLAIN)
    epi = fam != "f32" and geo[3] % 8 == 0
    # K ranges: the partial launch stores fp32 tiles only (bias / residual / sums belong to the reduce kernel), and is tagged so
    tag = "gemm:%s cfg=%d fmt=%s conv=%d stats=%d splitk=%d epi=%d outF=%d outB=%d res=%d act=%d%s remap=0 stacked=0" % (
        kernel, code, fmt, conv, stats and not splitk, splitk, epi, outF, outB, res and not splitk, act, "w" if win else "")
    return dict(tag=tag, entry="uni_gemm_ex" if fam == "f32" or win else "uni_gemm_h2",
                args=dict(fam=fam, geo=geo, act=act, act_col0=win, bias=bias and not stats, res=bool(res), G=16 if stats else 0, outF=bool(outF), outB=bool(outB),
                          cfg=force + (2000000 if splitk else 0)),
                ref="torch fp64: F.conv2d of the unrounded fp32 operands + activation + residual", bound=B_GEMM, bound_from="test_gemm_h2")


def _reduce(bias, res, stats, conv):
    c = _gemm("h2", "h2d", 22113, 331, conv, stats, 1, 1, 0, res, 0, bias=bool(bias))
    c["tag"] = "gemm:splitk_reduce bias=%d res=%d stats=%d stacked=0" % (bias, res, stats)
    return c


CASE_LIST += [_gemm("f32", "f32", 2211, 0, *t) for t in (
    # (conv, stats, splitk, outF, outB, res, act)
    (0, 0, 0, 0, 1, 0, 1), (0, 0, 0, 0, 1, 0, 2), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 1, 0), (0, 0, 0, 1, 1, 1, 0), (0, 1, 0, 1, 0, 0, 0),
    (1, 0, 0, 0, 1, 0, 1), (1, 0, 0, 1, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0))]
CASE_LIST += [_gemm("h2", "h2", 2222, 22, *t) for t in ((0, 0, 0, 0, 1, 0, 1), (0, 0, 0, 0, 1, 0, 2), (1, 1, 0, 1, 0, 0, 0))]
CASE_LIST += [_gemm("h2", "h2d", 22113, 331, *t) for t in (      # 64 x 64, 3-deep ring
    (0, 0, 0, 0, 1, 0, 2), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 1, 0), (0, 0, 0, 1, 1, 1, 0), (0, 0, 1, 1, 0, 1, 0), (0, 1, 0, 1, 0, 0, 0),
    (1, 0, 0, 1, 0, 0, 0), (1, 0, 1, 1, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0))]
CASE_LIST += [_gemm("h2", "h2d", 22123, 332, *t) for t in (      # 64 x 128
    (0, 0, 0, 0, 1, 0, 1), (0, 0, 0, 0, 1, 0, 2), (0, 0, 0, 1, 0, 1, 0), (0, 0, 0, 1, 1, 1, 0), (0, 1, 0, 1, 0, 0, 0),
    (1, 0, 0, 0, 1, 0, 1), (1, 0, 0, 1, 0, 0, 0), (1, 1, 0, 1, 0, 0, 0))]
CASE_LIST += [_gemm("h2", "h2d", 41134, 323, 0, 0, 0, 1, 0, 1, 0)]      # 128 x 96, 4-deep
CASE_LIST += [_gemm("h2", "h2d", 42232, 346, *t) for t in ((0, 0, 0, 0, 1, 0, 2), (0, 0, 0, 1, 0, 0, 0), (0, 0, 0, 1, 0, 1, 0))]      # 256 x 192
CASE_LIST += [_gemm("h2", "h2q_outB", 188, 188, 0, 0, 0, 0, 1, 0, 1), _gemm("h2", "h2q_outB", 188, 188, 0, 0, 0, 0, 1, 0, 2),
              _gemm("h2", "h2q_outF", 188, 188, 0, 0, 0, 1, 0, 0, 0), _gemm("h2", "h2q_outF", 188, 188, 0, 0, 0, 1, 0, 1, 0)]
CASE_LIST += [_reduce(0, 0, 1, 1), _reduce(1, 1, 0, 0)]
# What the 16-frame step and the head's remapped outputs run on (their tags carry stacked=1 / remap=1 and sit in CTX_ONLY; the closure asks
# for the same tag with both switches at 0, i.e. the same template instantiation on one sample): the ping-pong kernel as an implicit GEMM and
# with GroupNorm sums, the 256 x 192 tile with sums / as a conv, the direct-epilogue tiles of the N = 5 / 6 / 169 head layers with the
# sigmoid on every column and on a column window.
CASE_LIST += [
    _gemm("h2", "h2q_outB", 188, 188, 1, 0, 0, 0, 1, 0, 1), _gemm("h2", "h2q_outF", 188, 188, 0, 1, 0, 1, 0, 0, 0),
    _gemm("h2", "h2q_outF", 188, 188, 1, 0, 0, 1, 0, 0, 0), _gemm("h2", "h2q_outF", 188, 188, 1, 1, 0, 1, 0, 0, 0),
    _gemm("h2", "h2d", 42232, 346, 0, 1, 0, 1, 0, 0, 0, geo=PLAIN384), _gemm("h2", "h2d", 42232, 346, 1, 0, 0, 1, 0, 0, 0, geo=CONV384),
    _gemm("h2", "h2d", 42232, 346, 1, 1, 0, 1, 0, 0, 0, geo=CONV384),
    _gemm("h2", "h2d", 22113, 331, 1, 0, 0, 0, 1, 0, 1), _gemm("h2", "h2", 2222, 22, 1, 0, 0, 1, 0, 0, 0),
    _gemm("h2", "h2", 2211, 11, 1, 0, 0, 1, 0, 0, 0, geo=CTRL169),
    _gemm("h2", "h2", 2211, 11, 0, 0, 0, 1, 0, 0, 4, geo=HEAD5), _gemm("h2", "h2", 2211, 11, 0, 0, 0, 1, 0, 0, 4, geo=HEAD5, win=4),
    _gemm("h2", "h2", 2221, 21, 0, 0, 0, 1, 0, 0, 4, geo=HEAD5), _gemm("h2", "h2", 2221, 21, 0, 0, 0, 1, 0, 0, 4, geo=HEAD5, win=4),
    _gemm("f32", "f32", 2211, 0, 0, 0, 0, 1, 0, 0, 4, geo=HEAD5), _gemm("f32", "f32", 2211, 0, 0, 0, 0, 1, 0, 0, 4, geo=HEAD5, win=4),
]
# deep tile 322 (128 x 128, 4-deep ring): the heuristic keeps it for long-K plain GEMMs with 193 .. 256 tiles, which no census workload has
CASE_LIST += [_gemm("h2", "h2d", 22224, 322, 0, 0, 0, 1, 0, 0, 0)]


# ---------------------------------------------------------------------------------------------------------------- the rest
def _simple(tag, entry, args, ref, bound, bound_from):
    return dict(tag=tag, entry=entry, args=args, ref=ref, bound=bound, bound_from=bound_from)


B_CORR = 2e-5       # absolute, test_corr_softmax_pv
_CORR_REF = "torch fp64: values @ softmax(e_ref^T e_cur, dim = reference axis)"
CASE_LIST += [
    # pick_nsplit (csrc/corr.hip): R = 2048 allows 8 splits and 2 query blocks per frame leave the GPU empty -> split + merge; R = 300 < 512: one split
    _simple("corr f32 KV=1 split batched=0 vpf=0 lse=0", "uni_corr_softmax_pv", dict(B=0, R=2048, Q=130, K=1, prec=0), _CORR_REF, B_CORR, "test_corr_softmax_pv"),
    _simple("corr h2 KV=1 split batched=0 vpf=0 lse=0", "uni_corr_softmax_pv", dict(B=0, R=2048, Q=130, K=1, prec=2), _CORR_REF, B_CORR, "test_corr_softmax_pv"),
    _simple("corr merge KV=1 batched=0 lse=0", "uni_corr_softmax_pv", dict(B=0, R=2048, Q=131, K=1, prec=2), _CORR_REF, B_CORR, "test_corr_softmax_pv"),
    _simple("corr h2 KV=1 single batched=1 vpf=0 lse=0", "uni_corr_softmax_pv_batched", dict(B=2, R=300, Q=500, K=1, prec=2), _CORR_REF, B_CORR, "test_corr_softmax_pv_batched"),
    _simple("corr h2 KV=1 split batched=1 vpf=0 lse=0", "uni_corr_softmax_pv_batched", dict(B=2, R=2048, Q=130, K=1, prec=2), _CORR_REF, B_CORR, "test_corr_softmax_pv_batched"),
    _simple("corr merge KV=1 batched=1 lse=0", "uni_corr_softmax_pv_batched", dict(B=2, R=2048, Q=131, K=1, prec=2), _CORR_REF, B_CORR, "test_corr_softmax_pv_batched"),
    _simple("cast_operand fmt=h2", "uni_cast_h2", dict(M=257, C=64, fmt=2), "the fp64 value of the fp32 input", 2.0 ** -21, "test_h2_cast_and_pack_formats"),
    _simple("cast_operand fmt=f32", "uni_cast_f32", dict(M=257, C=64, fmt=1), "the fp64 value of the fp32 input (exact copy)", 2.0 ** -21, "test_h2_cast_and_pack_formats"),
    _simple("stem 4px CG=24 S=10 batched=0", "uni_stem_ex", dict(C=96, B=1, H=16, W=32), "oracle fp64: F.conv2d(stride 4) + ln_channels_first", 2e-4, "test_stem"),
    _simple("stem 4px CG=24 S=10 batched=1", "uni_stem_ex", dict(C=96, B=2, H=16, W=32), "oracle fp64: F.conv2d(stride 4) + ln_channels_first", 2e-4, "test_stem"),
    _simple("stem 4px CG=48 S=5 batched=0", "uni_stem_ex", dict(C=192, B=1, H=16, W=32), "oracle fp64: F.conv2d(stride 4) + ln_channels_first", 2e-4, "test_stem"),
    _simple("stem 1px CG=24 S=10 batched=0", "uni_stem_ex", dict(C=96, B=1, H=16, W=20), "oracle fp64: F.conv2d(stride 4) + ln_channels_first", 2e-4, "test_stem"),      # W % 16 != 0 (not dispatched: every census width is a multiple of 16)
    _simple("stem 4px CG=48 S=5 batched=1", "uni_stem_ex", dict(C=192, B=2, H=16, W=32), "oracle fp64: F.conv2d(stride 4) + ln_channels_first", 2e-4, "test_stem"),
    _simple("mlp_fused layout=0 C=96 outB=0 dbg=0", "uni_mlp_fused", dict(C=96, M=300, layout=0, outB=False), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("mlp_fused layout=1 C=192 outB=0 dbg=0", "uni_mlp_fused", dict(C=192, M=300, layout=1, outB=False), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("mlp_fused layout=1 C=256 outB=0 dbg=0", "uni_mlp_fused", dict(C=256, M=300, layout=1, outB=False), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("mlp_fused layout=1 C=256 outB=1 dbg=0", "uni_mlp_fused", dict(C=256, M=300, layout=1, outB=True), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("msda_fused fmt=f32 batched=0", "uni_msda_tokens", dict(B=1, h=7, w=5), "oracle fp64: msda_core on softmax weights and ref + off / (W, H)", 2e-5, "test_msda_wave_kernel_tokens"),
    _simple("prior_pyramid", "uni_prior_pyramid", dict(K=3, H8=44, W8=76), "oracle fp64: prior_pyramid", 1e-6, "test_prior_pyramid_label_map"),
    _simple("decode batched=0", "uni_decode_outputs", dict(B=1, H=320, W=352, nch=6), "oracle fp64: decode_outputs", 1e-5, "test_decode_outputs_device"),
    _simple("decode batched=1", "uni_decode_outputs", dict(B=2, H=320, W=352, nch=6), "oracle fp64: decode_outputs", 1e-5, "test_decode_outputs_device"),
    _simple("condinst final=1", "uni_condinst_masks", dict(n=5, H8=20, W8=28), "oracle fp64: aligned_bilinear(dynamic_mask_head)", 2e-5, "test_condinst_masks"),
]

# ---------------------------------------------------------------------------------------------------------------- not dispatched by the census
# Builds no census workload reaches (listed under not_dispatched in variant_census.json): the unpacked 12-wave C = 384 build needs a map with
# enough strips but too few strip groups, and no model configuration has C = 512.
CASE_LIST += [
    # n8 = 21 x 93 x 2 x 96 = 374976; 21 x 47 x 2 = 1974 strips, cdiv(1974, 4) = 494 >= 384; 11 x 47 x 2 = 1034 groups, cdiv(1034, 4) = 259 < 384 -> not packed
    _dw(_lnb(384, 2, 12, 0), 384, 2, 93, 163, 2),
    _dw(_lnb(512, 4, 8, 0), 512, 3, 99, 163, 2),        # C = 512: 1575 4-row strips >= 384 x 4
    _dw(_lnb(512, 2, 8, 0), 512, 2, 99, 163, 2),        # 1050 4-row strips < 1533 <= 2100 2-row strips
]

CASES = {c["tag"]: c for c in CASE_LIST}

# ---------------------------------------------------------------------------------------------------------------- context-only tags
# Launchers that keep NO context-free entry point; nothing else may be parked here (tests/test_variant_cases_cpu.py).
CTX_ONLY_ALLOWED = ("cast_operand_pair", "pixel_shuffle_bf16", "add_pos_bf16", "add_aligned_bilinear", "pos_embed", "gemm:", "msda_fused")
CTX_ONLY = [
    # (tag pattern, reason, model-level test that runs it)
    (r"^cast_operand_pair ", "token layout [B][2][hw] of the interaction stage, built from context buffers", "test_batched_frames_equal_single_frame_runs"),
    (r"^pixel_shuffle_bf16 ", "upsample-stage scatter between context buffers", "test_batched_frames_equal_single_frame_runs"),
    (r"^add_pos_bf16 ", "position + level embedding add of the interaction stage", "test_batched_frames_equal_single_frame_runs"),
    (r"^add_aligned_bilinear ", "FPN top-down / mask-branch upsample-add between context buffers", "test_batched_frames_equal_single_frame_runs"),
    (r"^pos_embed$", "learned position embedding table lives in the context", "test_tiny_320_vs_reference_golden"),
    (r"^gemm:.* remap=1 stacked=[01]$", "outF row remap of the head outputs (out_hw) is set by the engine only", "test_batched_frames_equal_single_frame_runs"),
    (r"^gemm:.* remap=[01] stacked=1$", "stacked samples (M != Mper): per-sample statistics slots and conv halos", "test_batched_frames_equal_single_frame_runs"),
    (r"^gemm:splitk_reduce .* stacked=1$", "stacked samples (M != Mper) in the split-K reduce", "test_batched_frames_equal_single_frame_runs"),
    (r"^msda_fused fmt=(bf16|h2) ", "operand-format output of the fused sampler (uni_msda_tokens is fp32 only)", "test_batched_frames_equal_single_frame_runs"),
]


def gemm_twin(tag):
    """a context-only GEMM / split-K reduce tag with the row-remap and stacked-sample switches at 0: the same template instantiation on one
    sample, which must have a case of its own (only the per-sample arithmetic needs a context)"""
    return re.sub(r"\bremap=1\b", "remap=0", re.sub(r"\bstacked=1\b", "stacked=0", tag))


def ctx_only_match(tag):
    for pat, reason, test in CTX_ONLY:
        if re.search(pat, tag):
            return pat
    return None
