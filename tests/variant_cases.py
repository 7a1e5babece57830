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
# What the 16-frame step and the head's remapped outputs run on, on one sample and without the remap (the stacked=1 / remap=1 tags have
# their own cases further down, on uni_gemm_stacked): the ping-pong kernel as an implicit GEMM and
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


# ---------------------------------------------------------------------------------------------------------------- GEMM: stacked samples, row remap
# uni_gemm_stacked sets the two switches the engine sets on a batch: B samples per launch (Mper != M: 3x3 halos stop at every sample's own
# border, GroupNorm sums of sample b at stats + 64 b) and the outF row remap of the head outputs.  Two maps, the smallest that make tiles
# straddle samples: (13, 17) x 3 -- Mper = 221, M = 663: every 64- / 128- / 256-row tile boundary falls inside a sample, the first 256-row
# tile holds parts of two samples, the last tile is ragged -- and (7, 9) x 5 -- Mper = 63, M = 315: one 256-row tile holds more than four
# samples (the b_lo .. b_hi loop of gemm_stats runs five times), a 64-row tile has a sample boundary at row 63.  Cin / N as the one-sample
# geometries above.  Sample b is drawn as x_b (1 + b) + 0.5 b, so a row attributed to the wrong sample moves a sum by far more than the
# tolerance (tests/test_variant_cases_cpu.py shows it for every case, without a GPU).
MAP_A, MAP_B = (13, 17, 3), (7, 9, 5)       # (Hin, Win, B)
REMAP = dict(out_stride=300, out_off=40)    # anchors per image / first anchor row of the level; out_hw = the level's rows per image (221)
STATS_RTOL, STATS_ATOL = 2e-5, 2e-2         # test_gemm_h2


def _gemms(fam, kernel, code, force, conv, stats, splitk, outF, outB, res, act, base, hwb, remap=0, win=0, bias=True, reduce_tag=False):
    """a uni_gemm_stacked case: `base` gives Cin / N / k / stride / pad, hwb = (Hin, Win, B) the map and the number of samples"""
    Hin, Win, B = hwb
    geo = (Hin, Win) + tuple(base[2:])
    N = geo[3]
    ldf = N if N == 169 else N + (4 if N % 4 == 0 else 3)      # the controller output keeps the engine's odd ld = 169; everything else has columns behind N
    epi = fam != "f32" and N % 8 == 0
    if reduce_tag:
        tag = "gemm:splitk_reduce bias=%d res=%d stats=%d stacked=%d" % (bias, res, stats, B > 1)
    else:
        tag = "gemm:%s cfg=%d fmt=%s conv=%d stats=%d splitk=%d epi=%d outF=%d outB=%d res=%d act=%d%s remap=%d stacked=%d" % (
            kernel, code, "f32" if fam == "f32" else "h2", conv, stats and not splitk, splitk, epi, outF, outB, res and not splitk, act, "w" if win else "",
            bool(remap) and not splitk, B > 1)
    args = dict(fam=fam, geo=geo, B=B, act=act, act_col0=win, bias=bool(bias), res=bool(res), G=16 if stats else 0, outF=bool(outF), outB=bool(outB), cfg=force,
                splitk=2 if splitk else 0, ldf=ldf, out_hw=0, out_stride=0, out_off=0, outF_rows=0)
    M = B * ((Hin + 2 * geo[6] - geo[4]) // geo[5] + 1) * ((Win + 2 * geo[6] - geo[4]) // geo[5] + 1)
    if remap:      # remap = images per launch: the rows of image i go to i * out_stride + out_off, 3 more rows behind the last one
        args.update(REMAP, out_hw=M // remap)
        args["outF_rows"] = (remap - 1) * REMAP["out_stride"] + REMAP["out_off"] + M // remap + 3
    elif outF:
        args["outF_rows"] = M + 1
    return dict(tag=tag, entry="uni_gemm_stacked", args=args,
                ref="torch fp64: F.conv2d of the (B, Cin, Hin, Win) batch of the unrounded fp32 operands (every sample padded on its own) + activation + residual; "
                    "per-sample fp64 group sums", bound=B_GEMM, bound_from="test_gemm_h2")


# (conv, stats, splitk, outF, outB, res, act) as above.  Every family as an implicit GEMM, with GroupNorm sums and with both; the map of a
# case is the one whose boundary pattern its tile height has not had yet in that family
def _family(fam, kernel, code, force, plain, conv3, m_conv, m_stats, m_both):
    return [_gemms(fam, kernel, code, force, 1, 0, 0, 1, 0, 0, 0, conv3, m_conv), _gemms(fam, kernel, code, force, 0, 1, 0, 1, 0, 0, 0, plain, m_stats),
            _gemms(fam, kernel, code, force, 1, 1, 0, 1, 0, 0, 0, conv3, m_both)]


STACKED = []
STACKED += _family("f32", "f32", 2211, 0, PLAIN, CONV3, MAP_A, MAP_B, MAP_A)
STACKED += _family("h2", "h2", 2222, 22, PLAIN, CONV3, MAP_A, MAP_B, MAP_B)
STACKED += _family("h2", "h2", 2211, 11, PLAIN, CONV3, MAP_B, MAP_A, MAP_B)
STACKED += _family("h2", "h2d", 22113, 331, PLAIN, CONV3, MAP_A, MAP_A, MAP_B)
STACKED += _family("h2", "h2d", 22123, 332, PLAIN, CONV3, MAP_B, MAP_B, MAP_A)
STACKED += _family("h2", "h2d", 42232, 346, PLAIN384, CONV384, MAP_A, MAP_A, MAP_B)
STACKED += _family("h2", "h2q_outF", 188, 188, PLAIN, CONV3, MAP_A, MAP_A, MAP_B)
STACKED += [_gemms("h2", "h2q_outB", 188, 188, 1, 0, 0, 0, 1, 0, 1, CONV3, MAP_B)]
# K ranges: the partial launch (64 x 64 deep tile, as the one-sample cases) and the reduce kernel, whose grid is (cdiv(Mper, 8), B): 221 and 63 are
# no multiples of 8, so the last block of every sample is ragged
STACKED += [_gemms("h2", "h2d", 22113, 331, 0, 0, 1, 1, 0, 1, 0, PLAIN, MAP_A), _gemms("h2", "h2d", 22113, 331, 1, 1, 1, 1, 0, 0, 0, CONV3, MAP_B, bias=False),
            _gemms("h2", "h2d", 22113, 331, 0, 0, 1, 1, 0, 1, 0, PLAIN, MAP_B, reduce_tag=True),
            _gemms("h2", "h2d", 22113, 331, 1, 1, 1, 1, 0, 0, 0, CONV3, MAP_A, bias=False, reduce_tag=True)]
# the head's remapped outputs: reg / obj predictions (N = 5, sigmoid on every column and on the columns >= 4), one launch over the 3 x 221 rows
# of three images as the engine launches it (a 1x1 convolution over [B * hw] rows: remap=1 stacked=0), and the controller conv (3x3, N = 169,
# ld 169, three stacked samples: remap=1 stacked=1), on the direct-epilogue tiles and the exact-fp32 kernel
HEAD5_ROWS = (663, 1, 1)
for _fam, _kernel, _code, _force in (("h2", "h2", 2211, 11), ("h2", "h2", 2221, 21), ("f32", "f32", 2211, 0)):
    STACKED += [_gemms(_fam, _kernel, _code, _force, 0, 0, 0, 1, 0, 0, 4, HEAD5, HEAD5_ROWS, remap=3),
                _gemms(_fam, _kernel, _code, _force, 0, 0, 0, 1, 0, 0, 4, HEAD5, HEAD5_ROWS, remap=3, win=4),
                _gemms(_fam, _kernel, _code, _force, 1, 0, 0, 1, 0, 0, 0, CTRL169, MAP_A, remap=3)]
# dispatched by the census and not among the above: the one-frame controller conv of the fp32 model (remap=1 on one sample: out_hw = Mper, the
# level's rows land at out_off), and the 64 x 64 deep tile as a conv + ReLU into operand rows on stacked samples
STACKED += [_gemms("f32", "f32", 2211, 0, 1, 0, 0, 1, 0, 0, 0, CTRL169, (13, 17, 1), remap=1),
            _gemms("h2", "h2d", 22113, 331, 1, 0, 0, 0, 1, 0, 1, CONV3, MAP_A)]
CASE_LIST += STACKED


def gemm_stacked_problem(a, bound=B_GEMM):
    """Inputs, fp64 reference and tolerances of a uni_gemm_stacked case, on the CPU (shared by the GPU runner and the CPU self-check of the
    cases).  raw = conv + bias as (M, N) rows, finish(raw) = activation window + residual, stats(raw, shift) = per-sample group sums of the
    rows [b Mper + shift, (b + 1) Mper + shift), orow = the outF row of every output row."""
    import torch
    import torch.nn.functional as F
    acts = {0: lambda t: t, 1: F.relu, 2: F.gelu, 3: F.silu, 4: torch.sigmoid}
    Hin, Win, Cin, N, k, stride, pad = a["geo"]
    B, act, G, c0 = a["B"], a["act"], a["G"], a["act_col0"]
    g = torch.Generator().manual_seed(Hin * 7 + N + a["cfg"] + act + 31 * B + c0)
    sb = torch.arange(B).float().reshape(B, 1, 1, 1)
    x = torch.randn(B, Cin, Hin, Win, generator=g) * 3.0 * (1.0 + sb) + 0.5 * sb
    w = torch.randn(N, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    bias = torch.randn(N, generator=g) * 0.1 if a["bias"] else None
    bd = bias.double() if a["bias"] else None

    def rows(t):
        return t.permute(0, 2, 3, 1).reshape(-1, N)

    raw = rows(F.conv2d(x.double(), w.double(), bd, stride=stride, padding=pad))
    mag = rows(F.conv2d(x.abs().double(), w.abs().double(), None, stride=stride, padding=pad))
    M = raw.shape[0]
    Mper = M // B
    res = torch.randn(M, N + 4, generator=g) if a["res"] else None

    def finish(r):
        return torch.cat([r[:, :c0], acts[act](r[:, c0:])], 1) + (res[:, :N].double() if a["res"] else 0)

    def stats(r, shift=0):
        out = torch.zeros(B, G, 2, dtype=torch.float64)
        for b in range(B):
            grp = r[b * Mper + shift:(b + 1) * Mper + shift].reshape(-1, G, N // G)
            out[b, :, 0], out[b, :, 1] = grp.sum((0, 2)), (grp ** 2).sum((0, 2))
        return out

    m = torch.arange(M)
    orow = (m // a["out_hw"]) * a["out_stride"] + a["out_off"] + m % a["out_hw"] if a["out_hw"] else m
    P = dict(x=x, w=w, bias=bias, res=res, raw=raw, exp=finish(raw), tol=(mag * bound + 1e-6) * 1.2, M=M, Mper=Mper, orow=orow, finish=finish, stats=stats, rows=rows)
    if G:
        P["stats_ref"] = stats(raw)
        P["stats_tol"] = STATS_ATOL + STATS_RTOL * P["stats_ref"].abs()
    return P


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
    _simple("mlp_fused layout=0 C=96 outB=0", "uni_mlp_fused", dict(C=96, M=300, layout=0, outB=False), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("mlp_fused layout=1 C=192 outB=0", "uni_mlp_fused", dict(C=192, M=300, layout=1, outB=False), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("mlp_fused layout=1 C=256 outB=0", "uni_mlp_fused", dict(C=256, M=300, layout=1, outB=False), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("mlp_fused layout=1 C=256 outB=1", "uni_mlp_fused", dict(C=256, M=300, layout=1, outB=True), "torch fp64 on the f16x2-decoded operand", 4e-6, "test_mlp_fused"),
    _simple("msda_fused fmt=f32 batched=0", "uni_msda_tokens", dict(B=1, h=7, w=5), "oracle fp64: msda_core on softmax weights and ref + off / (W, H)", 2e-5, "test_msda_wave_kernel_tokens"),
    _simple("prior_pyramid", "uni_prior_pyramid", dict(K=3, H8=44, W8=76), "oracle fp64: prior_pyramid", 1e-6, "test_prior_pyramid_label_map"),
    _simple("decode batched=0", "uni_decode_outputs", dict(B=1, H=320, W=352, nch=6), "oracle fp64: decode_outputs", 1e-5, "test_decode_outputs_device"),
    _simple("decode batched=1", "uni_decode_outputs", dict(B=2, H=320, W=352, nch=6), "oracle fp64: decode_outputs", 1e-5, "test_decode_outputs_device"),
    _simple("condinst final=1", "uni_condinst_masks", dict(n=5, H8=20, W8=28), "oracle fp64: aligned_bilinear(dynamic_mask_head)", 2e-5, "test_condinst_masks"),
]

# ---------------------------------------------------------------------------------------------------------------- glue launchers between context buffers
# the `_ex` entries of the launchers the engine runs between its own buffers: one case per census tag, one (7, 5) map or three stacked ones
# (every sample / frame drawn on its own scale), C as the stage that runs them: 256 interaction tokens, 128 -> 32 PixelShuffle channels.
# Operand rows: the restated row bound of the format, fp32 rows exact (run_cast).  fp32 results of fp32 arithmetic (add_aligned_bilinear,
# pos_embed): 4 x the distance of the oracle's own fp32 evaluation from its fp64 one, computed by the runner; `bound` is the cap on that.
def _glue(tag, entry, ref, fmt=1, bound=B_H2_ROWS, bound_from="test_dwconv7_ln_batched_all_formats", **args):
    return dict(tag=tag, entry=entry, args=dict(fmt=fmt, h=7, w=5, **args), ref=ref, bound=bound, bound_from=bound_from)


for _fmt, _B in ((1, 1), (2, 1), (2, 3)):
    _t = "fmt=%s batched=%d" % (("bf16", "f32", "h2")[_fmt], _B > 1)
    CASE_LIST += [
        _glue("cast_operand_pair " + _t, "uni_cast_operand_pair_ex", "the fp64 value of the fp32 inputs, laid out [B][2][hw][C]", _fmt, B=_B, C=256),
        _glue("pixel_shuffle_bf16 " + _t, "uni_pixel_shuffle_ex", "torch fp64: F.pixel_shuffle(., 2) of the (B, C, h, w) map", _fmt, B=_B, C=128),
        _glue("add_pos_bf16 " + _t, "uni_add_pos_ex", "torch fp64: src + pos + lvl per frame of the pair", _fmt, B=_B, C=256)]
    if _fmt == 2:      # (fmt=f32 batched=0 is uni_msda_tokens, above)
        CASE_LIST += [_glue("msda_fused " + _t, "uni_msda_tokens_ex", "oracle fp64: msda_core on softmax weights and ref + off / (W, H)", _fmt, B=_B)]
CASE_LIST += [_glue("add_aligned_bilinear factor=%d batched=%d" % (_f, _B > 1), "uni_add_aligned_bilinear_ex", "oracle fp64: dst + aligned_bilinear(src, factor) per sample",
                    bound=1e-5, bound_from="test_decode_outputs_device", B=_B, C=32, factor=_f) for _f in (2, 4) for _B in (1, 3)]
CASE_LIST += [_glue("pos_embed", "uni_pos_embed_ex", "oracle fp64: pos_embed (bilinear resize of the [col | row] table grid)", bound=1e-5,
                    bound_from="test_decode_outputs_device", sz=40, nf=128)]

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
# Launchers that keep NO context-free entry point; nothing else may be parked here (tests/test_variant_cases_cpu.py).  Every launcher the
# census dispatches has one now: the lists stay for the next launcher that is written against context buffers only.
CTX_ONLY_ALLOWED = ()
CTX_ONLY = [
    # (tag pattern, reason, model-level test that runs it)
]

def gemm_twin(tag):
    """a GEMM / split-K reduce tag with the row-remap and stacked-sample switches at 0: the same template instantiation on one sample.  The
    census closure asks for it for every GEMM tag parked in CTX_ONLY; none may be parked there any more (uni_gemm_stacked sets both switches)"""
    return re.sub(r"\bremap=1\b", "remap=0", re.sub(r"\bstacked=1\b", "stacked=0", tag))


def ctx_only_match(tag):
    for pat, reason, test in CTX_ONLY:
        if re.search(pat, tag):
            return pat
    return None
