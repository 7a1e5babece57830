"""The epilogue of the ping-pong f16x2 GEMM (csrc/gemm_h2q.hip, cfg 188) on its own: K = 64 is two K steps, the kernel's minimum, so a
launch is almost nothing but bias / activation / residual / the fp32 and operand-format stores.

Reference: float64 on the SAME split operands the kernel multiplies -- the rows uni_cast_h2 wrote, decoded hi + lo, and the host split of
the scaled weights restated here -- so what is left is the dropped lo.lo term and the fp32 accumulation.  Bounds as tests/test_kernels_gpu.py
holds the same quantities to: |err| <= 1.2 (2^-20 sum |a||w| + 1e-6) for fp32 rows, + 2^-21 |reference| for decoded operand rows
(test_gemm_h2_persistent), group sums rtol 2e-5 / atol 2e-2 (test_gemm_h2).

Exact: the operand rows of an operand-only launch equal those of the fp32 + operand launch byte for byte, and both equal the split of the
fp32 rows restated in numpy (clamp to +-65504, hi = float16(v), lo = float16(v - float32(hi))).

Two cases differ from the sizes first asked for, because the launcher refuses those: K ranges need two K steps each, so the split-K case has
K = 128; the statistics epilogue needs 256 / cpg + 2 <= 64, so the 64-channel conv has 8 groups, not 16."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_kernels_gpu import ACTS, cast_h2, h2_decode, pack_weight_h2

pytestmark = pytest.mark.gpu

K = 64
SHAPES = [
    (256, 256),        # one interior tile
    (257, 264),        # one spare row; a last N tile of 8 columns (N no multiple of 64): the clamped bias loads
    (511, 320),        # interior and edge tiles
    (4352, 4096),      # 272 tiles, more than CUs: a second tile follows an epilogue in the same block
]
OUTPUTS = ("B", "F", "F+res", "F+B")


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def split_weight_ref(w, wscale):
    """the value the packed weight stands for, in float64: the f16x2 split of w / wscale (a power of two), times wscale"""
    ws = (w.float() * (1.0 / wscale)).clamp(-65504.0, 65504.0)
    hi = ws.half()
    lo = (ws - hi.float()).half()
    return (hi.double() + lo.double()) * wscale


def split_rows_np(v):
    """fp32 rows (M, N) -> the operand rows act_store* write, as uint16 (M, N / 8, 2, 8)"""
    c = np.clip(v.astype(np.float32), np.float32(-65504.0), np.float32(65504.0))
    hi = c.astype(np.float16)
    lo = (c - hi.astype(np.float32)).astype(np.float16)
    M, N = v.shape
    return np.stack([hi.reshape(M, N // 8, 8), lo.reshape(M, N // 8, 8)], 2).view(np.uint16)


def rows_u16(outB, M, N):
    return outB.cpu().numpy().view(np.uint16).reshape(M, N // 8, 2, 8)


PAD = 8          # columns behind N in every output / residual row (ld = N + PAD), and one row behind M: the guard band
FILL_B = -1      # what the guard band of the operand rows holds (int32 storage)


def problem(L, M, N, Kk, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(M, Kk, generator=g) * 2.0).cuda()
    w = torch.randn(N, Kk, generator=g) / Kk ** 0.5
    bias = (torch.randn(N, generator=g) * 0.1).cuda()
    res = torch.randn(M, N + PAD, generator=g).cuda()
    A = cast_h2(L, x)
    Wp, wscale = pack_weight_h2(L, w.reshape(N, Kk, 1, 1))
    xs = h2_decode(A, M, Kk)[0].double()
    wsd = split_weight_ref(w, wscale).cuda()
    raw = xs @ wsd.t()
    mag = xs.abs() @ wsd.abs().t()
    return dict(A=A, Wp=Wp, wscale=wscale, bias=bias, res=res, raw=raw, tol=(mag * 2.0 ** -20 + 1e-6) * 1.2)


def launch(L, P, M, N, Kk, act, use_bias, out, cfg=188):
    """-> (outF, outB) as (M, N) views of buffers with M + 1 rows of N + PAD columns; the row behind M and the columns behind N must come
    back untouched (the kernel leaves rows past M and columns past N to the bounds of its buffer descriptors)"""
    ld = N + PAD
    bufF = torch.full((M + 1, ld), float("nan"), device="cuda") if "F" in out else None
    bufB = torch.full((M + 1, ld), FILL_B, device="cuda", dtype=torch.int32) if "B" in out else None
    res = P["res"] if "res" in out else None
    L.check(L.lib().uni_gemm_h2(L.ptr(P["A"]), Kk, L.ptr(P["Wp"]), P["wscale"], M, N, M, 1, Kk, 1, 1, 1, 0, L.ptr(P["bias"] if use_bias else None), act,
                                L.ptr(res), ld, L.ptr(bufF), ld, L.ptr(bufB), ld, None, 0, cfg, L.stream_ptr()), "gemm_h2")
    torch.cuda.synchronize()
    if bufF is not None:
        assert torch.isnan(bufF[M]).all() and torch.isnan(bufF[:M, N:]).all(), (M, N, act, use_bias, out, "fp32 guard band written")
    if bufB is not None:
        assert (bufB[M] == FILL_B).all() and (bufB[:M, N:] == FILL_B).all(), (M, N, act, use_bias, out, "operand guard band written")
    return (bufF[:M, :N].contiguous() if bufF is not None else None), (bufB[:M, :N].contiguous() if bufB is not None else None)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_h2q_epilogue(L, shape):
    """act none / ReLU / GELU x bias on / off x the four output sets, one reference per shape"""
    M, N = shape
    P = problem(L, M, N, K, M * 3 + N)
    for act in (0, 1, 2):
        for use_bias in (True, False):
            pre = ACTS[act](P["raw"] + (P["bias"].double() if use_bias else 0))
            got = {}
            for out in OUTPUTS:
                exp = pre + (P["res"][:, :N].double() if "res" in out else 0)
                outF, outB = launch(L, P, M, N, K, act, use_bias, out)
                tag = (shape, act, use_bias, out)
                if outF is not None:
                    assert torch.isfinite(outF).all(), tag
                    err = (outF.double() - exp).abs()
                    assert (err <= P["tol"]).all(), (tag, (err / P["tol"]).max().item())
                if outB is not None:
                    dec = h2_decode(outB, M, N)[0].double()
                    err = (dec - exp).abs()
                    assert (err <= P["tol"] + exp.abs() * 2.0 ** -21).all(), (tag, (err / P["tol"]).max().item())
                got[out] = (outF, outB)
            # exact: operand rows alone == operand rows next to the fp32 rows == the split of the fp32 rows
            assert torch.equal(got["B"][1], got["F+B"][1]), (shape, act, use_bias)
            want = split_rows_np(got["F+B"][0].cpu().numpy())
            assert np.array_equal(rows_u16(got["F+B"][1], M, N), want), (shape, act, use_bias)


def test_h2q_epilogue_splitk(L):
    """two K ranges of two K steps as work units of the persistent kernel: every range stores its fp32 partial tile into its slab, the
    reduce kernel adds bias and residual (511 x 320: interior and edge tiles in both slabs)"""
    M, N, Kk = 511, 320, 128
    P = problem(L, M, N, Kk, 77)
    exp = P["raw"] + P["bias"].double() + P["res"][:, :N].double()
    outF, _ = launch(L, P, M, N, Kk, 0, True, "F+res", cfg=188 + 2000000)
    assert torch.isfinite(outF).all()
    err = (outF.double() - exp).abs()
    assert (err <= P["tol"]).all(), (err / P["tol"]).max().item()


def test_h2q_epilogue_conv_stats(L):
    """3x3 conv + GroupNorm sums on two stacked samples of 12 x 14 pixels (Cin 32, N 64, 8 groups): 336 rows, so the first 256-row tile holds
    all of sample 0 and part of sample 1 and the second one is ragged; N = 64 leaves three of the four wave columns without a valid column"""
    B, H, W, Cin, N, G = 2, 12, 14, 32, 64, 8
    g = torch.Generator().manual_seed(5)
    sb = torch.arange(B).float().reshape(B, 1, 1, 1)
    x = torch.randn(B, Cin, H, W, generator=g) * 2.0 * (1.0 + sb) + 0.5 * sb       # a row counted for the wrong sample moves a sum by far more than the bound
    w = torch.randn(N, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    bias = (torch.randn(N, generator=g) * 0.1).cuda()
    M = B * H * W
    A = cast_h2(L, x.permute(0, 2, 3, 1).reshape(M, Cin).contiguous().cuda())
    Wp, wscale = pack_weight_h2(L, w)
    xs = h2_decode(A, M, Cin)[0].double().reshape(B, H, W, Cin).permute(0, 3, 1, 2)
    wsd = split_weight_ref(w, wscale).cuda()
    raw = F.conv2d(xs, wsd, bias.double(), padding=1).permute(0, 2, 3, 1).reshape(M, N)
    mag = F.conv2d(xs.abs(), wsd.abs(), None, padding=1).permute(0, 2, 3, 1).reshape(M, N)
    tol = (mag * 2.0 ** -20 + 1e-6) * 1.2
    outF = torch.full((M + 1, N), float("nan"), device="cuda")
    stats = torch.zeros(64 * B, device="cuda", dtype=torch.float64)
    L.check(L.lib().uni_gemm_stacked(L.ptr(A), Cin, L.ptr(Wp), wscale, 2, B, M, N, H, W, Cin, 3, 3, 1, 1, L.ptr(bias), 0, 0, None, N, L.ptr(outF), N,
                                     0, 0, 0, M + 1, None, N, L.ptr(stats), N // G, 0, 188, L.stream_ptr()), "gemm_stacked")
    torch.cuda.synchronize()
    assert torch.isnan(outF[M]).all()                      # the row behind the last one is untouched
    err = (outF[:M].double() - raw).abs()
    assert (err <= tol).all(), (err / tol).max().item()
    grp = raw.reshape(B, H * W, G, N // G)
    s_ref = torch.stack([grp.sum((1, 3)), (grp ** 2).sum((1, 3))], 2)              # (B, G, 2)
    s_got = stats.reshape(B, 64)[:, :2 * G].reshape(B, G, 2)
    assert ((s_got - s_ref).abs() <= 2e-2 + 2e-5 * s_ref.abs()).all(), (s_got - s_ref).abs().max().item()
