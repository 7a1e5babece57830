"""The ConvNeXt training operators (csrc/pw_mlp.hip, block_tail.hip, lncf_train.hip, dwln_train.hip) at maps of more than 2^31 elements and at
column sums of training length: the shapes, the memory each case needs, the inputs (drawn chunk by chunk from seeds, so that any chunk can be
drawn again after an in-place call has overwritten it), the references (the operators' restatements in fp64, one chunk of at most CHUNK
elements at a time) and the checking functions.  tests/test_train_scale_gpu.py runs them on the device, tests/test_train_scale_cpu.py checks
the shapes against the host plans and the checking functions on small maps with the boundary moved down.

How a result is judged -- the operators' existing rule, unchanged: a map is held to 4 x the fp32 yardstick (the deviation of the same lines
in fp32 from fp64 on the same values, measured in the same pass; for pw_mlp the larger of the restatement's and of eager F.gelu + autograd),
plus half an ulp where the map is fp16 / bf16; a parameter gradient is held against the chunk-accumulated fp64 sum to 4 x the deviation of
ONE fp32 torch sum over the whole map of fp32 values.  rel_err is max |got - ref| / max |ref| over the whole map, as everywhere in tests/; it
is reported apart for the elements before and behind `boundary` (an element offset).  Every output is filled with NaN before the call and
must come back without one.  The exact runs (small integers) are held to the last bit.

The _f64 forms are not run at this size: they double the memory and share every index expression with the fp32 forms through the templates.

Importable without a device; nothing here is cached."""
import math

import torch
import torch.nn.functional as F

import block_tail_ref as RB
import dwln_train_ref as RD
import lncf_ref as RL
import pw_mlp_ref as RP

B31, B32 = 2 ** 31, 2 ** 32
BEHIND = 2 ** 24                            # at least this many elements lie behind the boundary
CHUNK = 1 << 25                             # elements of a reference chunk (the issue allows 64 M; half of it keeps the fp64 temporaries at 4 GiB)
TEMPS = 16 * 8 * CHUNK                      # bytes allowed for the temporaries of a chunk: sixteen fp64 tensors of CHUNK elements
CAP = 40 * 2 ** 30                          # no case may need more device memory than this
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
ESIZE = {"f32": 4, "f16": 2, "bf16": 2}
CODE = {"f32": 0, "f16": 1, "bf16": 2}      # the h_dtype / y_dtype / x_dtype argument of the C-ABI
HALF_ULP = {"f32": 0.0, "f16": 2.0 ** -11, "bf16": 2.0 ** -8}


def rows_past(boundary, N):
    """the smallest M with M N >= boundary + BEHIND"""
    return -(-(boundary + BEHIND) // N)


# ================================================================================================================ the shapes
# pw_mlp, part A: tag -> (dt, M, Hd, Co, boundary, forms).  Hd = 520: 65 vectors of 8 or 130 of 4 on tiles of L = 8, seven or six idle slots
# behind the last one; Co = 68: 17 vectors of 4, seven idle.  M is no multiple of the 32 rows of a block.  The 2^32 case is there for the
# `unsigned` group counters; it runs in place only.
PW_A = {
    "f16": ("f16", rows_past(B31, 520), 520, 68, B31, ("out", "in")),
    "f32": ("f32", rows_past(B31, 520), 520, 68, B31, ("out", "in")),
    "f16_2p32": ("f16", rows_past(B32, 520), 520, 68, B32, ("in",)),
}
# pw_mlp, part B: tag -> (dt, M, Hd = Co, L, terms a lane adds serially = ceil(ceil(M / rpb) / PW_ROWS)).  The smallest maps (2^28 + a few
# elements, 2^29 for fp16) that give a lane of a class with L = 256 (one row per block) and of one with L = 8 (32 rows) 1025 terms.
PW_B = {
    "f32_L256": ("f32", 262147, 1024, 256, 1025),
    "f32_L8": ("f32", 8388617, 32, 8, 1025),
    "f16_L256": ("f16", 262147, 2048, 256, 1025),
    "f16_L8": ("f16", 8388617, 64, 8, 1025),
}
PW_B_MEANS = (0.0, 1.0)
# block_tail: tag -> (dt of y, nchw, (B, C, H, W)).  Three samples, the middle one dropped; H W is no multiple of 64 (the NCHW tile) or of the
# 40 pixels of a channels-last chunk at C = 200 (V = 8, 25 lanes a pixel, PP = 20, two steps); C = 136 is two channel tiles and one of 8.
BT_A = {
    "cl": ("f16", 0, (3, 200, 1899, 1901)),
    "nchw": ("f16", 1, (3, 136, 2303, 2305)),
}
BT_SCALE = (1 / 0.7, 0.0, 1 / 0.7)
BT_SCALE_EXACT = (2.0, 0.0, 2.0)
# lncf_train: tag -> (dt of x, nchw, (B, C, H, W), plan class, idle vector slots (channels-last) or channels of the last wave slice (NCHW)).
# C = 136 in fp16: 17 vectors of 8 on G = 8 lanes of 3, seven idle; 32 pixels per block, B H W = 6 (mod 32).  NCHW: H W is no multiple of
# the 64-pixel tile and C = 4 (mod 8), so the eight waves own slices of two lengths; C = 260 streams slices of 33 and 32 in chunks of 8.
LN_A = {
    "cl": ("f16", 0, (2, 136, 2821, 2823), "cl<f16,V=8,NV=3> G=8"),
    "regs16": ("f16", 1, (2, 100, 3289, 3291), "nchw<f16,regs=16>"),
    "regs32": ("f16", 1, (2, 204, 2303, 2305), "nchw<f16,regs=32>"),
    "stream8": ("f16", 1, (2, 260, 2039, 2043), "nchw<f16,stream=8>"),
}
# dwln_train (fp32): (B, C, H, W).  H and W odd; W = 5493 is 687 strips of 8 pixels (the last of 5) and 43 strips of 128 in the weight pass
# (the last of 117); B H 687 is no multiple of the 8 strips of a block, B H 43 none of the 4 strips of a weight-pass block
DW_A = (2, 68, 2899, 5493)
DW_CLASS = "<f32,PXT=8> wps=1 NS=8"
DW_BAND = 8                                 # image rows of a value band


def elements(shape):
    return math.prod(shape)


def pw_need(tag):
    """bytes at the peak of a part-A pw_mlp case: h, grad_a and two more maps of the element type (the outputs of the out-of-place call, or the
    copies of the first in-place call), grad_y, and the fp32 map of the sum yardstick where it cannot reuse one of those (half types: it is
    allocated after the two spare maps are freed, so the peak is the larger of the two stages)"""
    dt, M, Hd, Co, _, _ = PW_A[tag]
    e = ESIZE[dt]
    maps, gy = M * Hd * e, M * Co * e
    stage1 = 4 * maps + gy
    stage2 = 2 * maps + gy + M * Co * 4 + M * Hd * 4 if dt != "f32" else 0
    return max(stage1, stage2) + TEMPS


def pw_b_need(tag):
    """h, grad_a, grad_y of the element type, the fp32 map of the yardstick and one fp32 copy of grad_y"""
    dt, M, Hd, _, _ = PW_B[tag]
    return 3 * M * Hd * ESIZE[dt] + 2 * M * Hd * 4 + TEMPS


def bt_need(tag):
    """y (half), x and out (fp32), and either the second out or the two grad_y (half); the check holds less: out, grad_y and the yardstick's map"""
    dt, _, shape = BT_A[tag]
    E = elements(shape)
    return E * (ESIZE[dt] + 3 * 4) + TEMPS


def ln_need(tag):
    """second backward call: x and two grad_x (half), y and grad_y (fp32), stats; the check holds as much: the yardstick's map for x and a grad_x"""
    dt, _, shape, _ = LN_A[tag]
    E = elements(shape)
    return E * (3 * ESIZE[dt] + 2 * 4) + 2 * 4 * (E // shape[1]) + TEMPS


def dw_workspace(shape):
    """uni_dwln_train_workspace_bytes restated (include/unicorn_hip.h)"""
    B, C, H, W = shape
    up = lambda n: -(-n // 64) * 64                                  # noqa: E731
    NS = 512 // (64 * -(-C // 256))
    RA = min(-(-(B * H * -(-W // 2)) // NS), 1024)
    slen = -(-W // -(-W // 128))
    RB_ = -(-(B * H * -(-W // slen)) // 4)
    return 4 * (up(B * H * W * C) + up(2 * C * RA) + up(50 * C * RB_))


def dw_need():
    """backward with grad_x: x, grad_y, grad_x, the workspace (du and the partials) and stats; the check of the parameter gradients holds as
    many maps (x, grad_y and the two fp32 maps of the yardstick)"""
    E = elements(DW_A)
    return 3 * 4 * E + dw_workspace(DW_A) + 2 * 4 * (E // DW_A[1]) + TEMPS


# ================================================================================================================ shared pieces
class Err:
    """running max |got - ref| before and behind the boundary, and max |ref|"""

    def __init__(self):
        self.lo = self.hi = self.ref = 0.0

    def add(self, got, ref, split):
        """rows [0, split) lie before the boundary, the others behind it"""
        d = (got.double() - ref).abs()
        if split > 0:
            self.lo = max(self.lo, float(d[:split].max()))
        if split < d.shape[0]:
            self.hi = max(self.hi, float(d[split:].max()))
        self.ref = max(self.ref, float(ref.abs().max()))

    def rel(self):
        """(before, behind), NaN-propagating: a NaN in `got` gives NaN, which no bound admits"""
        return self.lo / self.ref, self.hi / self.ref


def sum_err(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def normal_chunk(seed, i, rows, N, device, mean=0.0):
    """chunk i of a map of plain fp32 normal draws (+ mean)"""
    g = torch.Generator(device=device).manual_seed(seed * 1000003 + i)
    t = torch.randn(rows, N, generator=g, device=device)
    return t + mean if mean else t


def count_nan(t, chunk=1 << 28):
    """NaNs of a buffer of any shape, counted in pieces"""
    flat = t.reshape(-1)
    return sum(int(torch.isnan(flat[i:i + chunk]).sum()) for i in range(0, flat.numel(), chunk))


def same_bits(a, b, chunk=1 << 28):
    """torch.equal in pieces (NaN is equal to nothing: a buffer that kept its NaN fill differs)"""
    a, b = a.reshape(-1), b.reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and all(torch.equal(a[i:i + chunk], b[i:i + chunk]) for i in range(0, a.numel(), chunk))


def digest(t, chunk=1 << 25):
    """a position-weighted sum of the bit patterns, for the one map that has no room for a second copy (dwln grad_x)"""
    flat = t.reshape(-1).view(torch.int32 if t.element_size() == 4 else torch.int16)
    tot = 0
    for i in range(0, flat.numel(), chunk):
        p = flat[i:i + chunk].to(torch.int64)
        w = torch.arange(i, i + p.numel(), device=t.device) % 65521 + 1
        tot = (tot + int((p * w).sum())) % (1 << 61)
    return tot


class Report(dict):
    """{result: (err before, err behind, bound)} plus .nan {buffer: count}, .yard {result: yardstick(s)}, .wrong {buffer: exact mismatches}"""

    def __init__(self):
        super().__init__()
        self.nan, self.yard, self.wrong, self.notes = {}, {}, {}, []

    def failures(self):
        bad = ["%s: err %.3e / %.3e, bound %.3e" % ((n,) + v) for n, v in self.items() if not (v[0] <= v[2] and v[1] <= v[2])]
        bad += ["%s: %d NaN left" % kv for kv in self.nan.items() if kv[1]]
        bad += ["%s: %s" % kv for kv in self.wrong.items() if kv[1]]
        bad += ["%s: yardstick %r is not positive" % kv for kv in self.yard.items() if not all(y > 0 for y in kv[1])]
        return bad

    def lines(self):
        out = ["%-10s err %.3e (before) %.3e (behind)  bound %.3e  err/bound %.3f" % (n, v[0], v[1], v[2], max(v[0], v[1]) / v[2] if v[2] else math.inf)
               for n, v in self.items()]
        return out + ["%-10s %s" % (k, v or "equal to the last bit") for k, v in self.wrong.items()] + self.notes


# ================================================================================================================ pw_mlp
class PwCase:
    """inputs of one pw_mlp case, drawn per chunk of whole rows.  exact: None, or the base b of the integer pattern (pw_mlp_ref.exact_maps
    has b = 1; b = 0 keeps the sums of more than 2^24 / 3 rows below 2^24)"""

    def __init__(self, dt, M, Hd, Co, mean=0.0, exact=None, seed=11, chunk=CHUNK):
        self.dt, self.M, self.Hd, self.Co, self.mean, self.exact, self.seed, self.chunk = dt, M, Hd, Co, mean, exact, seed, chunk
        self.dtype = DT[dt]

    def spans(self, N):
        rows = max(1, self.chunk // N)
        return [(i, r0, min(r0 + rows, self.M)) for i, r0 in enumerate(range(0, self.M, rows))]

    def _pattern(self, r0, r1, N, mul, device):
        r, c = torch.arange(r0, r1, device=device)[:, None], torch.arange(N, device=device)[None, :]
        return (self.exact + (mul * r + c) % 3).to(self.dtype)

    def h(self, i, r0, r1, device):
        if self.exact is not None:
            return torch.full((r1 - r0, self.Hd), 30.0, device=device, dtype=self.dtype)
        return normal_chunk(self.seed, i, r1 - r0, self.Hd, device).to(self.dtype)

    def ga(self, i, r0, r1, device):
        if self.exact is not None:
            return self._pattern(r0, r1, self.Hd, 1, device)
        return normal_chunk(self.seed + 1, i, r1 - r0, self.Hd, device, self.mean).to(self.dtype)

    def gy(self, i, r0, r1, device):
        if self.exact is not None:
            return self._pattern(r0, r1, self.Co, 2, device)
        return normal_chunk(self.seed + 2, i, r1 - r0, self.Co, device, self.mean).to(self.dtype)

    def fill(self, name, buf):
        """buf (M, Hd or Co) <- the map `name` (h, ga or gy)"""
        for i, r0, r1 in self.spans(buf.shape[1]):
            buf[r0:r1] = getattr(self, name)(i, r0, r1, buf.device)
        return buf


PW_KEY = {"a_fwd": "a", "a": "a", "grad_h": "grad_h"}


def pw_check(case, out, boundary=B31, scratch=None, gy=None):
    """out: any of a_fwd, a, grad_h ((M, Hd) maps of the case's type), g_b1 (Hd,), g_b2 (Co,) fp32 -> Report.  scratch: an fp32 (M, Hd) buffer
    for the fp32 grad_h whose one torch sum is the yardstick of g_b1 (allocated here when None); gy: the grad_y buffer the kernel read
    (drawn again when None)"""
    assert case.exact is None
    rep = Report()
    maps = [n for n in ("a_fwd", "a", "grad_h") if out.get(n) is not None]
    dev = next(v for v in out.values() if v is not None).device
    M, Hd, Co = case.M, case.Hd, case.Co
    split = boundary // Hd
    acc = {n: Err() for n in maps}
    yr, ye = {k: Err() for k in ("a", "grad_h")}, {k: Err() for k in ("a", "grad_h")}
    s1 = torch.zeros(Hd, dtype=torch.float64, device=dev)
    if scratch is None:
        scratch = torch.empty(M, Hd, dtype=torch.float32, device=dev)
    for i, r0, r1 in case.spans(Hd):
        h, ga = case.h(i, r0, r1, dev), case.ga(i, r0, r1, dev)
        ref = RP.act_maps(h.double(), ga.double())
        s1 += ref["g_b1"]
        cut = min(max(split - r0, 0), r1 - r0)
        for n in maps:
            acc[n].add(out[n][r0:r1], ref[PW_KEY[n]], cut)
        f32 = RP.act_maps(h.float(), ga.float())
        he = h.float().requires_grad_(True)
        ae = F.gelu(he)
        ae.backward(ga.float())
        for k, e in (("a", ae.detach()), ("grad_h", he.grad)):
            yr[k].add(f32[k], ref[k], cut)
            ye[k].add(e, ref[k], cut)
        scratch[r0:r1] = f32["grad_h"]
        del ref, f32, he, ae, h, ga
    for k in ("a", "grad_h"):
        rep.yard[k] = (max(yr[k].rel()), max(ye[k].rel()))
    for n in maps:
        rep[n] = acc[n].rel() + (4 * max(rep.yard[PW_KEY[n]]) + HALF_ULP[case.dt],)
        rep.nan[n] = count_nan(out[n])
    if out.get("g_b1") is not None:
        y = sum_err(scratch.sum(0), s1)
        rep.yard["g_b1"] = (y,)
        rep["g_b1"] = (0.0, sum_err(out["g_b1"], s1), 4 * y)
        rep.nan["g_b1"] = count_nan(out["g_b1"])
    if out.get("g_b2") is not None:
        if gy is None:
            gy = case.fill("gy", torch.empty(M, Co, dtype=case.dtype, device=dev))
        s2 = torch.zeros(Co, dtype=torch.float64, device=dev)
        for _, r0, r1 in case.spans(Co):
            s2 += gy[r0:r1].double().sum(0)
        y = sum_err(gy.float().sum(0), s2)
        rep.yard["g_b2"] = (y,)
        rep["g_b2"] = (0.0, sum_err(out["g_b2"], s2), 4 * y)
        rep.nan["g_b2"] = count_nan(out["g_b2"])
    return rep


def pw_check_exact(case, out):
    """the integer run: a == h == 30, grad_h == grad_a and both sums to the last bit -> Report with .wrong only"""
    assert case.exact is not None
    rep = Report()
    dev = next(v for v in out.values() if v is not None).device
    wrong = {n: 0 for n in ("a_fwd", "a", "grad_h") if out.get(n) is not None}
    s1 = torch.zeros(case.Hd, dtype=torch.float64, device=dev)
    s2 = torch.zeros(case.Co, dtype=torch.float64, device=dev)
    for i, r0, r1 in case.spans(case.Hd):
        ga = case.ga(i, r0, r1, dev)
        s1 += ga.double().sum(0)
        for n in wrong:
            want = ga if n == "grad_h" else case.h(i, r0, r1, dev)
            wrong[n] += int((out[n][r0:r1] != want).sum())
    for i, r0, r1 in case.spans(case.Co):
        s2 += case.gy(i, r0, r1, dev).double().sum(0)
    assert float(s1.max()) < 2 ** 24 and float(s2.max()) < 2 ** 24, "the integer sums must stay exact in fp32"
    for n, s in (("g_b1", s1), ("g_b2", s2)):
        if out.get(n) is not None:
            wrong[n] = int((out[n].double() != s).sum())
    rep.wrong = {n: ("%d elements differ" % k if k else "") for n, k in wrong.items()}
    return rep


# ================================================================================================================ maps of pixels (block_tail, lncf)
class PixCase:
    """a (B, C, H, W) case whose maps are drawn per chunk of whole pixels of ONE image, in channels-last order (q, C); store / load move a chunk
    into / out of a buffer in either memory layout"""

    def __init__(self, dt, nchw, shape, seed=23, exact=False, chunk=CHUNK):
        self.dt, self.nchw, self.shape, self.seed, self.exact, self.chunk = dt, nchw, shape, seed, exact, chunk
        self.B, self.C, self.H, self.W = shape
        self.HW, self.M = self.H * self.W, self.B * self.H * self.W
        self.dtype = DT[dt]

    def spans(self):
        """[(chunk index, n, q0, q1)]"""
        rows = max(1, self.chunk // self.C)
        return [(n * 100000 + k, n, q0, min(q0 + rows, self.HW)) for n in range(self.B) for k, q0 in enumerate(range(0, self.HW, rows))]

    def normal(self, which, i, n, q0, q1, device):
        return normal_chunk(self.seed + which, i, q1 - q0, self.C, device)

    def ints(self, mul, mod, n, q0, q1, device, add=0):
        q, c = torch.arange(q0, q1, device=device)[:, None], torch.arange(self.C, device=device)[None, :]
        return ((q + mul * c + n) % mod + add).float()

    def store(self, buf, nchw, n, q0, q1, chunk):
        if nchw:
            buf.view(self.B, self.C, self.HW)[n, :, q0:q1] = chunk.t()
        else:
            buf.view(self.M, self.C)[n * self.HW + q0:n * self.HW + q1] = chunk

    def load(self, buf, nchw, n, q0, q1):
        if nchw:
            return buf.view(self.B, self.C, self.HW)[n, :, q0:q1].t()
        return buf.view(self.M, self.C)[n * self.HW + q0:n * self.HW + q1]

    def fill(self, fn, buf, nchw):
        for i, n, q0, q1 in self.spans():
            self.store(buf, nchw, n, q0, q1, fn(i, n, q0, q1, buf.device).to(buf.dtype))
        return buf

    def cut(self, boundary, n, q0, q1):
        """rows of the chunk before the boundary (an element offset in the channels-last map)"""
        return min(max(boundary // self.C - (n * self.HW + q0), 0), q1 - q0)

    def whole_sum(self, buf, nchw):
        """one torch sum over every pixel of an fp32 map -> (C,)"""
        return buf.view(self.B, self.C, self.HW).sum((0, 2)) if nchw else buf.view(self.M, self.C).sum(0)


# ---------------------------------------------------------------------------------------------------------------- block_tail
class BtCase(PixCase):
    """y (channels-last, half), x = residual in the forward and grad_out in the backward (fp32, either layout), gamma, scale"""

    def __init__(self, dt, nchw, shape, exact=False, **kw):
        super().__init__(dt, nchw, shape, exact=exact, **kw)
        self.scale = torch.tensor(BT_SCALE_EXACT if exact else BT_SCALE, dtype=torch.float32)
        assert len(self.scale) == self.B
        if exact:
            self.gamma = (1 + torch.arange(self.C) % 3).float()
        else:
            self.gamma = 0.5 * torch.randn(self.C, generator=torch.Generator().manual_seed(self.seed))

    def y(self, i, n, q0, q1, device):
        return (self.ints(1, 2, n, q0, q1, device) if self.exact else self.normal(0, i, n, q0, q1, device)).to(self.dtype)

    def x(self, i, n, q0, q1, device):
        return self.ints(2, 3, n, q0, q1, device) if self.exact else self.normal(1, i, n, q0, q1, device)


def _bt_lines(y, x, gamma, s, dtype):
    """block_tail_ref.value_and_grads on a chunk (q, C) of one image with the factor s; x is residual and grad_out -> out, g_y (q, C), g_gamma"""
    q, C = y.shape
    r = RB.value_and_grads(y.float().reshape(1, q, 1, C), x.t().reshape(1, C, q, 1), gamma, s.reshape(1), x.t().reshape(1, C, q, 1), dtype=dtype)
    return r["out"][0, :, :, 0].t(), r["g_y"][0, :, 0, :], r["g_gamma"]


def bt_check(case, out, boundary=B31, scratch=None):
    """out: out (M, C) fp32, g_y (M, C) half, g_gamma (C,) -> Report.  scratch: an fp32 (M, C) buffer for the products whose one torch sum is
    the yardstick of g_gamma.  With exact inputs every result is held to the last bit instead"""
    rep = Report()
    dev = next(v for v in out.values() if v is not None).device
    M, C = case.M, case.C
    gamma, scale = case.gamma.to(dev), case.scale.to(dev)
    maps = [n for n in ("out", "g_y") if out.get(n) is not None]
    acc, yard = {n: Err() for n in maps}, {n: Err() for n in ("out", "g_y")}
    wrong = {n: 0 for n in maps}
    sg = torch.zeros(C, dtype=torch.float64, device=dev)
    if scratch is None and not case.exact:
        scratch = torch.empty(M, C, dtype=torch.float32, device=dev)
    for i, n, q0, q1 in case.spans():
        y, x = case.y(i, n, q0, q1, dev), case.x(i, n, q0, q1, dev)
        ref = dict(zip(("out", "g_y", "g_gamma"), _bt_lines(y, x, gamma, scale[n], torch.float64)))
        sg += ref["g_gamma"]
        r0 = n * case.HW
        if case.exact:
            for k in maps:
                wrong[k] += int((out[k][r0 + q0:r0 + q1].double() != ref[k]).sum())
            continue
        cut = case.cut(boundary, n, q0, q1)
        f32 = dict(zip(("out", "g_y", "g_gamma"), _bt_lines(y, x, gamma, scale[n], torch.float32)))
        for k in maps:
            acc[k].add(out[k][r0 + q0:r0 + q1], ref[k], cut)
        for k in ("out", "g_y"):
            yard[k].add(f32[k], ref[k], cut)
        scratch[r0 + q0:r0 + q1] = (x * scale[n]) * y.float()
    for k in maps + (["g_gamma"] if out.get("g_gamma") is not None else []):
        rep.nan[k] = count_nan(out[k])
    if case.exact:
        assert float(sg.abs().max()) < 2 ** 24, "the integer sums must stay exact in fp32"
        if out.get("g_gamma") is not None:
            wrong["g_gamma"] = int((out["g_gamma"].double() != sg).sum())
        rep.wrong = {n: ("%d elements differ" % k if k else "") for n, k in wrong.items()}
        return rep
    for k in maps:
        rep.yard[k] = (max(yard[k].rel()),)
        rep[k] = acc[k].rel() + (4 * rep.yard[k][0] + (HALF_ULP[case.dt] if k == "g_y" else 0.0),)
    if out.get("g_gamma") is not None:
        yg = sum_err(scratch.sum(0), sg)
        rep.yard["g_gamma"] = (yg,)
        rep["g_gamma"] = (0.0, sum_err(out["g_gamma"], sg), 4 * yg)
    return rep


# ---------------------------------------------------------------------------------------------------------------- lncf_train
class LnCase(PixCase):
    """x (half) and grad_y (fp32) in the layout under test, weight = 1 + 0.1 n, bias = 0.1 n"""

    def __init__(self, dt, nchw, shape, **kw):
        super().__init__(dt, nchw, shape, **kw)
        g = torch.Generator().manual_seed(self.seed)
        self.weight, self.bias = 1.0 + 0.1 * torch.randn(self.C, generator=g), 0.1 * torch.randn(self.C, generator=g)

    def x(self, i, n, q0, q1, device):
        return self.normal(0, i, n, q0, q1, device).to(self.dtype)

    def gy(self, i, n, q0, q1, device):
        return self.normal(1, i, n, q0, q1, device)


def _ln_lines(x, gy, w, b, dtype):
    """lncf_ref.value_and_grads on a chunk (q, C) -> y, g_x (q, C), g_weight, g_bias, stats (q, 2) = mean, rstd"""
    q, C = x.shape
    xx = x.float().t().reshape(1, C, q, 1)
    r = RL.value_and_grads(xx, w, b, gy.t().reshape(1, C, q, 1), dtype=dtype)
    xd = x.to(dtype)
    u = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt((xd - u).pow(2).mean(1, keepdim=True) + RL.EPS)
    return {"y": r["y"][0, :, :, 0].t(), "g_x": r["g_x"][0, :, :, 0].t(), "g_weight": r["g_weight"], "g_bias": r["g_bias"],
            "stats": torch.cat([u, rstd], 1), "xhat": (xd - u) * rstd}


def ln_check(case, out, boundary=B31, scratch=None, gy=None):
    """out: y (fp32), g_x (half) in the case's layout, stats (M, 2), g_weight, g_bias (C,) -> Report.  scratch: an fp32 buffer of the map's size
    for the products grad_y xhat whose one torch sum is the yardstick of g_weight; gy: the grad_y buffer the kernel read, for that of g_bias"""
    rep = Report()
    dev = next(v for v in out.values() if v is not None).device
    C = case.C
    w, b = case.weight.to(dev), case.bias.to(dev)
    maps = [n for n in ("y", "g_x", "stats") if out.get(n) is not None]
    acc, yard = {n: Err() for n in maps}, {n: Err() for n in ("y", "g_x", "stats")}
    sw, sb = torch.zeros(C, dtype=torch.float64, device=dev), torch.zeros(C, dtype=torch.float64, device=dev)
    if scratch is None:
        scratch = torch.empty(case.M * C, dtype=torch.float32, device=dev)
    if gy is None:
        gy = case.fill(case.gy, torch.empty(case.M * C, dtype=torch.float32, device=dev), case.nchw)
    for i, n, q0, q1 in case.spans():
        x, g = case.x(i, n, q0, q1, dev), case.gy(i, n, q0, q1, dev)
        ref, f32 = _ln_lines(x, g, w, b, torch.float64), _ln_lines(x, g, w, b, torch.float32)
        sw += ref["g_weight"]
        sb += ref["g_bias"]
        cut = case.cut(boundary, n, q0, q1)
        for k in maps:
            got = out[k][n * case.HW + q0:n * case.HW + q1] if k == "stats" else case.load(out[k], case.nchw, n, q0, q1)
            acc[k].add(got, ref[k], cut)
        for k in yard:
            yard[k].add(f32[k], ref[k], cut)
        case.store(scratch, case.nchw, n, q0, q1, g * f32["xhat"])
        del ref, f32
    for k in maps:
        rep.yard[k] = (max(yard[k].rel()),)
        rep[k] = acc[k].rel() + (4 * rep.yard[k][0] + (HALF_ULP[case.dt] if k == "g_x" else 0.0),)
    for k, ref, src in (("g_weight", sw, scratch), ("g_bias", sb, gy)):
        if out.get(k) is not None:
            y = sum_err(case.whole_sum(src, case.nchw), ref)
            rep.yard[k] = (y,)
            rep[k] = (0.0, sum_err(out[k], ref), 4 * y)
    for k in out:
        if out[k] is not None:
            rep.nan[k] = count_nan(out[k])
    return rep


# ================================================================================================================ dwln_train
class DwCase:
    """x on the 2^-6 grid and grad_y plain, drawn per band of whole image rows (channels-last [B][H][W][C]); the parameters as dwln_train_ref.draw"""

    def __init__(self, shape, seed=37, band=64):
        self.shape, self.seed, self.band = shape, seed, band
        self.B, self.C, self.H, self.W = shape
        g = torch.Generator().manual_seed(seed)
        C = self.C
        self.weight = RD._grid(torch.randn(C, 1, 7, 7, generator=g) / 7, 8)
        self.bias = RD._grid(0.1 * torch.randn(C, generator=g), 10)
        self.ln_weight = 1 + RD._grid(0.1 * torch.randn(C, generator=g), 10)
        self.ln_bias = RD._grid(0.1 * torch.randn(C, generator=g), 10)

    def w49(self):
        """the C-ABI's weight layout [49][C]"""
        return self.weight.reshape(self.C, 49).t().contiguous()

    def spans(self):
        """[(chunk index, n, r0, r1)]: bands of image rows of one image"""
        return [(n * 100000 + k, n, r0, min(r0 + self.band, self.H)) for n in range(self.B) for k, r0 in enumerate(range(0, self.H, self.band))]

    def x(self, i, n, r0, r1, device):
        return RD._grid(normal_chunk(self.seed, i, (r1 - r0) * self.W, self.C, device), 6).view(r1 - r0, self.W, self.C)

    def gy(self, i, n, r0, r1, device):
        return normal_chunk(self.seed + 1, i, (r1 - r0) * self.W, self.C, device).view(r1 - r0, self.W, self.C)

    def fill(self, fn, buf):
        v = buf.view(self.B, self.H, self.W, self.C)
        for i, n, r0, r1 in self.spans():
            v[n, r0:r1] = fn(i, n, r0, r1, buf.device)
        return buf

    def value_bands(self, boundary=B31):
        """[(name, n, r0, r1)]: the first DW_BAND rows, the last, and the rows around the one in which the element offset passes the boundary"""
        rg = boundary // (self.W * self.C)
        n, r = divmod(rg, self.H)
        assert n < self.B, "the boundary lies behind the map"
        lo = min(max(r - DW_BAND // 2, 0), self.H - DW_BAND)
        return [("first", 0, 0, DW_BAND), ("boundary", n, lo, lo + DW_BAND), ("last", self.B - 1, self.H - DW_BAND, self.H)]


def dw_band_check(case, x, gy, out, boundary=B31):
    """y, stats and grad_x (whichever are given) in the three value bands against dwln_train_ref in fp64 on the CPU, computed on the band with a
    halo of 6 image rows (3 suffice for y): -> Report; the yardstick is the same restatement in fp32 on the same rows"""
    rep = Report()
    B, C, H, W = case.shape
    v = lambda t, last=C: t.view(B, H, W, last)                                   # noqa: E731
    params = (case.weight, case.bias, case.ln_weight, case.ln_bias)
    for name, n, r0, r1 in case.value_bands(boundary):
        h0, h1 = max(r0 - 6, 0), min(r1 + 6, H)
        xb = v(x)[n, h0:h1].cpu().permute(2, 0, 1).unsqueeze(0).contiguous()
        gb = v(gy)[n, h0:h1].cpu().unsqueeze(0) if gy is not None else torch.zeros(1, h1 - h0, W, C)
        ref = RD.value_and_grads(xb.double(), *(p.double() for p in params), gb.double())
        f32 = RD.value_and_grads(xb, *params, gb)
        sl = slice(r0 - h0, r1 - h0)
        for r in (ref, f32):
            u = F.conv2d(xb.to(r["y"].dtype), case.weight.to(r["y"].dtype), case.bias.to(r["y"].dtype), padding=3, groups=C).permute(0, 2, 3, 1)
            m = u.mean(-1, keepdim=True)
            r["stats"] = torch.cat([m, 1.0 / torch.sqrt((u - m).pow(2).mean(-1, keepdim=True) + RD.EPS)], -1)
            r["gx"] = r["gx"].permute(0, 2, 3, 1)
        for k, key in (("y", "y"), ("stats", "stats"), ("grad_x", "gx")):
            if out.get(k) is None:
                continue
            got = v(out[k], 2 if k == "stats" else C)[n, r0:r1].cpu()
            want, near = ref[key][0, sl], f32[key][0, sl]
            behind = (n * H + r1) * W * C > boundary                              # the band ends behind the boundary
            e = float((got.double() - want).abs().max() / want.abs().max())
            y = float((near.double() - want).abs().max() / want.abs().max())
            rep.yard["%s %s" % (k, name)] = (y,)
            rep["%s %s" % (k, name)] = (0.0 if behind else e, e if behind else 0.0, 4 * y)
    for k in out:
        if out[k] is not None:
            rep.nan[k] = count_nan(out[k])
    return rep


def dw_param_reference(case, x, gy, dtype=torch.float64, keep=None):
    """grad_weight [49][C], grad_bias, grad_ln_weight, grad_ln_bias of the whole map, accumulated band by band on the device of x from shifted
    multiply-adds on channels-last slices (no convolution call): u = b + sum w[ky][kx] x[. + ky - 3][. + kx - 3], the LayerNorm backward per
    pixel, dw[ky][kx] = sum du x[. + ky - 3][. + kx - 3].  In `dtype`; every band sum is one torch sum, the bands are added in `dtype`.
    keep: two buffers of the map's size that receive grad_y xhat and du of every band"""
    B, C, H, W = case.shape
    dev = x.device
    xv, gv = x.view(B, H, W, C), gy.view(B, H, W, C)
    w = case.w49().to(dev, dtype)
    b, gam = case.bias.to(dev, dtype), case.ln_weight.to(dev, dtype)
    gw = torch.zeros(49, C, dtype=dtype, device=dev)
    gb, gg, gbe = (torch.zeros(C, dtype=dtype, device=dev) for _ in range(3))
    for _, n, r0, r1 in case.spans():
        R = r1 - r0
        xp = torch.zeros(R + 6, W + 6, C, dtype=dtype, device=dev)
        h0, h1 = max(r0 - 3, 0), min(r1 + 3, H)
        xp[h0 - (r0 - 3):h1 - (r0 - 3), 3:W + 3] = xv[n, h0:h1]
        u = b.expand(R, W, C).clone()
        for t in range(49):
            u.addcmul_(xp[t // 7:t // 7 + R, t % 7:t % 7 + W], w[t])
        m = u.mean(-1, keepdim=True)
        u -= m
        rstd = 1.0 / torch.sqrt(u.pow(2).mean(-1, keepdim=True) + RD.EPS)
        u *= rstd                                                                  # xhat
        g = gv[n, r0:r1].to(dtype)
        gu = g * u
        gg += gu.sum((0, 1))
        gbe += g.sum((0, 1))
        g = g * gam
        du = rstd * (g - g.mean(-1, keepdim=True) - u * (g * u).mean(-1, keepdim=True))
        gb += du.sum((0, 1))
        if keep is not None:
            keep[0].view(B, H, W, C)[n, r0:r1] = gu
            keep[1].view(B, H, W, C)[n, r0:r1] = du
        for t in range(49):
            gw[t] += (du * xp[t // 7:t // 7 + R, t % 7:t % 7 + W]).sum((0, 1))
        del xp, u, g, gu, du
    return {"grad_weight": gw, "grad_bias": gb, "grad_ln_weight": gg, "grad_ln_bias": gbe}


def dw_whole_map_sums(case, x, gy, prod, du):
    """the four sums as ONE fp32 torch sum over the whole map each (49 for grad_weight), from the fp32 maps prod = grad_y xhat and du that
    dw_param_reference kept: the yardstick of a parameter gradient.  prod is overwritten with the shifted products du x"""
    B, C, H, W = case.shape
    M = B * H * W
    rows = lambda t: t.view(M, C)                                                 # noqa: E731
    out = {"grad_ln_weight": rows(prod).sum(0), "grad_ln_bias": rows(gy).sum(0), "grad_bias": rows(du).sum(0)}
    gw = torch.empty(49, C, dtype=torch.float32, device=x.device)
    xv, dv, pv = (t.view(B, H, W, C) for t in (x, du, prod))
    for t in range(49):
        dy, dx = t // 7 - 3, t % 7 - 3
        y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
        torch.mul(dv[:, y0:y1, x0:x1], xv[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx], out=pv[:, y0:y1, x0:x1])
        pv[:, :y0], pv[:, y1:], pv[:, :, :x0], pv[:, :, x1:] = 0, 0, 0, 0         # the pixels whose neighbour lies outside the image
        gw[t] = rows(prod).sum(0)
    out["grad_weight"] = gw
    return out


def dw_param_check(case, x, gy, out):
    """the four parameter gradients against dw_param_reference in fp64.  The yardstick is the rule for a sum: the same lines in fp32, each
    gradient ONE torch sum over the whole map (dw_whole_map_sums).  The band-wise fp32 accumulation -- 64 image rows per torch sum, the
    bands added in fp32 -- is closer to fp64 than that; its deviation is reported next to it, for the record -> Report"""
    rep = Report()
    ref = dw_param_reference(case, x, gy)
    prod, du = (torch.empty(x.numel(), dtype=torch.float32, device=x.device) for _ in range(2))
    banded = dw_param_reference(case, x, gy, torch.float32, keep=(prod, du))
    whole = dw_whole_map_sums(case, x, gy, prod, du)
    for k in ref:
        if out.get(k) is not None:
            y = sum_err(whole[k], ref[k])
            rep.yard[k] = (y,)
            rep[k] = (0.0, sum_err(out[k].view_as(ref[k]), ref[k]), 4 * y)
            rep.notes.append("%s: fp32 in bands of %d rows deviates by %.3e" % (k, case.band, sum_err(banded[k], ref[k])))
            rep.nan[k] = count_nan(out[k])
    return rep
