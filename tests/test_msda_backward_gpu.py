"""MSDeformAttn backward on the MI355X (csrc/msda.hip msda_bwd_kernel behind uni_msda_bwd / uni_msda_bwd_f64) through the public
surface: unicorn_amd.ops.msda_backward, MSDeformAttnFunction and the fp64 forward.

Yardsticks: tests/golden/msda_backward.npz (the reference's own pure-PyTorch core under fp64 autograd, see
tests/golden/make_golden_msda_backward.py) and, for geometries the fixture cannot hold, oracle.msda_core under fp64 autograd on the CPU
(tests/test_msda_backward_cpu.py pins it to the fixture at 1e-12).  Bounds:
  fp64  1e-12 x tensor max: an fp64 evaluation of the same formula; the sums have at most Lq*P addends per destination, so the reorder
        error n * 2^-53 * sum|terms| is far below that bar.
  fp32  max|got - ref| / max|ref| <= 4 x the fp32-vs-fp64 error of the YARDSTICK's own fp32 evaluation of the same inputs, per tensor
        (the factor 4 for a different operation order and FMA contraction).  Never a figure taken from the kernel.
Every set of sampling locations is lattice-safe (no pixel coordinate within 1e-3 of an integer, by construction, nothing excluded):
grad_sampling_loc is discontinuous there and fp32 / fp64 could floor differently."""
import importlib.util
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("a", "b", "c")
NAMES = ("grad_value", "grad_loc", "grad_attn")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_msda_backward",
                                                  os.path.join(ROOT, "tests", "golden", "make_golden_msda_backward.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


GEN = _generator()


def _lsi(shapes):
    s = torch.as_tensor(shapes, dtype=torch.long)
    return s, torch.cat((s.new_zeros((1,)), s.prod(1).cumsum(0)[:-1]))


def _relmax(got, ref):
    return float((got.detach().double().cpu() - ref.double()).abs().max() / ref.double().abs().max())


def _load(golden_dir, case):
    g = np.load(os.path.join(golden_dir, "msda_backward.npz"))
    shapes = [tuple(int(v) for v in r) for r in g["shapes_" + case]]
    t = {k: torch.from_numpy(g[k + "_" + case]) for k in ("value", "loc", "attn", "grad_out", "out") + NAMES}
    assert GEN.lattice_ok(t["loc"], shapes)
    return shapes, t, g["fp32_ref_err_" + case]


def _hip_grads(dtype, shapes, value, loc, attn, gout):
    """out and the three gradients through MSDeformAttnFunction.apply(...).backward(grad_out) on cuda:0"""
    from unicorn_amd.ops import MSDeformAttnFunction
    shp, lsi = _lsi(shapes)
    v, l, a = (t.to(dtype).cuda().requires_grad_(True) for t in (value, loc, attn))
    out = MSDeformAttnFunction.apply(v, shp.cuda(), lsi.cuda(), l, a, 64)
    out.backward(gout.to(dtype).cuda())
    torch.cuda.synchronize()
    return out.detach(), v.grad, l.grad, a.grad


def _oracle_grads(dtype, shapes, value, loc, attn, gout):
    import unicorn_oracle as uo
    v, l, a = (t.to(dtype).clone().requires_grad_(True) for t in (value, loc, attn))
    out = uo.msda_core(v, shapes, l, a)
    out.backward(gout.to(dtype))
    return out.detach(), v.grad, l.grad, a.grad


def _random_problem(seed, N, shapes, M, D, Lq, P, lo, hi, vscale=1.0):
    g = torch.Generator().manual_seed(seed)
    L, S = len(shapes), sum(h * w for h, w in shapes)
    value = torch.randn(N, S, M, D, generator=g) * vscale
    loc = GEN.make_lattice_safe(torch.rand(N, Lq, M, L, P, 2, generator=g) * (hi - lo) + lo, shapes)
    attn = torch.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P)
    gout = torch.randn(N, Lq, M * D, generator=g)
    assert GEN.lattice_ok(loc, shapes)
    return value, loc, attn, gout


# ---------------------------------------------------------------------------------------------------- 1, 2, 8: the fixture
@pytest.mark.parametrize("case", CASES)
def test_fp64_against_fixture(case, golden_dir):
    shapes, t, _ = _load(golden_dir, case)
    got = _hip_grads(torch.float64, shapes, t["value"], t["loc"], t["attn"], t["grad_out"])
    for name, g in zip(("out",) + NAMES, got):
        err = _relmax(g, t[name])
        print("fp64 case %s %s: rel-to-max err %.3e (bound 1e-12)" % (case, name, err))
    for name, g in zip(("out",) + NAMES, got):
        assert g.dtype == torch.float64 and g.shape == t[name].shape
        assert _relmax(g, t[name]) <= 1e-12, name


@pytest.mark.parametrize("case", CASES)
def test_fp32_against_fixture(case, golden_dir):
    shapes, t, ref_err = _load(golden_dir, case)
    got = _hip_grads(torch.float32, shapes, t["value"], t["loc"], t["attn"], t["grad_out"])[1:]
    errs = [_relmax(g, t[name]) for name, g in zip(NAMES, got)]
    for name, e, r in zip(NAMES, errs, ref_err):
        print("fp32 case %s %s: rel-to-max err %.3e, reference's own fp32 err %.3e, ratio %.2f (bound 4)" % (case, name, e, r, e / r))
    for name, g, e, r in zip(NAMES, got, errs, ref_err):
        assert g.dtype == torch.float32
        assert e <= 4 * r, (name, e, r)


@pytest.mark.parametrize("case", CASES)
def test_forward_fp64_against_fixture(case, golden_dir):
    from unicorn_amd.ops import msda_forward
    shapes, t, _ = _load(golden_dir, case)
    shp, lsi = _lsi(shapes)
    out = msda_forward(t["value"].double().cuda(), shp, lsi, t["loc"].double().cuda(), t["attn"].double().cuda())
    err = _relmax(out, t["out"])
    print("fp64 forward case %s: rel-to-max err %.3e" % (case, err))
    assert out.dtype == torch.float64 and err <= 1e-12


def test_dtype_rules():
    from unicorn_amd import _lib
    from unicorn_amd.ops import msda_backward, msda_forward
    shapes = [(6, 4), (3, 2)]
    shp, lsi = _lsi(shapes)
    value, loc, attn, gout = (t.cuda() for t in _random_problem(0, 1, shapes, 2, 4, 2, 2, 0.0, 1.0))
    with pytest.raises(_lib.UnicornHipError):
        msda_forward(value.double(), shp, lsi, loc, attn)
    with pytest.raises(_lib.UnicornHipError):
        msda_backward(value, shp, lsi, loc, attn, gout.double())
    with pytest.raises(_lib.UnicornHipError):
        msda_backward(value.half(), shp, lsi, loc.half(), attn.half(), gout.half())
    with pytest.raises(_lib.UnicornHipError):                                  # a level that lies outside value must not be scattered into
        msda_backward(value, shp, torch.tensor([0, 25]), loc, attn, gout)


# ---------------------------------------------------------------------------------------------------- 3: gradcheck + the large D
def _test_py_problem(D, seed):
    """the shapes and value / weight recipe of the reference's ops/test.py:21-36,63-69, locations made lattice-safe"""
    shapes = [(6, 4), (3, 2)]
    g = torch.Generator().manual_seed(seed)
    value = torch.rand(1, 30, 2, D, generator=g) * 0.01
    loc = GEN.make_lattice_safe(torch.rand(1, 2, 2, 2, 2, 2, generator=g), shapes)
    attn = torch.rand(1, 2, 2, 2, 2, generator=g) + 1e-5
    attn /= attn.sum(-1, keepdim=True).sum(-2, keepdim=True)
    assert GEN.lattice_ok(loc, shapes)
    return shapes, value, loc, attn


@pytest.mark.parametrize("D", [30, 32, 64, 71])
def test_gradcheck_double(D):
    """torch.autograd.gradcheck as in ops/test.py:63-78.  nondet_tol: each grad_value destination receives at most 4 addends of
    magnitude <= 1, so reordering moves it by <= 4 * 4 * 2^-53 < 1e-14; gradcheck's eps 1e-6 stays inside the 1e-3 lattice margin."""
    from unicorn_amd.ops import MSDeformAttnFunction
    shapes, value, loc, attn = _test_py_problem(D, 3)
    shp, lsi = _lsi(shapes)
    v, l, a = (t.double().cuda().requires_grad_(True) for t in (value, loc, attn))
    assert torch.autograd.gradcheck(MSDeformAttnFunction.apply, (v, shp.cuda(), lsi.cuda(), l, a, 2), nondet_tol=1e-14)


@pytest.mark.parametrize("D", [1025, 2048, 3096])
def test_large_channel_counts_fp64(D):
    """The rest of ops/test.py:85's list: a gradcheck Jacobian at D=3096 is ~18 GB, so the HIP fp64 gradients are held to msda_core's
    fp64 autograd instead (1e-12 x max)."""
    shapes, value, loc, attn = _test_py_problem(D, 4)
    gout = torch.randn(1, 2, 2 * D, generator=torch.Generator().manual_seed(5))
    got = _hip_grads(torch.float64, shapes, value, loc, attn, gout)
    want = _oracle_grads(torch.float64, shapes, value, loc, attn, gout)
    for name, g, w in zip(("out",) + NAMES, got, want):
        err = _relmax(g, w)
        print("D=%d %s: rel-to-max err %.3e" % (D, name, err))
        assert err <= 1e-12, name


def test_d32_odd_sample_count_fp64():
    """D == 32 path with an odd L*P (the upper half-wave idles in the last step) and a task count that is no multiple of 4."""
    shapes = [(5, 7), (3, 4), (2, 2)]
    value, loc, attn, gout = _random_problem(11, 3, shapes, 3, 32, 7, 3, -0.3, 1.3)
    got = _hip_grads(torch.float64, shapes, value, loc, attn, gout)
    want = _oracle_grads(torch.float64, shapes, value, loc, attn, gout)
    for name, g, w in zip(("out",) + NAMES, got, want):
        assert _relmax(g, w) <= 1e-12, name


# ---------------------------------------------------------------------------------------------------- 4: Unicorn geometry
@pytest.fixture(scope="module")
def unicorn_problem():
    shapes = [(50, 80), (50, 80)]
    prob = _random_problem(21, 2, shapes, 8, 32, 8000, 4, -0.05, 1.05)
    want64 = _oracle_grads(torch.float64, shapes, *prob)[1:]
    want32 = _oracle_grads(torch.float32, shapes, *prob)[1:]
    return shapes, prob, want64, want32


def test_unicorn_geometry_fp64(unicorn_problem):
    shapes, prob, want64, _ = unicorn_problem
    got = _hip_grads(torch.float64, shapes, *prob)[1:]
    errs = [_relmax(g, w) for g, w in zip(got, want64)]
    print("unicorn geometry fp64: rel-to-max err %s (bound 1e-12)" % ["%.3e" % e for e in errs])
    for name, e in zip(NAMES, errs):
        assert e <= 1e-12, name


def test_unicorn_geometry_fp32(unicorn_problem):
    """D == 32 fast path, heavy collisions in grad_value, N > 1.  Yardstick: msda_core's own fp32-vs-fp64 error on the same inputs."""
    shapes, prob, want64, want32 = unicorn_problem
    got = _hip_grads(torch.float32, shapes, *prob)[1:]
    for name, g, w64, w32 in zip(NAMES, got, want64, want32):
        e, r = _relmax(g, w64), _relmax(w32, w64)
        print("unicorn geometry fp32 %s: rel-to-max err %.3e, msda_core fp32 err %.3e, ratio %.2f (bound 4)" % (name, e, r, e / r))
    for name, g, w64, w32 in zip(NAMES, got, want64, want32):
        assert _relmax(g, w64) <= 4 * _relmax(w32, w64), name


# ---------------------------------------------------------------------------------------------------- 5, 6, 7
def test_partial_requires_grad(golden_dir):
    from unicorn_amd.ops import MSDeformAttnFunction
    shapes, t, _ = _load(golden_dir, "b")
    shp, lsi = _lsi(shapes)
    for which, name in ((0, "grad_value"), (1, "grad_loc")):
        ins = [t[k].double().cuda() for k in ("value", "loc", "attn")]
        ins[which].requires_grad_(True)
        out = MSDeformAttnFunction.apply(ins[0], shp.cuda(), lsi.cuda(), ins[1], ins[2], 64)
        out.backward(t["grad_out"].double().cuda())
        assert _relmax(ins[which].grad, t[name]) <= 1e-12
        assert all(ins[i].grad is None for i in range(3) if i != which)
    # torch.autograd.grad for one input while all three require grad: the unused gradients are dropped without error
    ins = [t[k].double().cuda().requires_grad_(True) for k in ("value", "loc", "attn")]
    out = MSDeformAttnFunction.apply(ins[0], shp.cuda(), lsi.cuda(), ins[1], ins[2], 64)
    (gl,) = torch.autograd.grad(out, ins[1], t["grad_out"].double().cuda())
    assert _relmax(gl, t["grad_loc"]) <= 1e-12


def test_noncontiguous_grad_output(golden_dir):
    from unicorn_amd.ops import MSDeformAttnFunction, msda_backward
    shapes, t, _ = _load(golden_dir, "b")
    shp, lsi = _lsi(shapes)
    gc = t["grad_out"].double().cuda()
    gnc = gc.transpose(1, 2).contiguous().transpose(1, 2)                       # same values, (N, M*D, Lq) memory
    assert not gnc.is_contiguous() and torch.equal(gnc, gc)
    res = []
    for g in (gc, gnc):
        ins = [t[k].double().cuda().requires_grad_(True) for k in ("value", "loc", "attn")]
        MSDeformAttnFunction.apply(ins[0], shp.cuda(), lsi.cuda(), ins[1], ins[2], 64).backward(g)
        res.append([i.grad for i in ins])
    direct = msda_backward(t["value"].double().cuda(), shp, lsi, t["loc"].double().cuda(), t["attn"].double().cuda(), gnc)
    for other in (res[1], direct):
        assert _relmax(other[0], res[0][0].cpu()) <= 1e-12                      # grad_value: float atomics, arrival order in the last bits
        assert torch.equal(other[1], res[0][1]) and torch.equal(other[2], res[0][2])   # one writer per element: bitwise
    assert _relmax(res[1][0], t["grad_value"]) <= 1e-12


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_no_queries(dtype):
    from unicorn_amd.ops import msda_backward
    shapes = [(6, 4), (3, 2)]
    shp, lsi = _lsi(shapes)
    value = torch.randn(2, 30, 2, 32, dtype=dtype).cuda()
    loc = torch.rand(2, 0, 2, 2, 2, 2, dtype=dtype).cuda()
    attn = torch.rand(2, 0, 2, 2, 2, dtype=dtype).cuda()
    gv, gl, ga = msda_backward(value, shp, lsi, loc, attn, torch.zeros(2, 0, 64, dtype=dtype).cuda())
    assert gv.shape == value.shape and gv.dtype == dtype and not gv.any()
    assert gl.shape == loc.shape and ga.shape == attn.shape and gl.numel() == 0 and ga.numel() == 0
    # the C entry itself with Lq = 0 (a host passes buffers of its own for the empty arrays): returns 0 with grad_value zeroed
    import ctypes as C
    from unicorn_amd import _lib
    dummy, gv2 = torch.zeros(4, dtype=dtype).cuda(), torch.ones_like(value)
    fn = getattr(_lib.lib(), "uni_msda_bwd" if dtype == torch.float32 else "uni_msda_bwd_f64")
    rc = fn(_lib.ptr(value), (C.c_int64 * 4)(6, 4, 3, 2), (C.c_int64 * 2)(0, 24), _lib.ptr(dummy), _lib.ptr(dummy), _lib.ptr(dummy),
            _lib.ptr(gv2), _lib.ptr(dummy), _lib.ptr(dummy), 2, 30, 2, 32, 0, 2, 2, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and not gv2.any() and not dummy.any()


# ---------------------------------------------------------------------------------------------------- 9: as a layer
class TinyDeformAttn(nn.Module):
    """value / offset / attention projections around the sampler (what ops/modules/ms_deform_attn.py:78-115 does, restated):
    softmax over L*P, loc = reference point + offset / (W, H).  `core` selects the sampler: "hip" (MSDeformAttnFunction) or "oracle"."""

    def __init__(self, d_model, M, L, P):
        super().__init__()
        self.M, self.L, self.P = M, L, P
        self.value_proj = nn.Linear(d_model, d_model)
        self.sampling_offsets = nn.Linear(d_model, M * L * P * 2)
        self.attention_weights = nn.Linear(d_model, M * L * P)

    def locations(self, query, ref_pts, shapes):
        N, Lq, _ = query.shape
        off = self.sampling_offsets(query).view(N, Lq, self.M, self.L, self.P, 2)
        norm = torch.tensor([[w, h] for (h, w) in shapes], dtype=query.dtype, device=query.device)
        return ref_pts[:, :, None, :, None, :] + off / norm[None, None, None, :, None, :]

    def forward(self, query, ref_pts, src, shapes, core):
        N, Lq, C = query.shape
        value = self.value_proj(src).view(N, -1, self.M, C // self.M)
        aw = F.softmax(self.attention_weights(query).view(N, Lq, self.M, self.L * self.P), -1).view(N, Lq, self.M, self.L, self.P)
        loc = self.locations(query, ref_pts, shapes)
        if core == "hip":
            from unicorn_amd.ops import MSDeformAttnFunction
            shp, lsi = _lsi(shapes)
            return MSDeformAttnFunction.apply(value, shp.to(query.device), lsi.to(query.device), loc, aw, 64)
        import unicorn_oracle as uo
        return uo.msda_core(value, shapes, loc, aw)


def test_layer_parameter_gradients():
    """Parameter gradients of the layer on the GPU (fp32, HIP sampler) against the same layer on the CPU with msda_core in fp64; bound
    per parameter: 4 x the error the CPU layer in fp32 shows against its own fp64 run.  The reference points are a pixel-centre grid,
    moved per (query, level, coordinate) by 0.37 pixel where needed so that the locations the initial parameters produce are
    lattice-safe."""
    torch.manual_seed(7)
    shapes, M, P, C, N = [(10, 16), (10, 16)], 8, 4, 256, 2
    L, hw = len(shapes), 160
    Lq = S = L * hw
    layer = TinyDeformAttn(C, M, L, P)
    with torch.no_grad():
        layer.sampling_offsets.bias.uniform_(-3.0, 3.0)                         # offsets of a few pixels, some samples leave the map
    src = torch.randn(N, S, C)
    query = src + 0.5 * torch.randn(N, Lq, C)
    gout = torch.randn(N, Lq, C)
    ys, xs = torch.meshgrid(torch.arange(10.0) + 0.5, torch.arange(16.0) + 0.5, indexing="ij")
    grid = torch.stack((xs.reshape(-1) / 16, ys.reshape(-1) / 10), -1)          # (hw, 2) pixel centres
    ref_pts = grid.repeat(L, 1)[None, :, None, :].repeat(N, 1, L, 1).contiguous()   # (N, Lq, L, 2)
    norm = torch.tensor([[w, h] for (h, w) in shapes], dtype=torch.float64)[None, None, :, :]
    l64 = TinyDeformAttn(C, M, L, P).double()
    l64.load_state_dict(layer.state_dict())
    for _ in range(32):
        with torch.no_grad():
            loc = l64.locations(query.double(), ref_pts.double(), shapes)
        bad = GEN.lattice_bad(loc, shapes).any(4).any(2)                        # (N, Lq, L, 2)
        if not bad.any():
            break
        ref_pts = torch.where(bad, (ref_pts.double() + 0.37 / norm).float(), ref_pts)
    with torch.no_grad():
        assert GEN.lattice_ok(l64.locations(query.double(), ref_pts.double(), shapes), shapes)

    def run(mod, dtype, device, core):
        mod.zero_grad()
        out = mod(query.to(dtype).to(device), ref_pts.to(dtype).to(device), src.to(dtype).to(device), shapes, core)
        out.backward(gout.to(dtype).to(device))
        return {k: p.grad.detach().double().cpu() for k, p in mod.named_parameters()}

    g64 = run(l64, torch.float64, "cpu", "oracle")
    g32 = run(layer, torch.float32, "cpu", "oracle")
    gpu = TinyDeformAttn(C, M, L, P)
    gpu.load_state_dict(layer.state_dict())
    ghip = run(gpu.cuda(), torch.float32, "cuda", "hip")
    torch.cuda.synchronize()
    errs = {k: (_relmax(ghip[k], g64[k]), _relmax(g32[k], g64[k])) for k in g64}
    for k, (e, r) in errs.items():
        print("layer %s: GPU fp32 err %.3e, CPU fp32 err %.3e, ratio %.2f (bound 4)" % (k, e, r, e / r))
    assert len(errs) == 6
    for k, (e, r) in errs.items():
        assert float(g64[k].abs().max()) > 0 and e <= 4 * r, k
