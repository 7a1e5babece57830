"""The differentiable depthwise 7x7 + LayerNorm operator on the GPU (ops.dwconv7_ln, csrc/dwln_train.hip): the fixtures written from the
reference's own Block in fp64 (1e-12) and fp32 (4 x the reference's own fp32 deviation), gradcheck, bitwise reproducibility, shapes that need
several blocks per reduction, zero variance, every subset of the need flags with the variant trace, what autograd keeps, autocast, the two
layouts of x, and a fused stand-in block under FusedAdamWEMA."""
import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dwln_train_ref as R  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
CL = torch.channels_last


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def run_op(ins, dtype, need=(True,) * 5, layout=CL, eps=R.EPS):
    """ops.dwconv7_ln + backward on the device -> {y, gx, gw, gb, ggamma, gbeta} (None where not needed)"""
    from unicorn_amd.ops import dwconv7_ln
    x = ins[0].to(DEV, dtype).contiguous(memory_format=layout)
    leaves = [x] + [t.to(DEV, dtype) for t in ins[1:5]]
    for t, n in zip(leaves, need):
        t.requires_grad_(bool(n))
    y = dwconv7_ln(*leaves, eps=eps)
    assert y.is_contiguous() and y.dtype == dtype and tuple(y.shape) == (x.shape[0], x.shape[2], x.shape[3], x.shape[1])
    if any(need):
        y.backward(ins[5].to(DEV, dtype))
    torch.cuda.synchronize()
    return dict(zip(R.RESULTS, [y.detach()] + [t.grad for t in leaves]))


def fixture_inputs(c):
    return [torch.from_numpy(c[n]) for n in R.INPUTS]


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp64_matches_the_fixture(L, tag):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float64)
    for n in R.RESULTS:
        err = R.rel_err(got[n], torch.from_numpy(c[n]))
        print("%s fp64 %-6s err %.3e" % (tag, n, err))
        assert got[n].shape == c[n].shape and err <= 1e-12, (n, err)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp32_within_four_times_the_reference_fp32_deviation(L, tag):
    c = R.load_case(tag)
    got = run_op(fixture_inputs(c), torch.float32)
    ratios = {}
    for n in R.RESULTS:
        err, bound = R.rel_err(got[n], torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
        ratios[n] = err / bound
        print("%s fp32 %-6s err %.3e  bound %.3e  ratio %.3f" % (tag, n, err, bound, ratios[n]))
    assert max(ratios.values()) <= 1.0, ratios


@pytest.mark.parametrize("shape", [None, (2, 8, 4, 9)])
def test_gradcheck_fp64(L, shape):
    from unicorn_amd.ops import dwconv7_ln
    ins = R.draw("small", 7, shape)
    leaves = [ins[0].to(DEV, torch.float64).contiguous(memory_format=CL).requires_grad_(True)]
    leaves += [t.to(DEV, torch.float64).requires_grad_(True) for t in ins[1:5]]
    assert torch.autograd.gradcheck(lambda *a: dwconv7_ln(*a), leaves, nondet_tol=0.0)


# ------------------------------------------------------------------------------------------------ shapes with several blocks per reduction
# the issue's three shapes, plus two that reach the paths the small ones do not
LARGE = [(2, 384, 23, 37), (1, 768, 10, 10), (2, 192, 40, 50), (1, 4, 96, 700), (1, 260, 32, 260)]


@functools.lru_cache(maxsize=None)
def large_case(shape):
    """inputs, the restatement on the CPU in fp64, and its own deviation in fp32 (computed once per shape, shared, never modified)"""
    ins = R.draw("plain", sum(shape), shape)
    ref = R.value_and_grads(*(t.double() for t in ins))
    f32 = R.value_and_grads(*ins)
    return ins, ref, {n: R.rel_err(f32[n], ref[n]) for n in R.RESULTS}


@pytest.mark.parametrize("shape", LARGE)
def test_larger_shapes_against_the_restatement(L, shape):
    """A block of the forward, of pass A and of the data pass takes NS strips of 8 pixels (2 in fp64) of one row, NS = 512 / (64 ceil(C / 256))
    strips at once, and pass A runs at most 1024 blocks, each of which writes one row of dgamma / dbeta partials; a wave of the weight pass
    walks a strip of ceil(W / ceil(W / 128)) pixels of one row and four waves make a block, one row of dw / db partials.
      (2, 384, 23, 37)   5 strips per row, the last of 5 pixels; NS = 4: 58 blocks in pass A; weight pass 46 strips of 37: 12 blocks, the last half full
      (1, 768, 10, 10)   2 strips per row, the last of 2 pixels; NS = 2, three waves per strip: 10 blocks; weight pass 10 strips: 3 blocks, the last half full
      (2, 192, 40, 50)   7 strips per row, the last of 2 pixels; NS = 8: 70 blocks; weight pass 80 strips: 20 blocks
      (1, 4, 96, 700)    88 strips per row, the last of 4 pixels; 8448 strips in 1056 groups of 8: more than the 1024 blocks of pass A, so blocks take a
                         second group; W > 128: six weight-pass strips of 117 per row, the last of 115
      (1, 260, 32, 260)  two waves per strip; in fp64 130 strips per row, 4160 in 1040 groups of 4: the second-group path with the LDS sums
    fp32 bound: 4 x the deviation of the same restatement in fp32 on the CPU; the fp64 run is held to 1e-12."""
    ins, ref, dev = large_case(shape)
    got = run_op(ins, torch.float32)
    ratios = {n: R.rel_err(got[n], ref[n]) / (4 * dev[n]) for n in R.RESULTS}
    print("%s fp32 err / bound: %s" % (shape, ", ".join("%s %.3f" % kv for kv in ratios.items())))
    got64 = run_op(ins, torch.float64)
    err64 = {n: R.rel_err(got64[n], ref[n]) for n in R.RESULTS}
    print("%s fp64 err: %s" % (shape, ", ".join("%s %.2e" % kv for kv in err64.items())))
    assert max(ratios.values()) <= 1.0, ratios
    assert max(err64.values()) <= 1e-12, err64


@pytest.mark.parametrize("shape", [R.CASES["c96"], (2, 192, 40, 50)])
def test_two_runs_are_bitwise_equal(L, shape):
    ins = R.draw("plain", 11, shape)
    a, b = run_op(ins, torch.float32), run_op(ins, torch.float32)
    for n in R.RESULTS:
        assert torch.equal(a[n], b[n]), n


def test_zero_variance(L):
    """x = 0 and a constant bias: every pixel has u = 0.5 in all 64 channels, variance 0, rstd = 1000; y is ln_bias exactly"""
    shape = (1, 64, 5, 6)
    ins = list(R.draw("plain", 3, shape))
    ins[0] = torch.zeros_like(ins[0])
    ins[2] = torch.full_like(ins[2], 0.5)
    got = run_op(ins, torch.float32)
    assert torch.equal(got["y"].cpu(), ins[4].expand(1, 5, 6, 64))
    ref = R.value_and_grads(*(t.double() for t in ins))
    f32 = R.value_and_grads(*ins)
    for n in R.RESULTS[1:]:
        assert torch.isfinite(got[n]).all(), n
        if float(ref[n].abs().max()) == 0.0:            # gw, ggamma: sums of exact zeros
            assert not got[n].any(), n
            continue
        err, bound = R.rel_err(got[n], ref[n]), 4 * R.rel_err(f32[n], ref[n])
        print("zero variance %-6s err %.3e bound %.3e" % (n, err, bound))
        assert err <= bound, (n, err, bound)


# ------------------------------------------------------------------------------------------------ need flags
@pytest.mark.parametrize("need_x,need_w,need_g", [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1) if a or b or c])
def test_need_flags(L, need_x, need_w, need_g):
    ins = fixture_inputs(R.load_case("c96"))
    full = run_op(ins, torch.float32)
    need = (need_x, need_w, need_w, need_g, need_g)
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        got = run_op(ins, torch.float32, need)
    finally:
        lib.uni_variant_trace(0)
    tags = vc.read_trace(lib)
    for n, k in zip(R.RESULTS[1:], need):
        if k:
            assert torch.equal(got[n], full[n]), n
        else:
            assert got[n] is None, n
    assert torch.equal(got["y"], full["y"])
    count = lambda key: sum(v for t, v in tags.items() if t.startswith("dwln_train " + key))        # noqa: E731
    assert count("fwd<f32") == 1 and count("bwd_a<f32") == 1, tags
    assert count("bwd_dx") == need_x and count("bwd_dw") == need_w and count("reduce") == (1 if need_w or need_g else 0), tags
    a_tag = [t for t in tags if t.startswith("dwln_train bwd_a")][0]
    assert ("du=%d gb=%d" % (1 if need_x or need_w else 0, need_g)) in a_tag, tags
    assert sum(tags.values()) == 2 + need_x + need_w + (1 if need_w or need_g else 0), tags


def test_autograd_keeps_x_and_no_second_map(L):
    from unicorn_amd.ops import dwconv7_ln
    B, C, H, W = R.CASES["c100"]
    ins = fixture_inputs(R.load_case("c100"))
    leaves = [ins[0].to(DEV).contiguous(memory_format=CL).requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in ins[1:5]]
    y = dwconv7_ln(*leaves)
    saved = y.grad_fn.saved_tensors
    maps = [t for t in saved if t.numel() == B * H * W * C]
    assert len(maps) == 1 and maps[0].data_ptr() == leaves[0].data_ptr()
    assert sorted(t.numel() for t in saved) == sorted([B * H * W * C, 49 * C, C, C, C, 2 * B * H * W])


def test_autocast_half_input(L):
    from unicorn_amd.ops import dwconv7_ln
    ins = fixture_inputs(R.load_case("c96"))
    xh = ins[0].to(DEV).half().contiguous(memory_format=CL)
    ref = run_op([xh.float().cpu()] + ins[1:], torch.float32)
    leaves = [xh.clone().requires_grad_(True)] + [t.to(DEV).requires_grad_(True) for t in ins[1:5]]
    with torch.autocast("cuda", torch.float16):
        y = dwconv7_ln(*leaves)
        eager = F.layer_norm(F.conv2d(leaves[0], *leaves[1:3], padding=3, groups=xh.shape[1]).permute(0, 2, 3, 1), (xh.shape[1],), *leaves[3:5], R.EPS)
    assert y.dtype == eager.dtype == torch.float32 and torch.equal(y, ref["y"])
    y.backward(ins[5].to(DEV))
    assert leaves[0].grad.dtype == torch.float16 and torch.equal(leaves[0].grad, ref["gx"].half())
    for t, n in zip(leaves[1:], R.RESULTS[2:]):
        assert t.grad.dtype == torch.float32 and torch.equal(t.grad, ref[n]), n


def test_nchw_contiguous_x_gives_the_same_values(L):
    ins = fixture_inputs(R.load_case("c100"))
    a, b = run_op(ins, torch.float32, layout=CL), run_op(ins, torch.float32, layout=torch.contiguous_format)
    for n in R.RESULTS:
        assert torch.equal(a[n], b[n]), n


def test_empty_batch(L):
    from unicorn_amd.ops import dwconv7_ln
    ins = R.draw("plain", 1, (1, 8, 3, 3))
    y = dwconv7_ln(torch.zeros(0, 8, 3, 3, device=DEV), *(t.to(DEV) for t in ins[1:5]))
    assert tuple(y.shape) == (0, 3, 3, 8)


# ------------------------------------------------------------------------------------------------ a fused block under FusedAdamWEMA
class StandInBlock(nn.Module):
    def __init__(self, C):
        super().__init__()
        self.dwconv = nn.Conv2d(C, C, kernel_size=7, padding=3, groups=C)
        self.norm = nn.LayerNorm(C, eps=1e-6)
        self.pw = nn.Linear(C, C)

    def forward(self, x):
        y = self.norm(self.dwconv(x).permute(0, 2, 3, 1))
        return x + self.pw(y).permute(0, 3, 1, 2)


def test_fused_block_trains_like_the_unfused_one(L):
    """Two FusedAdamWEMA steps of a stand-in block, fused and unfused on the GPU, against torch.optim.AdamW on the CPU in fp64; the bound of every
    parameter is 4 x the deviation of the same two steps in fp32 on the CPU."""
    from unicorn_amd import optim
    from unicorn_amd.nn import fuse_dwconv_ln
    torch.manual_seed(5)
    C = 16
    proto = StandInBlock(C)
    with torch.no_grad():
        proto.dwconv.bias.normal_(0, 0.1), proto.norm.weight.normal_(1, 0.1), proto.norm.bias.normal_(0, 0.1)
    xs = [torch.randn(2, C, 6, 7) for _ in range(2)]
    ts = [torch.randn(2, C, 6, 7) for _ in range(2)]
    kw = dict(lr=1e-2, weight_decay=5e-4)

    def cpu_run(dtype):
        net = copy.deepcopy(proto).to(dtype)
        opt = torch.optim.AdamW(net.parameters(), foreach=False, **kw)
        for x, t in zip(xs, ts):
            opt.zero_grad()
            (net(x.to(dtype)) * t.to(dtype)).sum().backward()
            opt.step()
        return [p.detach() for p in net.parameters()]

    def gpu_run(fuse):
        net = copy.deepcopy(proto).to(DEV).train()
        if fuse:
            assert fuse_dwconv_ln(net) == 1
        ema = copy.deepcopy(net).eval()
        opt = optim.FusedAdamWEMA(net, ema, ema_decay=0.9998, **kw)
        for x, t in zip(xs, ts):
            opt.zero_grad()
            (net(x.to(DEV)) * t.to(DEV)).sum().backward()
            opt.step()
        torch.cuda.synchronize()
        return [p.detach() for p in net.parameters()], [p.detach() for p in ema.parameters()]

    exp, ref32 = cpu_run(torch.float64), cpu_run(torch.float32)
    (fused, fused_ema), (plain, plain_ema) = gpu_run(True), gpu_run(False)
    names = [n for n, _ in proto.named_parameters()]
    bounds = {}
    for n, e, r, f, p in zip(names, exp, ref32, fused, plain):
        bound = bounds[n] = 4 * R.rel_err(r, e)
        print("%-14s fused %.3e  unfused %.3e  bound %.3e" % (n, R.rel_err(f, e), R.rel_err(p, e), bound))
        assert R.rel_err(f, e) <= bound and R.rel_err(p, e) <= bound, n
    # the EMA copy (a deep copy of the fused model) was driven too; an average of parameters that are each within `bound` of the exact ones
    for n, f, p, start in zip(names, fused_ema, plain_ema, proto.parameters()):
        assert not torch.equal(f.cpu(), start.detach()) and R.rel_err(f, p) <= 2 * bounds[n], n
