"""GPU checks of the differentiable label propagation, through the public surface only (ops.propagate_labels, ops.CorrSoftmaxPVFunction,
ops.corr_softmax_pv_lse): the fp64 path against the fixture of the reference's own lines, the fp32 kernels against the same fixture with the
bound of tests/test_msda_backward_gpu.py (4 x the error of an fp32 evaluation of the same lines: another summation order and FMA
contraction, never a figure taken from the kernel), gradcheck, the unchanged forward, the headline geometry with its memory condition."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("flat", "ragged", "peaky", "batch")
GRADS = ("g_embed_0", "g_embed_1", "g_labels")


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "corr_backward_%s.npz" % tag)))


def relerr(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref.cpu()).abs().max() / ref.abs().max())


def three_lines(embed_0, embed_1, labels):
    """what unicorn.py:321-322 and the product of :326 compute, stated in torch: maps (B, C, HW) or (B, C, H, W), labels (B, K, HW_0)"""
    scores = embed_0.flatten(2).transpose(1, 2) @ embed_1.flatten(2)          # (B, HW_0, HW_1)
    return labels @ torch.softmax(scores, dim=1)


def run_op(e0, e1, lb, g, precision=0, need=(True, True, True)):
    """forward + backward through ops.propagate_labels on device tensors -> out, (grads)"""
    from unicorn_amd import ops
    e0 = e0.detach().clone().requires_grad_(need[0])
    e1 = e1.detach().clone().requires_grad_(need[1])
    lb = lb.detach().clone().requires_grad_(need[2])
    out = ops.propagate_labels(e0, e1, lb, precision)
    out.backward(g)
    return out.detach(), (e0.grad, e1.grad, lb.grad)


def dev_inputs(c, dtype):
    return [torch.from_numpy(c[n]).to("cuda", dtype) for n in ("embed_0", "embed_1", "labels", "grad_out")]


@pytest.mark.parametrize("tag", CASES)
def test_fp64_path_equals_the_fixture(tag):
    from unicorn_amd import ops
    c = load_case(tag)
    e0, e1, lb, g = dev_inputs(c, torch.float64)
    out, grads = run_op(e0, e1, lb, g)
    _, lse = ops.corr_softmax_pv_lse(e0.transpose(1, 2), e1.transpose(1, 2), lb)
    got = dict(zip(GRADS, grads), out=out, lse=lse)
    for n, t in got.items():
        err = relerr(t, torch.from_numpy(c[n]))
        print("fp64 %-7s %-10s err %.3g" % (tag, n, err))
        assert err <= 1e-12, (tag, n, err)


@pytest.mark.parametrize("tag", CASES)
def test_fp32_precision0_against_the_fixture(tag):
    from unicorn_amd import ops
    c = load_case(tag)
    e0, e1, lb, g = dev_inputs(c, torch.float32)
    out, grads = run_op(e0, e1, lb, g, precision=0)
    out2, lse = ops.corr_softmax_pv_lse(e0.transpose(1, 2), e1.transpose(1, 2), lb, precision=0)
    assert torch.equal(out, out2)
    bad = []
    for n, t in zip(GRADS, grads):
        err, bound = relerr(t, torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
        print("fp32 %-7s %-10s err %.3g  fp32_ref_err %.3g  ratio %.2f (bound 4)" % (tag, n, err, bound / 4, 4 * err / bound))
        if not err <= bound:
            bad.append((n, err, bound))
    for n, t in (("out", out), ("lse", lse)):                    # the existing forward's bar (test_kernels_gpu.py::test_corr_softmax_pv)
        ref = torch.from_numpy(c[n])
        d, bar = float((t.double().cpu() - ref).abs().max()), 2e-5 * max(1.0, float(ref.abs().max()))
        print("fp32 %-7s %-10s max|diff| %.3g  bar %.3g  ratio %.3f" % (tag, n, d, bar, d / bar))
        if not d < bar:
            bad.append((n, d, bar))
    assert not bad, bad


@pytest.mark.parametrize("R,Q,K", [(33, 64, 1), (97, 33, 3), (64, 97, 3)])
def test_gradcheck_fp64(R, Q, K):
    from unicorn_amd import ops
    g = torch.Generator().manual_seed(R * 1000 + Q)
    e0 = (0.4 * torch.randn(1, R, 128, generator=g, dtype=torch.float64)).cuda().requires_grad_(True)
    e1 = (0.4 * torch.randn(1, Q, 128, generator=g, dtype=torch.float64)).cuda().requires_grad_(True)
    lb = torch.rand(1, K, R, generator=g, dtype=torch.float64).cuda().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda a, b, c: ops.CorrSoftmaxPVFunction.apply(a, b, c, 0), (e0, e1, lb))      # nondet_tol = 0


@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("per_frame", [False, True])
def test_lse_forward_is_bitwise_the_existing_forward(precision, K, per_frame):
    from unicorn_amd import ops
    g = torch.Generator().manual_seed(7 + K)
    B, R, Q = 3, 700, 530
    er = torch.randn(B, 128, R, generator=g).cuda()
    ec = torch.randn(B, 128, Q, generator=g).cuda()
    v = (torch.rand(B, K, R, generator=g) if per_frame else torch.rand(K, R, generator=g)).cuda()
    ref = ops.corr_softmax_pv_batched(er, ec, v, precision=precision, values_per_frame=per_frame)
    out, lse = ops.corr_softmax_pv_lse(er.transpose(1, 2), ec.transpose(1, 2), v, precision=precision)
    assert torch.equal(out, ref)
    want = torch.logsumexp(torch.bmm(er.double().transpose(1, 2), ec.double()), dim=1)
    assert float((lse.double() - want).abs().max()) < 2e-5 * max(1.0, float(want.abs().max()))


def _chunked_reference(e0, e1, lb, g, dtype, chunk=2000):
    """the three lines under autograd on the CPU, chunked over query columns (columns are independent): e0 (1,C,R), e1 (1,C,Q)"""
    e0 = e0.detach().clone().to(dtype).requires_grad_(True)
    lb = lb.detach().clone().to(dtype).requires_grad_(True)
    e1 = e1.detach().to(dtype)
    outs, lses, g1 = [], [], []
    for q0 in range(0, e1.shape[2], chunk):
        c1 = e1[:, :, q0:q0 + chunk].clone().requires_grad_(True)
        simi = torch.bmm(e0.transpose(1, 2), c1)
        out = torch.bmm(lb, torch.softmax(simi, dim=1))
        out.backward(g[:, :, q0:q0 + chunk].to(dtype))
        outs.append(out.detach())
        lses.append(torch.logsumexp(simi.detach(), dim=1))
        g1.append(c1.grad)
    return {"out": torch.cat(outs, 2), "lse": torch.cat(lses, 1), "g_embed_0": e0.grad, "g_embed_1": torch.cat(g1, 2), "g_labels": lb.grad}


def test_headline_geometry_accuracy_and_memory():
    """R = Q = 16000 (800 x 1280 at stride 8), K = 1, fp32: gradients within 4 x the error of an fp32 evaluation of the same lines on the
    CPU (both against fp64), out / lse within the forward's bar, and forward + backward in less than a quarter of ONE R x Q fp32 matrix."""
    from unicorn_amd import ops
    gen = torch.Generator().manual_seed(11)
    R = Q = 16000
    e0 = 0.3 * torch.randn(1, 128, R, generator=gen)
    e1 = 0.3 * torch.randn(1, 128, Q, generator=gen)
    lb = torch.rand(1, 1, R, generator=gen)
    g = torch.randn(1, 1, Q, generator=gen)
    ref = _chunked_reference(e0, e1, lb, g, torch.float64)
    f32 = _chunked_reference(e0, e1, lb, g, torch.float32)
    d0, d1, dl, dg = e0.cuda(), e1.cuda(), lb.cuda(), g.cuda()
    out, _ = run_op(d0[:, :, :256], d1[:, :, :256], dl[:, :, :256], dg[:, :, :256])       # library, LDS opt-in, allocator warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out, grads = run_op(d0, d1, dl, dg)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("headline: peak memory rise over forward + backward %.1f MB" % (rise / 2 ** 20))
    _, lse = ops.corr_softmax_pv_lse(d0.transpose(1, 2), d1.transpose(1, 2), dl)
    bad = []
    for n, t in zip(GRADS, grads):
        err, own = relerr(t, ref[n]), relerr(f32[n], ref[n])
        print("headline %-10s err %.3g  fp32 CPU err %.3g  ratio %.2f (bound 4)" % (n, err, own, err / own))
        if not err <= 4 * own:
            bad.append((n, err, own))
    for n, t in (("out", out), ("lse", lse)):
        d, bar = float((t.double().cpu() - ref[n]).abs().max()), 2e-5 * max(1.0, float(ref[n].abs().max()))
        print("headline %-10s max|diff| %.3g  bar %.3g" % (n, d, bar))
        if not d < bar:
            bad.append((n, d, bar))
    assert not bad, bad
    assert rise < 256 * 2 ** 20, "forward + backward allocated %.1f MB: the R x Q matrix (1024 MB) or a per-split slab was materialised" % (rise / 2 ** 20)


def _small(B, R, Q, K, seed, scale=0.4):
    g = torch.Generator().manual_seed(seed)
    return ((scale * torch.randn(B, 128, R, generator=g)).cuda(), (scale * torch.randn(B, 128, Q, generator=g)).cuda(),
            torch.rand(B, K, R, generator=g).cuda(), torch.randn(B, K, Q, generator=g).cuda())


def _check_against_torch(e0, e1, lb, g, what):
    """fp32 operator against the three lines in fp64 on the CPU.  Bound: 4 x the error of the three lines in fp32 on the CPU (the bound of the
    fixture test).  On these deliberately tiny problems the maximum over a few hundred elements is a noisy estimate of that error, and the
    three gradients are contractions of ONE recomputed P, so they share an error class: the yardstick of a gradient is the largest of the
    three gradients' fp32 errors.  (With a per-tensor yardstick g_labels of R = 300, Q = 11, K = 2 -- 600 elements, 11-term sums -- measured
    1.24e-6 against 2.93e-7, 4.2 x, while a CPU simulation of nothing but the scores accumulated as one fp32 FMA chain, the arithmetic of
    precision 0, gives 1.16e-6 for that tensor; torch's own fp32 scores carry the larger maximum error there, 3.5e-6 against 2.6e-6.)"""
    out, grads = run_op(e0, e1, lb, g)

    def ref(dtype):
        a, b, c = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (e0, e1, lb))
        o = three_lines(a, b, c)
        o.backward(g.cpu().to(dtype))
        return o.detach(), a.grad, b.grad, c.grad
    r64, r32 = ref(torch.float64), ref(torch.float32)
    own = [relerr(b, a) for a, b in zip(r64, r32)]
    yard = [own[0]] + [max(own[1:])] * 3
    for n, t, a, o1, y in zip(("out",) + GRADS, (out,) + grads, r64, own, yard):
        err = relerr(t, a.reshape(t.shape))
        print("%s %-10s err %.3g  fp32 CPU err %.3g  yardstick %.3g" % (what, n, err, o1, y))
        assert err <= 4 * y, (what, n, err, y)
    return out, grads


@pytest.mark.parametrize("B,R,Q,K", [(1, 150, 140, 17), (1, 20, 300, 2), (1, 300, 11, 2), (3, 130, 70, 9)])
def test_chunked_rows_small_maps_and_batches(B, R, Q, K):
    _check_against_torch(*_small(B, R, Q, K, 100 + K), "B%d R%d Q%d K%d" % (B, R, Q, K))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_shared_value_rows_sum_their_gradient_over_the_frames(dtype):
    """values_per_frame = 0 of the C-ABI (value rows shared by the frames, the forward's SOT layout): grad_values is the sum over the frames of
    the per-frame gradients, frames added in order by the one writer of each element"""
    from unicorn_amd import ops
    e0, e1, lb, g = (t.to(dtype) for t in _small(3, 90, 75, 2, 5))
    er, ec, v = e0.transpose(1, 2).contiguous(), e1.transpose(1, 2).contiguous(), lb[0].contiguous()
    out, lse = ops.corr_softmax_pv_lse(er, ec, v)
    out_pf, lse_pf = ops.corr_softmax_pv_lse(er, ec, v.unsqueeze(0).expand(3, -1, -1))
    assert torch.equal(out, out_pf) and torch.equal(lse, lse_pf)
    ger, gec, gv = ops.corr_softmax_pv_backward(er, ec, v, out, lse, g)
    per, pec, pv = ops.corr_softmax_pv_backward(er, ec, v.unsqueeze(0).expand(3, -1, -1), out, lse, g)
    assert torch.equal(ger, per) and torch.equal(gec, pec) and gv.shape == v.shape
    # the same B x Q non-negative-weighted terms added in two orders: the a-priori bound of a recursive sum, n eps sum |term|, with
    # sum |term| = the gradient for |grad_out| (P >= 0)
    eps = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    mag = ops.corr_softmax_pv_backward(er, ec, v, out, lse, g.abs(), need=(False, False, True))[2]
    assert float((gv - pv.sum(0)).abs().max()) <= 3 * 75 * eps * float(mag.max())
    only = ops.corr_softmax_pv_backward(er, ec, v, out, lse, g, need=(False, False, True))
    assert only[0] is None and only[1] is None and torch.equal(only[2], gv)


def test_partial_requires_grad_and_layouts():
    from unicorn_amd import ops
    e0, e1, lb, g = _small(2, 8 * 13, 8 * 13, 3, 9)
    out, full = run_op(e0, e1, lb, g)
    for need in ((False, True, False), (True, True, False), (True, False, True)):
        o, part = run_op(e0, e1, lb, g, need=need)
        assert torch.equal(o, out)
        for want, a, b in zip(need, part, full):
            assert (a is None) if not want else torch.equal(a, b), need          # one writer per element: the same bits
    # nothing requires a gradient: the graph is not recorded and the result is the same
    assert torch.equal(ops.propagate_labels(e0, e1, lb), out) and not ops.propagate_labels(e0, e1, lb).requires_grad
    # non-contiguous grad_output
    gt = g.transpose(1, 2).contiguous().transpose(1, 2)
    assert not gt.is_contiguous()
    _, part = run_op(e0, e1, lb, gt)
    assert all(torch.equal(a, b) for a, b in zip(part, full))
    # NCHW and channels_last maps
    m0, m1 = e0.reshape(2, 128, 8, 13), e1.reshape(2, 128, 8, 13)
    for fmt in (torch.contiguous_format, torch.channels_last):
        a, b = m0.contiguous(memory_format=fmt), m1.contiguous(memory_format=fmt)
        o, part = run_op(a, b, lb, g)
        assert torch.equal(o, out) and part[0].shape == m0.shape
        assert torch.equal(part[0].reshape(2, 128, -1), full[0]) and torch.equal(part[1].reshape(2, 128, -1), full[1]) and torch.equal(part[2], full[2])
    # a precision without a backward is refused when a gradient is wanted, not silently widened
    from unicorn_amd import _lib
    with pytest.raises(_lib.UnicornHipError, match="precision 0"):
        ops.propagate_labels(e0.clone().requires_grad_(True), e1, lb, precision=2)
    assert ops.propagate_labels(e0, e1, lb, precision=2).shape == out.shape


def test_two_runs_are_bitwise_equal():
    """one writer per output element and a fixed summation order (two recompute passes, no float atomics): the structure is deterministic"""
    e0, e1, lb, g = _small(2, 1500, 1300, 3, 21)
    o1, g1 = run_op(e0, e1, lb, g)
    o2, g2 = run_op(e0, e1, lb, g)
    assert torch.equal(o1, o2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_end_to_end_loss_shape_on_a_small_map():
    """propagate_labels -> bilinear 1/2, 1/4 pyramid -> a scalar, backward into two nn.Conv2d-produced embeddings (unicorn.py:321-334);
    parameter gradients against the same graph built from the three torch lines in fp64 on the CPU, bound 4 x that graph's own fp32 error."""
    from unicorn_amd import ops
    H, W = 40, 64
    torch.manual_seed(3)
    # conv0 has no bias: a constant added to every reference embedding shifts each column of the scores by a constant, the softmax over the
    # reference axis does not see it, so that gradient is exactly zero and a relative comparison of it would divide by rounding noise
    conv0, conv1 = torch.nn.Conv2d(16, 128, 3, padding=1, bias=False), torch.nn.Conv2d(16, 128, 3, padding=1)
    x0, x1 = torch.randn(1, 16, H, W), torch.randn(1, 16, H, W)
    lbs = torch.rand(1, 1, H * W)
    tgt = torch.rand(1, 1, H, W)
    w = [torch.randn(1, 1, H, W), torch.randn(1, 1, H // 2, W // 2), torch.randn(1, 1, H // 4, W // 4)]

    def graph(dtype, dev, prop):
        c0, c1 = torch.nn.Conv2d(16, 128, 3, padding=1, bias=False).to(dev, dtype), torch.nn.Conv2d(16, 128, 3, padding=1).to(dev, dtype)
        c0.load_state_dict({k: v.to(dtype) for k, v in conv0.state_dict().items()})
        c1.load_state_dict({k: v.to(dtype) for k, v in conv1.state_dict().items()})
        e0, e1 = 0.25 * c0(x0.to(dev, dtype)), 0.25 * c1(x1.to(dev, dtype))
        pred = prop(e0, e1, lbs.to(dev, dtype)).view(1, 1, H, W)
        ms = (pred, F.interpolate(pred, scale_factor=1 / 2, mode="bilinear", align_corners=False),
              F.interpolate(pred, scale_factor=1 / 4, mode="bilinear", align_corners=False))
        loss = sum((m * wi.to(dev, dtype)).sum() for m, wi in zip(ms, w)) + ((pred - tgt.to(dev, dtype)) ** 2).sum()
        loss.backward()
        return [loss.detach()] + [p.grad for p in list(c0.parameters()) + list(c1.parameters())]
    ref = graph(torch.float64, "cpu", three_lines)
    own = graph(torch.float32, "cpu", three_lines)
    got = graph(torch.float32, "cuda", ops.propagate_labels)
    for n, a, b, c in zip(("loss", "w0", "w1", "b1"), got, own, ref):
        err, e32 = relerr(a, c), relerr(b, c)
        print("end-to-end %-4s err %.3g  fp32 CPU graph err %.3g" % (n, err, e32))
        assert err <= 4 * max(e32, 2.0 ** -24), (n, err, e32)
