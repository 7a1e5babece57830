"""GPU checks of the fused CondInst mask loss through the public surface (ops.condinst_dice_loss, ops.CondInstDiceFunction): the fp64 path
against the fixtures of the reference's own functions, the fp32 kernels against the same fixtures with the bound of
tests/test_corr_backward_gpu.py and tests/test_msda_backward_gpu.py (4 x the error of an fp32 evaluation of the same lines: another summation
order and FMA contraction, never a figure taken from the kernel), gradcheck, reproducibility, partial gradients, the existing inference
operator, and the headline geometry with its memory condition."""
import numpy as np
import pytest
import torch

import condinst_loss_ref as R

pytestmark = pytest.mark.gpu

GRADS = ("g_mask_feats", "g_up_masks", "g_params")


def relerr(got, ref):
    ref = ref.double()
    return float((got.double().cpu() - ref.cpu()).abs().max() / ref.abs().max())


def dev_case(c, dtype):
    f = [torch.from_numpy(c[n]).to("cuda", dtype) for n in ("mask_feats", "up_masks", "params", "inst_loc")]
    return f + [torch.from_numpy(c["inst_lvl"]).cuda(), torch.from_numpy(c["gt"]).to("cuda", dtype), torch.from_numpy(c["grad_loss"]).to("cuda", dtype)]


def run_op(mf, um, p, loc, lvl, gt, g, r, need=(True, True, True), ldp=None):
    """forward + backward through ops.condinst_dice_loss -> loss, (grad_mask_feats, grad_up_masks, grad_params)"""
    from unicorn_amd import ops
    mf = mf.detach().clone().requires_grad_(need[0])
    um = um.detach().clone().requires_grad_(need[1])
    if ldp is None:
        p = p.detach().clone().requires_grad_(need[2])
        pv = p
    else:                                                # rows of pitch ldp > 169: the C-ABI's ldp, reached without a copy
        wide = torch.full((p.shape[0], ldp), float("nan"), device=p.device, dtype=p.dtype)
        wide[:, :169] = p
        p = wide.requires_grad_(need[2])
        pv = p[:, :169]
        assert pv.stride(0) == ldp
    loss = ops.condinst_dice_loss(mf, um, pv, loc, lvl, gt, r)
    if any(need):
        loss.backward(g)
    gp = p.grad if ldp is None or p.grad is None else p.grad[:, :169]
    return loss.detach(), (mf.grad, um.grad, gp)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp64_path_equals_the_fixture(tag):
    c = R.load_case(tag)
    mf, um, p, loc, lvl, gt, g = dev_case(c, torch.float64)
    loss, grads = run_op(mf, um, p, loc, lvl, gt, g, R.CASES[tag][2], ldp=176 if tag == "ragged" else None)
    for n, t in dict(zip(GRADS, grads), loss=loss).items():
        err = relerr(t, torch.from_numpy(c[n]))
        print("fp64 %-7s %-13s err %.3g" % (tag, n, err))
        assert err <= 1e-12, (tag, n, err)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_fp32_against_the_fixture(tag):
    c = R.load_case(tag)
    mf, um, p, loc, lvl, gt, g = dev_case(c, torch.float32)
    loss, grads = run_op(mf, um, p, loc, lvl, gt, g, R.CASES[tag][2], ldp=176 if tag == "ragged" else None)
    bad = []
    for n, t in dict(zip(GRADS, grads), loss=loss).items():
        err, bound = relerr(t, torch.from_numpy(c[n])), 4 * float(c[n + "_fp32_ref_err"])
        print("fp32 %-7s %-13s err %.3g  fp32_ref_err %.3g  ratio %.2f (bound 4)" % (tag, n, err, bound / 4, 4 * err / bound))
        if not err <= bound:
            bad.append((n, err, bound))
    assert not bad, bad


def _small(H, W, r, n, seed, dtype=torch.float32, kink=None):
    """random small problem on the device; kink: redraw (next seed) until every hidden pre-activation is farther than this from zero"""
    while True:
        g = torch.Generator().manual_seed(seed)
        mf = torch.randn(1, 8, H, W, generator=g, dtype=torch.float64)
        um = torch.randn(1, 9 * r * r, H, W, generator=g, dtype=torch.float64)
        p = 0.5 * torch.randn(n, 169, generator=g, dtype=torch.float64)
        loc = torch.stack([torch.randint(0, 8 * W, (n,), generator=g), torch.randint(0, 8 * H, (n,), generator=g)], dim=1).double()
        lvl = torch.randint(0, 5, (n,), generator=g).to(torch.int32)
        gt = (torch.rand(n, 1, r * H, r * W, generator=g) < 0.4).double()
        go = torch.randn(n, generator=g, dtype=torch.float64)
        if kink is None:
            break
        _, p0, p1 = R.pre_activations(mf, p, loc, lvl)
        if min(float(p0.abs().min()), float(p1.abs().min())) > kink:
            break
        seed += 1
    return [t.to("cuda", dtype) for t in (mf, um, p, loc)] + [lvl.cuda(), gt.to("cuda", dtype), go.to("cuda", dtype), r]


@pytest.mark.parametrize("H,W,r,n", [(3, 4, 2, 2), (2, 3, 4, 3)])
def test_gradcheck_fp64(H, W, r, n):
    """finite differences of step 1e-6 must not cross a ReLU kink: the draw keeps every pre-activation 1e-3 away from zero"""
    from unicorn_amd import ops
    mf, um, p, loc, lvl, gt, _, r = _small(H, W, r, n, 10 * H + W, torch.float64, kink=1e-3)
    mf, um, p = (t.requires_grad_(True) for t in (mf, um, p))
    assert torch.autograd.gradcheck(lambda a, b, c: ops.condinst_dice_loss(a, b, c, loc, lvl, gt, r), (mf, um, p), nondet_tol=0)


def test_two_runs_are_bitwise_equal():
    """one writer per output element and fixed summation orders (no float atomics); 37 instances: three backward chunks"""
    args = _small(20, 28, 4, 37, 5)
    l1, g1 = run_op(*args)
    l2, g2 = run_op(*args)
    assert torch.equal(l1, l2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


def test_partial_requires_grad():
    from unicorn_amd import ops
    args = _small(9, 13, 4, 19, 6)
    loss, full = run_op(*args)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)):
        l, part = run_op(*args, need=need)
        assert torch.equal(l, loss)
        for want, a, b in zip(need, part, full):
            assert (a is None) if not want else torch.equal(a, b), need          # one writer per element: the same bits
    l, part = run_op(*args, need=(False, False, False))                           # nothing requires a gradient: no graph, the same result
    assert torch.equal(l, loss) and not ops.condinst_dice_loss(*args[:6], args[7]).requires_grad
    # the (N, rH, rW) form of the ground truth, integer levels of another width, no instance at all
    mf, um, p, loc, lvl, gt, g, r = args
    assert torch.equal(ops.condinst_dice_loss(mf, um, p, loc, lvl.long(), gt[:, 0], r), loss)
    empty = ops.condinst_dice_loss(mf, um, p[:0], loc[:0], lvl[:0], gt[:0], r)
    assert empty.shape == (0,) and empty.dtype == torch.float32


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_forward_agrees_with_the_inference_operator(tag):
    """sigmoid scores of ops.condinst_masks(d_rate = 1), dice sums redone in torch fp64, against this operator's loss: the fp32 bound of the
    fixture test (the inference kernel uses __expf, so not bitwise)"""
    from unicorn_amd import ops
    c = R.load_case(tag)
    mf, um, p, loc, lvl, gt, _ = dev_case(c, torch.float32)
    r = R.CASES[tag][2]
    loss = ops.condinst_dice_loss(mf, um, p, loc, lvl, gt, r)
    s = ops.condinst_masks(mf, um, p, loc, lvl, r, 1).double().reshape(p.shape[0], -1)
    g = gt.double().reshape(p.shape[0], -1)
    redone = 1 - 2 * (s * g).sum(1) / ((s * s).sum(1) + (g * g).sum(1) + 1e-5)
    ref = torch.from_numpy(c["loss"])
    bound = 4 * float(c["loss_fp32_ref_err"]) * float(ref.abs().max())
    d = float((redone - loss.double()).abs().max())
    print("inference %-7s max|redone - loss| %.3g  bound %.3g  ratio %.2f; redone vs fixture %.3g" % (
        tag, d, bound, d / bound, float((redone.cpu() - ref).abs().max())))
    assert d <= bound, (tag, d, bound)


KINK = 5e-5


def _headline_inputs(n, H, W, r, seed):
    """Synthetic inputs with no hidden unit on a ReLU kink, the rule of the fixtures: at a kink the gradient legitimately jumps by one pixel's
    share (about 1 / 16000 of a parameter gradient here, two orders above fp32 rounding), so inputs whose fp32 and fp64 evaluations take
    different branches would measure the draw, not the kernel.  Among 128 x 16000 x 16 random pre-activations some always fall within fp32
    rounding of zero and a redraw cannot help, so the bias of a unit (instance, channel) that has a pixel with |pre-activation| <= KINK is
    moved by steps of 2^-10 until none has, layer 0 first.  KINK = 5e-5 is above the a-priori fp32 error of these 10- and 8-term sums
    (terms below 40: 10 x 2^-24 x 40 = 2.4e-5)."""
    g = torch.Generator().manual_seed(seed)
    mf = torch.randn(1, 8, H, W, generator=g).cuda()
    um = torch.randn(1, 9 * r * r, H, W, generator=g).cuda()
    p = (0.35 * torch.randn(n, 169, generator=g)).cuda()
    loc = (torch.stack([torch.randint(0, 32 * W, (n,), generator=g), torch.randint(0, 32 * H, (n,), generator=g)], dim=1).float() / 4).cuda()
    lvl = torch.randint(0, 5, (n,), generator=g).to(torch.int32).cuda()
    gt = torch.zeros(n, 1, r * H, r * W)
    for i in range(n):
        y0, x0 = int(torch.randint(0, r * H // 2, (1,), generator=g)), int(torch.randint(0, r * W // 2, (1,), generator=g))
        gt[i, 0, y0:y0 + 8 + int(torch.randint(0, r * H // 2, (1,), generator=g)), x0:x0 + 8 + int(torch.randint(0, r * W // 2, (1,), generator=g))] = 1
    go = torch.randn(n, generator=g).cuda()
    for layer, cols in ((0, slice(152, 160)), (1, slice(160, 168))):
        for _ in range(200):
            pre = R.pre_activations(mf.double(), p.double(), loc.double(), lvl)[1 + layer]
            bad = (pre.abs() <= KINK).any(dim=2)                          # (n, 8): units with a pixel on the kink
            if not bool(bad.any()):
                break
            p[:, cols] += bad.float() * 2.0 ** -10
        assert not bool(bad.any())
    return mf, um, p, loc, lvl, gt.cuda(), go


def test_headline_geometry_accuracy_and_memory():
    """800 x 1280 (H8 x W8 = 100 x 160), up_rate 4, 128 instances, fp32: loss and gradients within 4 x the error of the torch restatement in
    fp32 on the same GPU (both against the restatement in fp64, instance chunks of 16), and forward + backward in less than ONE
    (N, rH8, rW8) fp32 map of additional memory (131 MB): the feature's defining condition."""
    n, H, W, r = 128, 100, 160, 4
    mf, um, p, loc, lvl, gt, go = _headline_inputs(n, H, W, r, 17)
    _, a0, a1 = R.pre_activations(mf.double(), p.double(), loc.double(), lvl)
    _, b0, b1 = R.pre_activations(mf, p, loc, lvl)
    assert min(float(a0.abs().min()), float(a1.abs().min())) > KINK and torch.equal(a0 > 0, b0 > 0) and torch.equal(a1 > 0, b1 > 0)
    assert max(float((a0 - b0).abs().max()), float((a1 - b1).abs().max())) < KINK / 2      # the fp32 evaluation stays well inside the margin
    del a0, a1, b0, b1
    ref = R.loss_and_grads(mf.double(), um.double(), p.double(), loc.double(), lvl, gt.double(), r, go.double(), chunk=16)
    f32 = R.loss_and_grads(mf, um, p, loc, lvl, gt, r, go, chunk=16)
    small = _small(6, 8, 4, 3, 1)
    run_op(*small)                                                       # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, grads = run_op(mf, um, p, loc, lvl, gt, go, r)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    one_map = n * r * H * r * W * 4
    print("headline: peak memory rise over forward + backward %.1f MB (one (N, rH8, rW8) fp32 map: %.1f MB)" % (rise / 1e6, one_map / 1e6))
    bad = []
    for k, t in dict(zip(GRADS, grads), loss=loss).items():
        err, own = relerr(t, ref[k]), relerr(f32[k], ref[k])
        print("headline %-13s err %.3g  fp32 restatement err %.3g  ratio %.2f (bound 4)" % (k, err, own, err / own))
        if not err <= 4 * own:
            bad.append((k, err, own))
    assert not bad, bad
    assert rise < one_map, "forward + backward allocated %.1f MB: a full-resolution per-instance tensor (%.1f MB) was materialised" % (
        rise / 1e6, one_map / 1e6)
