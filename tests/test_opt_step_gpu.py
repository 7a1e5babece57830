"""ops.adamw_ema_step / unicorn_amd.optim.FusedAdamWEMA (uni_opt_step) on the GPU.

Bound of every float comparison with an fp64 expectation: err = max |got - expected| over the whole list / max |expected| over the whole list,
per kind (p, m, v), must be <= 2 x the fp32 reference error + 2^-23.  The reference error is torch's own fp32 result against its fp64 result
on the CPU (recorded in the fixtures; computed by the restatement of tests/opt_step_ref.py for shapes the fixtures do not hold); the factor 2
allows a different but equally valid rounding order, 2^-23 is half an fp32 ulp of the scale.  No figure comes from the kernel.  The EMA is
held to BITS: torch's two lines evaluated on the CPU from the same inputs."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

import opt_step_ref as R  # noqa: E402
import variant_cases as vc  # noqa: E402

DEV = "cuda"
ULP = 2.0 ** -23


@pytest.fixture(scope="module")
def L():
    from unicorn_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return _lib


def traced(L, fn):
    lib = L.lib()
    lib.uni_variant_trace(1)
    try:
        r = fn()
        torch.cuda.synchronize()
    finally:
        lib.uni_variant_trace(0)
    return r, {t: n for t, n in vc.read_trace(lib).items() if t.startswith("opt_step")}


def ema_lines(e_old, p_new, d):
    """ModelEMA.update's two lines on the CPU"""
    v = e_old.detach().cpu().clone()
    v *= d
    v += (1.0 - d) * p_new.detach().cpu()
    return v


def bits(t):
    return t.detach().contiguous().view(torch.int32) if t.numel() else t.detach().reshape(0).view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a.cpu()), bits(b.cpu()))


def list_err(got, exp):
    """max |got - exp| over the list / max |exp| over the list"""
    num = max((float((g.detach().double().cpu() - x).abs().max()) for g, x in zip(got, exp) if x.numel()), default=0.0)
    den = max(float(x.abs().max()) for x in exp if x.numel())
    return num / den


# ------------------------------------------------------------------------------------------------ fixtures
@pytest.mark.parametrize("tag", list(R.CASES))
def test_fixture(L, tag):
    from unicorn_amd import ops
    c, cfg = R.load_case(tag), R.CASES[tag]
    ent = [(n, s, k) for n, s, k in R.shapes(tag) if k != "ibuf"]
    p = [torch.from_numpy(c["p0_" + n]).to(DEV) for n, _, _ in ent]
    e = [torch.from_numpy(c["e0_" + n]).to(DEV) for n, _, _ in ent]
    m = [torch.zeros_like(x) if k == "param" else None for x, (_, _, k) in zip(p, ent)]
    v = [torch.zeros_like(x) if k == "param" else None for x, (_, _, k) in zip(p, ent)]
    g = [torch.empty_like(x) if k == "param" else None for x, (_, _, k) in zip(p, ent)]
    lrf = [R.group_of(tag, i)[0] for i in range(len(ent))]
    wds = [cfg["wd"] * R.group_of(tag, i)[1] for i in range(len(ent))]
    step = torch.zeros((), device=DEV)
    words = None
    if cfg["scaler"]:
        words = (torch.full((), cfg["scaler"]["init_scale"], device=DEV), torch.zeros((), dtype=torch.int32, device=DEV), torch.ones((), device=DEV))
    sc = {k: cfg["scaler"][k] for k in ("growth_factor", "backoff_factor", "growth_interval")} if cfg["scaler"] else {}
    plan, e_only = None, [x.cpu().clone() for x in e]
    for k in range(cfg["steps"]):
        for gi, (n, _, kind) in zip(g, ent):
            if kind == "param":
                gi.copy_(torch.from_numpy(c["gs_" + n][k]))
        d = R.ema_decay_at(cfg["updates"] + k + 1)
        e_old = [x.clone() for x in e]
        plan = ops.adamw_ema_step(p, g, m, v, e, step, lr=cfg["lr"], betas=R.BETAS, eps=R.EPS, weight_decay=wds, lr_factors=lrf, ema_decay=d,
                                  scaler=words, plan=plan, **sc)
        for i, (n, _, kind) in enumerate(ent):
            # parameters: the operator's own p_new and the old e through torch's two lines; EMA-only entries: the chain from the inputs
            assert same_bits(e[i], ema_lines(e_old[i], p[i], d)), (tag, k, n)
            if kind != "param":
                e_only[i] = ema_lines(e_only[i], torch.from_numpy(c["p0_" + n]), d)
                assert same_bits(e[i], e_only[i]) and same_bits(p[i], torch.from_numpy(c["p0_" + n])), (tag, k, n)
        if words is not None:
            assert float(words[2]) == (1.0 if k == cfg["bad_step"] else 0.0)
    assert plan.uploads == 1                                                      # the gradients kept their addresses
    assert float(step) == float(c["step"])
    if words is not None:
        assert float(words[0]) == float(c["scale"]) and int(words[1]) == int(c["growth_tracker"])
    par = [i for i, (_, _, k) in enumerate(ent) if k == "param"]
    for kind, got in (("p", p), ("m", m), ("v", v)):
        exp = [torch.from_numpy(c["%s_%s" % (kind, ent[i][0])]) for i in par]
        err, ref = list_err([got[i] for i in par], exp), float(c[kind + "_fp32_ref_err"])
        print("opt_step fixture %-8s %s: err %.3e, fp32 reference %.3e, ratio %.2f, bound %.3e" % (tag, kind, err, ref, err / ref, 2 * ref + ULP))
        assert err <= 2 * ref + ULP, (tag, kind, err, ref)


# ------------------------------------------------------------------------------------------------ the ragged list
def ragged(L, seed=3, scale=256.0):
    ch = L.lib().uni_opt_chunk_elems()
    spec = R.ragged_spec(ch)
    cpu = R.ragged_draw(spec, seed, grad_scale=scale)
    return ch, spec, cpu


def to_dev(stor):
    return {a: [None if t is None else t.to(DEV) for t in lst] for a, lst in stor.items()}


def run_ragged(L, spec, cpu, steps, scaler, d=0.9991, lr=1e-3):
    from unicorn_amd import ops
    stor = to_dev(cpu)
    v = R.ragged_views(spec, stor)
    n = len(spec)
    lrf, wds = [0.1 if i % 4 == 0 else 1.0 for i in range(n)], [0.0 if i % 3 == 0 else 5e-4 for i in range(n)]
    step = torch.full((), 7.0, device=DEV)
    words = (torch.full((), scaler, device=DEV), torch.zeros((), dtype=torch.int32, device=DEV), torch.ones((), device=DEV)) if scaler else None
    plan = None
    for _ in range(steps):
        plan = ops.adamw_ema_step(v["p"], v["g"], v["m"], v["v"], v["e"], step, lr=lr, betas=R.BETAS, eps=R.EPS, weight_decay=wds, lr_factors=lrf,
                                  ema_decay=d, scaler=words, growth_interval=2000, plan=plan)
    torch.cuda.synchronize()
    return stor, v, step, words, (lrf, wds)


def restated(spec, cpu, dtype, steps, scaler, lrf, wds, d=0.9991, lr=1e-3):
    stor = {a: [None if t is None else t.to(dtype).clone() for t in lst] for a, lst in cpu.items()}
    v = R.ragged_views(spec, stor)
    st = {"step": 7.0}
    sc = None
    if scaler:
        st.update(scale=scaler, tracker=0)
        sc = dict(growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
    for _ in range(steps):
        assert not R.adamw_ema_step(v["p"], v["g"], v["m"], v["v"], v["e"], st, lr=lr, lr_factors=lrf, wds=wds, d=d, scaler=sc)
    return stor, v, st


@pytest.fixture(scope="module")
def ragged_run(L):
    """one traced two-step run of the ragged list with a scaler, shared (and left unchanged) by the tests below"""
    ch, spec, cpu = ragged(L)
    (stor, v, step, words, hyper), tags = traced(L, lambda: run_ragged(L, spec, cpu, 2, 256.0))
    return dict(ch=ch, spec=spec, cpu=cpu, stor=stor, v=v, step=step, words=words, hyper=hyper, tags=tags)


def test_ragged_list_against_the_restatement(L, ragged_run):
    r = ragged_run
    spec, cpu = r["spec"], r["cpu"]
    lrf, wds = r["hyper"]
    _, v64, st64 = restated(spec, cpu, torch.float64, 2, 256.0, lrf, wds)
    _, v32, _ = restated(spec, cpu, torch.float32, 2, 256.0, lrf, wds)
    full = [i for i, s in enumerate(spec) if s["grad"]]
    for kind in ("p", "m", "v"):
        exp = [v64[kind][i] for i in full]
        ref = list_err([v32[kind][i] for i in full], exp)
        err = list_err([r["v"][kind][i] for i in full], exp)
        print("opt_step ragged %s: err %.3e, fp32 reference %.3e, bound %.3e" % (kind, err, ref, 2 * ref + ULP))
        assert err <= 2 * ref + ULP, (kind, err, ref)
    assert float(r["step"]) == st64["step"] == 9.0 and float(r["words"][0]) == 256.0 and int(r["words"][1]) == 2 and float(r["words"][2]) == 0.0
    # both forms ran, in one update launch per step
    assert r["tags"] == {"opt_step check scaler=1": 2, "opt_step update scaler=1 forms=vec+scalar": 2, "opt_step finish scaler=1": 2}, r["tags"]
    # what lies around the views in the enclosing storages keeps its bits; EMA-only entries keep their parameter; gradients are left alone
    for a in R.ARRAYS:
        for i, s in enumerate(spec):
            st = r["stor"][a][i]
            if st is None:
                continue
            o = s["off"][R.ARRAYS.index(a)]
            assert same_bits(st[:o], cpu[a][i][:o]) and same_bits(st[o + s["n"]:], cpu[a][i][o + s["n"]:]), (a, i)
            if a == "g" or (a == "p" and not s["grad"]):
                assert same_bits(st, cpu[a][i]), (a, i)


def test_ragged_list_ema_is_bitwise_torchs_two_lines(L):
    ch, spec, cpu = ragged(L, seed=4)
    stor, v, step, words, _ = run_ragged(L, spec, cpu, 1, 256.0)
    e0 = R.ragged_views(spec, cpu)["e"]
    for i, s in enumerate(spec):
        assert same_bits(v["e"][i], ema_lines(e0[i], v["p"][i], 0.9991)), (i, s)


def test_launch_count_and_bitwise_repeatability(L, ragged_run):
    from unicorn_amd import ops
    one = [torch.randn(1000, device=DEV) for _ in range(5)]
    one[3].abs_()
    step = torch.zeros((), device=DEV)
    words = (torch.full((), 8.0, device=DEV), torch.zeros((), dtype=torch.int32, device=DEV), torch.zeros((), device=DEV))

    def call(scaler):
        return ops.adamw_ema_step([one[0]], [one[1]], [one[2]], [one[3]], [one[4]], step, lr=1e-3, ema_decay=0.99, scaler=scaler)
    _, tags = traced(L, lambda: call(words))
    assert sum(tags.values()) == 3 and tags == {"opt_step check scaler=1": 1, "opt_step update scaler=1 forms=vec": 1, "opt_step finish scaler=1": 1}, tags
    _, tags = traced(L, lambda: call(None))
    assert sum(tags.values()) == 2 and tags == {"opt_step update scaler=0 forms=vec": 1, "opt_step finish scaler=0": 1}, tags
    assert float(step) == 2.0
    r = ragged_run
    assert sum(r["tags"].values()) == 3 * 2                                                      # 3 launches per step for 320 tensors
    (_, v0, _, _, _), tags = traced(L, lambda: run_ragged(L, r["spec"], r["cpu"], 2, None))
    assert sum(tags.values()) == 2 * 2 and tags["opt_step update scaler=0 forms=vec+scalar"] == 2, tags
    # two runs from the same state: the same bits (one writer per element, no atomics)
    stor2, _, step2, words2, _ = run_ragged(L, r["spec"], r["cpu"], 2, 256.0)
    for a in R.ARRAYS:
        for x, y in zip(r["stor"][a], stor2[a]):
            assert x is None or same_bits(x, y), a
    assert float(step2) == float(r["step"]) and float(words2[0]) == float(r["words"][0])


# ------------------------------------------------------------------------------------------------ the optimizer-shaped wrapper
class Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 8, 3)
        self.bn = torch.nn.BatchNorm2d(8)            # float buffers (EMA only) and an int64 buffer (not listed)
        self.fc = torch.nn.Linear(8, 5)
        self.frozen = torch.nn.Parameter(torch.randn(11), requires_grad=False)


def make(seed=0, **kw):
    from unicorn_amd import optim
    torch.manual_seed(seed)
    net = Net().to(DEV)
    with torch.no_grad():
        net.bn.running_mean.normal_()
    ema = copy.deepcopy(net).eval()
    with torch.no_grad():
        for t in ema.state_dict().values():
            if t.dtype.is_floating_point:
                t.add_(0.01)
    opt = optim.FusedAdamWEMA(net, ema, lr=1e-3, weight_decay=5e-4, ema_decay=0.9998, ema_updates=5000, **kw)
    return net, ema, opt


def grads_for(net, k, scale=1.0):
    g = torch.Generator().manual_seed(100 + k)
    return [(torch.randn(p.shape, generator=g) * 0.1 * scale).to(DEV) for p in net.parameters() if p.requires_grad]


def feed(net, gs, in_place):
    for p, g in zip((p for p in net.parameters() if p.requires_grad), gs):
        if in_place and p.grad is not None:
            p.grad.copy_(g)
        else:
            p.grad = g.clone()


def test_skipped_step_keeps_p_m_v_step_and_never_synchronises(L):
    net, ema, opt = make(scaler=dict(init_scale=64.0, growth_interval=100))
    for k in range(2):
        feed(net, grads_for(net, k, 64.0), in_place=True)
        opt.step()
    assert opt.plan.uploads == 1
    feed(net, grads_for(net, 2, 64.0), in_place=True)
    net.fc.weight.grad.view(-1)[7] = float("inf")
    torch.cuda.synchronize()
    before = {"p": [p.detach().clone() for p in opt._src], "m": [None if m is None else m.clone() for m in opt._m],
              "v": [None if v is None else v.clone() for v in opt._v], "e": [e.clone() for e in opt._ema], "step": opt._step.clone()}
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()                                    # steady state: no upload, no .item(), no stream synchronisation
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert opt.plan.uploads == 1 and opt.ema_updates == 5003
    d = R.ema_decay_at(5003)
    for i in range(len(opt._src)):
        assert same_bits(opt._src[i], before["p"][i])
        if opt._m[i] is not None:
            assert same_bits(opt._m[i], before["m"][i]) and same_bits(opt._v[i], before["v"][i])
        assert same_bits(opt._ema[i], ema_lines(before["e"][i], before["p"][i], d)) and not same_bits(opt._ema[i], before["e"][i])
    assert same_bits(opt._step, before["step"]) and float(opt._step) == 2.0
    assert float(opt._words[0]) == 32.0 and int(opt._words[1]) == 0 and float(opt._words[2]) == 1.0
    assert all(float(p.grad.abs().max()) == 0.0 for p in net.parameters() if p.requires_grad)      # zero_grad zeroed in place
    assert float(opt.scale(torch.ones((), device=DEV))) == 32.0
    assert ema.bn.num_batches_tracked.item() == 0 and len(opt._src) == 9 and sum(g >= 0 for g in opt._group) == 6


def test_replaced_gradients_cost_exactly_one_upload_and_change_no_bit(L):
    def run(replace):
        net, ema, opt = make(seed=1)
        keep = []
        for k in range(3):
            feed(net, grads_for(net, k), in_place=not (replace and k == 1))
            keep.append([p.grad for p in net.parameters()])          # old gradients stay alive: the new ones cannot land on their addresses
            opt.step()
        torch.cuda.synchronize()
        return net, ema, opt
    a, b = run(False), run(True)
    assert a[2].plan.uploads == 1 and b[2].plan.uploads == 2
    for x, y in zip(a[0].state_dict().values(), b[0].state_dict().values()):
        assert torch.equal(x, y)
    for x, y in zip(a[1].state_dict().values(), b[1].state_dict().values()):
        assert torch.equal(x, y)
    for x, y in zip(a[2]._m + a[2]._v, b[2]._m + b[2]._v):
        assert x is None or same_bits(x, y)
    assert float(a[2]._step) == 3.0 and float(b[2]._step) == 3.0


def test_state_dict_round_trip_with_torch_adamw(L):
    from unicorn_amd import optim
    torch.manual_seed(2)
    net0 = Net()
    gs = [[g.cpu() for g in grads_for(net0, k)] for k in range(4)]

    def torch_run(dtype, device, steps):
        net = copy.deepcopy(net0).to(dtype).to(device)
        ps = [p for p in net.parameters()]
        opt = torch.optim.AdamW([{"params": ps}], lr=1e-3, weight_decay=5e-4)
        for k in steps:
            for p, g in zip((p for p in ps if p.requires_grad), gs[k]):
                p.grad = g.to(dtype).to(device)
            opt.step()
        return net, opt
    exp = [p.detach() for p in torch_run(torch.float64, "cpu", range(4))[0].parameters() if p.requires_grad]
    ref = [p.detach() for p in torch_run(torch.float32, "cpu", range(4))[0].parameters() if p.requires_grad]
    ref_err = list_err(ref, exp)
    tnet, topt = torch_run(torch.float32, DEV, range(2))                        # torch.optim.AdamW on the GPU for 2 steps
    net = copy.deepcopy(tnet)
    ema = copy.deepcopy(net).eval()
    opt = optim.FusedAdamWEMA(net, ema, lr=1e-3, weight_decay=5e-4)
    opt.load_state_dict(topt.state_dict())
    assert float(opt._step) == 2.0
    for k in (2, 3):
        feed(net, [g.to(DEV) for g in gs[k]], in_place=True)
        opt.step()
        for p, g in zip((p for p in tnet.parameters() if p.requires_grad), gs[k]):
            p.grad = g.to(DEV)
        topt.step()
    got = [p for p in net.parameters() if p.requires_grad]
    err = list_err(got, exp)
    err_t = list_err([p for p in tnet.parameters() if p.requires_grad], exp)
    print("opt_step round trip: err %.3e (torch on the GPU %.3e), fp32 reference %.3e, bound %.3e" % (err, err_t, ref_err, 2 * ref_err + ULP))
    assert err <= 2 * ref_err + ULP
    sd = opt.state_dict()
    fresh = torch.optim.AdamW([{"params": [p for p in net.parameters()]}], lr=1e-3, weight_decay=5e-4)
    fresh.load_state_dict(sd)                                                  # and back into torch.optim.AdamW
    assert set(sd["param_groups"][0]) == set(topt.state_dict()["param_groups"][0])
    st = fresh.state[net.fc.weight]
    assert float(st["step"]) == 4.0 and torch.equal(st["exp_avg"], opt._m[[i for i, t in enumerate(opt._src) if t is net.fc.weight][0]])
    tst = topt.state[tnet.fc.weight]
    assert float((st["exp_avg"] - tst["exp_avg"]).abs().max()) <= 1e-6 * float(tst["exp_avg"].abs().max())
