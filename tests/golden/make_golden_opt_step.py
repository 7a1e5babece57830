"""Golden vectors for uni_opt_step / ops.adamw_ema_step / unicorn_amd.optim.FusedAdamWEMA, produced on the CPU by EXECUTING the three lines of
the reference's trainer (unicorn/core/trainer.py:260-275) on a small module:

    scaler.step(optimizer)        torch.optim.AdamW(foreach=False), groups as exp/unicorn_track.py:380-381 builds them (+ "factor")
    scaler.update()               torch.amp.GradScaler("cpu", ...)
    ema_model.update(model)       the reference's own ModelEMA (unicorn/utils/ema.py), imported for generation only

`scaler.scale(loss).backward()` is stood in for by assigning `p.grad = unscaled gradient of the draw x the scaler's current scale` (a power
of two: exact), with one inf and one NaN planted in different tensors of the bad step.  Every case is run in fp64 (the stored expectation)
and in fp32; <kind>_fp32_ref_err = max |fp32 - fp64| / max |fp64| over the whole list, per kind p / m / v / e: the yardstick of the GPU test
(no figure comes from the kernel).  Inputs are stored as fp32 (`gs_*`: the scaled gradients as fed), results as fp64, the seed with them.

    python tests/golden/make_golden_opt_step.py        -> tests/golden/opt_step_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import opt_step_ref as R  # noqa: E402

SEEDS = {"plain": 11, "scaled": 12, "groups": 13, "emaonly": 14}


def model_ema():
    import torch._dynamo  # noqa: F401  (optimizer.step imports it lazily; it must be in before the bootstrap's stub modules are)
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.utils.ema import ModelEMA
    return ModelEMA


class Net(torch.nn.Module):
    def __init__(self, tag, ins, dtype):
        super().__init__()
        for name, shape, kind in R.shapes(tag):
            if kind in ("param", "nograd"):
                self.register_parameter(name, torch.nn.Parameter(ins["p0_" + name].to(dtype).clone()))
            elif kind == "fbuf":
                self.register_buffer(name, ins["p0_" + name].to(dtype).clone())
            else:
                self.register_buffer(name, ins["p0_" + name].clone())


def run(tag, ins, dtype, ModelEMA):
    cfg = R.CASES[tag]
    net = Net(tag, ins, dtype)
    ema_model = ModelEMA(net, decay=R.EMA_DECAY, updates=cfg["updates"], is_distributed=False)
    esd = ema_model.ema.state_dict()
    for name, shape, kind in R.shapes(tag):
        if kind != "ibuf":
            esd[name].copy_(ins["e0_" + name].to(dtype))
    named = dict(net.named_parameters())
    groups = {}
    for i, (name, shape, kind) in enumerate(R.shapes(tag)):
        if kind in ("param", "nograd"):
            groups.setdefault(R.group_of(tag, i), []).append(named[name])
    param_dicts = [{"params": ps, "factor": f, "lr": cfg["lr"] * f, "weight_decay": cfg["wd"] * w} for (f, w), ps in groups.items()]
    optimizer = torch.optim.AdamW(param_dicts, lr=cfg["lr"], weight_decay=cfg["wd"], betas=R.BETAS, eps=R.EPS, foreach=False)
    scaler = torch.amp.GradScaler("cpu", enabled=cfg["scaler"] is not None, **(cfg["scaler"] or {}))
    fed, scales = {n: [] for n, _, k in R.shapes(tag) if k == "param"}, []
    for k in range(cfg["steps"]):
        optimizer.zero_grad()
        scaler.scale(torch.zeros((), dtype=dtype))          # the trainer's scaler.scale(loss): creates the scaler's device words on first use
        scale = float(scaler.get_scale()) if cfg["scaler"] else 1.0
        scales.append(scale)
        gk = {"g_" + n: (ins["g_" + n][k] * scale).clone() for n in fed}
        if cfg["bad_step"] == k:
            R.plant_bad(tag, gk)
        for n in fed:
            fed[n].append(gk["g_" + n])
            named[n].grad = gk["g_" + n].to(dtype)          # stands for scaler.scale(loss).backward()
        scaler.step(optimizer)
        scaler.update()
        ema_model.update(net)
    msd, st = net.state_dict(), optimizer.state
    res = {"p": {}, "m": {}, "v": {}, "e": {}}
    steps = set()
    for name, shape, kind in R.shapes(tag):
        if kind == "ibuf":
            assert torch.equal(esd[name], ins["p0_" + name]) and torch.equal(msd[name], ins["p0_" + name])
            continue
        res["p"][name], res["e"][name] = msd[name].detach().clone(), esd[name].detach().clone()
        s = st.get(named.get(name)) if name in named else None
        if kind == "param":
            res["m"][name], res["v"][name] = s["exp_avg"].clone(), s["exp_avg_sq"].clone()
            steps.add(float(s["step"]))
        else:
            assert not s, "%s must have no optimizer state" % name
            res["m"][name] = res["v"][name] = torch.zeros(shape, dtype=dtype)
    assert len(steps) == 1
    out = dict(res=res, step=steps.pop(), fed=fed, scales=scales, updates=ema_model.updates)
    if cfg["scaler"]:
        out.update(scale=float(scaler.get_scale()), tracker=int(scaler.state_dict()["_growth_tracker"]))
    return out


def main():
    ModelEMA = model_ema()
    for tag, seed in SEEDS.items():
        cfg = R.CASES[tag]
        ins = R.draw(tag, seed)
        r64, r32 = run(tag, ins, torch.float64, ModelEMA), run(tag, ins, torch.float32, ModelEMA)
        assert r64["step"] == r32["step"] and r64["scales"] == r32["scales"] and r64.get("scale") == r32.get("scale")
        assert r64["updates"] == cfg["updates"] + cfg["steps"]
        out = {"seed": np.int64(seed), "step": np.float32(r64["step"]), "scale_before": np.asarray(r64["scales"], np.float32)}
        if cfg["scaler"]:
            out.update(scale=np.float32(r64["scale"]), growth_tracker=np.int32(r64["tracker"]))
            assert r64["step"] == cfg["steps"] - 1, "the bad step must have been skipped"
        for k, t in ins.items():
            if not k.startswith("g_"):
                out[k] = t.numpy()
        for n, lst in r64["fed"].items():
            out["gs_" + n] = torch.stack(lst).numpy()
            assert out["gs_" + n].dtype == np.float32
        for kind in R.FLOAT_RESULTS:
            num = max(float((r32["res"][kind][n].double() - r64["res"][kind][n]).abs().max()) for n in r64["res"][kind])
            den = max(float(r64["res"][kind][n].abs().max()) for n in r64["res"][kind])
            out[kind + "_fp32_ref_err"] = np.float64(num / den)
            for n, t in r64["res"][kind].items():
                assert t.dtype == torch.float64
                out["%s_%s" % (kind, n)] = t.numpy()
        path = os.path.join(HERE, "opt_step_%s.npz" % tag)
        np.savez_compressed(path, **out)
        print("%-8s seed %d  step %g  scale %s  ref err p %.2e m %.2e v %.2e e %.2e  %d bytes" % (
            tag, seed, r64["step"], r64.get("scale"), out["p_fp32_ref_err"], out["m_fp32_ref_err"], out["v_fp32_ref_err"], out["e_fp32_ref_err"],
            os.path.getsize(path)))


if __name__ == "__main__":
    main()
