"""The tail of the reference's training iteration (unicorn/core/trainer.py:260-275: scaler.step(optimizer), scaler.update(),
ema_model.update(model)) over the tensor list of a whole model, taken from tests/golden/state_spec_<name>.json with random values:

  (a) unicorn_amd.optim.FusedAdamWEMA.step()                                    -- uni_opt_step, one pass
  (b) the three lines as the reference writes them: torch.optim.AdamW with its defaults, torch.cuda.amp.GradScaler, and the EMA loop
      (three elementwise launches per state-dict entry)
  (c) the best stock form: AdamW(fused=True) handed grad_scale / found_inf by the scaler, torch._foreach_mul_ / _foreach_add_ for the EMA

on the same GPU in the same run, each on its own copy of the state (allocated and freed in turn).  HIP events around every call, warm-up
first, median of the timed calls; kernel launches of one call by torch.profiler; host synchronisations of one call as the warnings of
torch.cuda.set_sync_debug_mode("warn"); peak memory of one call; effective bandwidth of (a) against 10 passes over the parameters
(read p, g, m, v, e, write p, m, v, e, + the gradient pass of the non-finite check).

    python tools/opt_step_bench.py [--model unicorn_track_large_mask] [--runs 20] [--out profiles/opt_step.txt]
"""
import argparse
import copy
import json
import os
import statistics
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from unicorn_amd import optim  # noqa: E402

LR, WD, DECAY = 1e-3, 5e-4, 0.9998


class Bag(torch.nn.Module):
    def __init__(self, shapes, dev):
        super().__init__()
        g = torch.Generator(device=dev).manual_seed(0)
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(tuple(s), generator=g, device=dev) * 0.1) for s in shapes])


def fill_grads(net, seed):
    g = torch.Generator(device=net.w[0].device).manual_seed(seed)
    for p in net.w:
        if p.grad is None:
            p.grad = torch.empty_like(p)
        p.grad.copy_(torch.randn(p.shape, generator=g, device=p.device) * 0.01)


def ema_loop(ema_sd, model_sd, d):
    """(b): every floating entry scaled, then the model's entry added through a temporary"""
    for k, v in ema_sd.items():
        if v.dtype.is_floating_point:
            v.mul_(d)
            v.add_(model_sd[k].detach() * (1.0 - d))


def measure(call, runs, warmup=3):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    torch.cuda.reset_peak_memory_stats()
    call()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        call()
        torch.cuda.synchronize()
    launches = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
                   and "memset" not in e.name.lower())
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            call()
        syncs = sum(1 for x in w if "synchroniz" in str(x.message).lower())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return dict(min=min(ts), median=statistics.median(ts), peak=peak, launches=launches, syncs=syncs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="unicorn_track_large_mask")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    spec = json.load(open(os.path.join(ROOT, "tests", "golden", "state_spec_%s.json" % a.model)))
    shapes = [s for s in spec.values()]
    numel = sum(int(torch.Size(s).numel()) for s in shapes)
    small = sum(1 for s in shapes if torch.Size(s).numel() < 4096)
    lines = ["fused AdamW + loss scale + EMA step, fp32 -- tools/opt_step_bench.py on %s" % torch.cuda.get_device_name(0),
             "tensor list of %s: %d tensors, %d elements (%.2f GB per array, 5 arrays), %d tensors under 4096 elements" % (
                 a.model, len(shapes), numel, 4 * numel / 1e9, small),
             "times: HIP events around every call, 3 warm-up calls, min / median of %d timed calls; launches by torch.profiler; host synchronisations = "
             "warnings of torch.cuda.set_sync_debug_mode(\"warn\") in one call" % a.runs, ""]
    res = {}

    # (a)
    net = Bag(shapes, dev)
    ema = copy.deepcopy(net).eval()
    opt = optim.FusedAdamWEMA(net, ema, lr=LR, weight_decay=WD, ema_decay=DECAY, ema_updates=20000, scaler=dict(init_scale=1.0, growth_interval=2000))
    fill_grads(net, 1)
    res["a"] = measure(opt.step, a.runs)
    res["a"]["uploads"] = opt.plan.uploads
    del net, ema, opt
    torch.cuda.empty_cache()

    # (b)
    net = Bag(shapes, dev)
    ema = copy.deepcopy(net).eval()
    topt = torch.optim.AdamW([{"params": [p for _, p in net.named_parameters()]}], lr=LR, weight_decay=WD)
    scaler = torch.cuda.amp.GradScaler(init_scale=1.0)
    fill_grads(net, 1)
    one = torch.ones((), device=dev)

    def ref_lines():
        scaler.scale(one)
        scaler.step(topt)
        scaler.update()
        ema_loop(ema.state_dict(), net.state_dict(), DECAY)
    res["b"] = measure(ref_lines, a.runs)
    del net, ema, topt, scaler
    torch.cuda.empty_cache()

    # (c)
    net = Bag(shapes, dev)
    ema = copy.deepcopy(net).eval()
    fopt = torch.optim.AdamW([{"params": [p for _, p in net.named_parameters()]}], lr=LR, weight_decay=WD, fused=True)
    scaler = torch.cuda.amp.GradScaler(init_scale=1.0)
    fill_grads(net, 1)
    ps, es = [p.detach() for p in net.w], [p.detach() for p in ema.w]

    def stock():
        scaler.scale(one)
        scaler.step(fopt)
        scaler.update()
        torch._foreach_mul_(es, DECAY)
        torch._foreach_add_(es, ps, alpha=1.0 - DECAY)
    res["c"] = measure(stock, a.runs)
    del net, ema, fopt, scaler, ps, es
    torch.cuda.empty_cache()

    for k, name in (("a", "(a) uni_opt_step          "), ("b", "(b) reference's lines     "), ("c", "(c) fused AdamW + foreach ")):
        r = res[k]
        lines.append("  %s min %9.4f ms   median %9.4f ms   kernel launches %5d   host synchronisations %d   peak %8.1f MB" % (
            name, r["min"], r["median"], r["launches"], r["syncs"], r["peak"] / 1e6))
    gb = 10 * 4 * numel / 1e9
    lines += ["",
              "  (b) / (a) median %.2f x; (c) / (a) median %.2f x" % (res["b"]["median"] / res["a"]["median"], res["c"]["median"] / res["a"]["median"]),
              "  (a): %.2f GB in 10 passes -> %.2f TB/s effective; table uploads over all %d calls: %d" % (
                  gb, gb / res["a"]["median"], a.runs + 6, res["a"]["uploads"])]
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
