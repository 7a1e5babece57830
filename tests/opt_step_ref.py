"""Per-element torch restatement of uni_opt_step (include/unicorn_hip.h): GradScaler.step + torch.optim.AdamW (single-tensor form) +
GradScaler.update + ModelEMA.update over a list of tensors, in the dtype of the tensors it is given, on any device.  It is NOT how the
fixtures were made (tests/golden/make_golden_opt_step.py runs torch.optim.AdamW, torch.amp.GradScaler and the reference's ModelEMA); the
CPU test holds it to them in fp64.  Also here: the cases of the fixtures and their seeded draw.  Data and helpers only; no GPU work at import."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 4099)
SHAPE_4D = (8, 6, 3, 3)
BETAS, EPS, EMA_DECAY = (0.9, 0.999), 1e-8, 0.9998

# tag -> steps, lr, weight decay, scaler (None or dict), step (0-based) that carries the inf and the NaN, EMA counter before the first step
CASES = {
    "plain": dict(steps=4, lr=1e-3, wd=5e-4, scaler=None, bad_step=None, updates=20000),
    "scaled": dict(steps=5, lr=2e-3, wd=5e-4, scaler=dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2), bad_step=2,
                   updates=20000),
    "groups": dict(steps=4, lr=1e-3, wd=5e-4, scaler=None, bad_step=None, updates=300),
    "emaonly": dict(steps=4, lr=1e-3, wd=5e-4, scaler=None, bad_step=None, updates=4000),
}
FLOAT_RESULTS = ("p", "m", "v", "e")


def shapes(tag):
    """the tensor list of every case: name -> (shape, kind); kind = "param" (AdamW + EMA), "nograd" (a parameter that never gets a gradient),
    "fbuf" (float buffer), "ibuf" (integer buffer: not in the operator's list at all)"""
    out = [("t%02d" % i, (n,), "param") for i, n in enumerate(SIZES)] + [("t%02d" % len(SIZES), SHAPE_4D, "param")]
    if tag == "emaonly":
        out += [("frozen", (37,), "nograd"), ("running", (130,), "fbuf"), ("count", (3,), "ibuf")]
    return out


def group_of(tag, i):
    """groups: index -> (lr factor, weight decay factor); `groups` has two lr factors and weight_decay 0 on some tensors"""
    if tag != "groups":
        return 1.0, 1.0
    return (0.1 if i % 3 == 0 else 1.0), (0.0 if i % 2 == 1 else 1.0)


def draw(tag, seed):
    """the seeded draw of a case: fp32 tensors p0 / e0 per entry and the UNSCALED gradients [steps] per parameter"""
    g = torch.Generator().manual_seed(int(seed))
    c = CASES[tag]
    out = {}
    for name, shape, kind in shapes(tag):
        if kind == "ibuf":
            out["p0_" + name] = torch.randint(0, 100, shape, generator=g, dtype=torch.int64)
            continue
        out["p0_" + name] = torch.randn(shape, generator=g) * 0.5
        out["e0_" + name] = out["p0_" + name] + torch.randn(shape, generator=g) * 0.01
        if kind == "param":
            out["g_" + name] = torch.randn((c["steps"],) + tuple(shape), generator=g) * torch.logspace(-3, 0, c["steps"]).view((-1,) + (1,) * len(shape))
    return out


def plant_bad(tag, grads_of_step):
    """the inf and the NaN of the bad step, in different tensors (dict name -> gradient of that step, changed in place)"""
    grads_of_step["g_t07"].view(-1)[11] = float("inf")
    grads_of_step["g_t11"].view(-1)[4098] = float("nan")


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "opt_step_%s.npz" % tag)))


def ema_decay_at(updates, decay=EMA_DECAY):
    return decay * (1 - math.exp(-updates / 2000))


def adamw_ema_step(p, g, m, v, e, state, *, lr, lr_factors, wds, betas=BETAS, eps=EPS, d, scaler=None):
    """ONE call of the operator on lists of tensors (changed in place), per element, in their dtype.  g[i] None: EMA only (m[i], v[i] unused).
    state: dict step (float) and, with a scaler dict, scale (float), tracker (int); changed in place.  -> found_inf (bool)"""
    f32 = np.float32
    inv, found = 1.0, False
    if scaler is not None:
        inv = float(f32(1.0 / float(f32(state["scale"]))))
        for gi in g:
            if gi is not None and not bool(torch.isfinite(gi * inv).all()):
                found = True
    if not found:
        t = state["step"] + 1.0
        bc1, bc2 = 1.0 - betas[0] ** t, 1.0 - betas[1] ** t
        for i, gi in enumerate(g):
            if gi is None:
                continue
            lri = lr * lr_factors[i]
            gh = gi * inv
            p[i].mul_(1.0 - lri * wds[i])
            m[i].add_((gh - m[i]) * (1.0 - betas[0]))
            v[i].mul_(betas[1]).add_((1.0 - betas[1]) * gh * gh)
            p[i].sub_((lri / bc1) * (m[i] / (v[i].sqrt() / math.sqrt(bc2) + eps)))
        state["step"] = t
    for i in range(len(p)):
        e[i].mul_(d)                      # ModelEMA.update's two lines: three roundings
        e[i].add_((1.0 - d) * p[i])
    if scaler is not None:
        if found:
            state["scale"] = float(f32(state["scale"] * scaler["backoff_factor"]))
            state["tracker"] = 0
        else:
            ok = state["tracker"] + 1
            if ok == scaler["growth_interval"]:
                grown = float(f32(state["scale"] * scaler["growth_factor"]))
                if math.isfinite(grown):
                    state["scale"] = grown
                state["tracker"] = 0
            else:
                state["tracker"] = ok
    return found


def run_case(tag, c, dtype):
    """the restatement over all steps of fixture `c` (its stored inputs) -> dict of final lists + scalars, like the fixture's results"""
    cfg = CASES[tag]
    ent = [(n, s, k) for n, s, k in shapes(tag) if k != "ibuf"]
    p = [torch.from_numpy(c["p0_" + n]).to(dtype) for n, _, _ in ent]
    e = [torch.from_numpy(c["e0_" + n]).to(dtype) for n, _, _ in ent]
    m = [torch.zeros_like(x) for x in p]
    v = [torch.zeros_like(x) for x in p]
    lrf = [group_of(tag, i)[0] for i in range(len(ent))]
    wds = [cfg["wd"] * group_of(tag, i)[1] for i in range(len(ent))]
    st = {"step": 0.0}
    if cfg["scaler"]:
        st.update(scale=cfg["scaler"]["init_scale"], tracker=0)
    skipped = []
    for k in range(cfg["steps"]):
        g = [torch.from_numpy(c["gs_" + n][k]).to(dtype) if kind == "param" else None for n, _, kind in ent]
        d = ema_decay_at(cfg["updates"] + k + 1)
        skipped.append(adamw_ema_step(p, g, m, v, e, st, lr=cfg["lr"], lr_factors=lrf, wds=wds, d=d, scaler=cfg["scaler"]))
    return dict(names=[n for n, _, _ in ent], kinds=[k for _, _, k in ent], p=p, m=m, v=v, e=e, step=st["step"], scale=st.get("scale"),
                tracker=st.get("tracker"), skipped=skipped)


# ---- the ragged list of the GPU tests (tests/test_opt_step_gpu.py, tests/test_opt_step_bounds_gpu.py) ---------------------------------------
ARRAYS = ("p", "g", "m", "v", "e")
PAD = 5                    # elements of the enclosing storage behind every view


def ragged_spec(ch):
    """entries of the ragged list for chunk size `ch`: n elements, off = where the view of each array (p, g, m, v, e) starts in its enclosing
    storage (elements), cl = a channels_last 4-D shape, grad = False: EMA only.  Sizes around the chunk, 300 tiny tensors, views 1 / 2 / 3
    elements into a larger storage (p alone: the scalar form; all five: the 16-byte form with a head in every chunk), a gradient that alone
    is misaligned, a channels_last parameter, EMA-only entries in both forms."""
    import random
    rng = random.Random(5)
    spec = [dict(n=n) for n in (0, 1, 3, 4, 5, ch - 1, ch, ch + 1, 2 * ch + 3, 3 * ch)]
    spec += [dict(n=rng.randint(1, 7)) for _ in range(300)]
    spec += [dict(n=1000 + k, off=(k, 0, 0, 0, 0)) for k in (1, 2, 3)]
    spec += [dict(n=2 * ch + 1 + k, off=(k,) * 5) for k in (1, 2, 3)]
    spec += [dict(n=777, off=(0, 1, 0, 0, 0))]
    spec += [dict(n=120, cl=(2, 5, 3, 4))]
    spec += [dict(n=50, grad=False), dict(n=ch + 2, grad=False, off=(2, 0, 0, 0, 3))]
    for s in spec:
        s.setdefault("off", (0,) * 5)
        s.setdefault("grad", True)
        s.setdefault("cl", None)
    return spec


def ragged_draw(spec, seed, grad_scale=1.0):
    """-> per array a list of fp32 CPU storages (off + n + PAD elements each; None where the entry has no such array)"""
    g = torch.Generator().manual_seed(seed)
    out = {a: [] for a in ARRAYS}
    for s in spec:
        for j, a in enumerate(ARRAYS):
            if a in ("g", "m", "v") and not s["grad"]:
                out[a].append(None)
                continue
            x = torch.randn(s["off"][j] + s["n"] + PAD, generator=g)
            x = {"p": x * 0.5, "g": x * 0.3 * grad_scale, "m": x * 0.05, "v": x * x * 1e-3, "e": x * 0.5}[a]
            out[a].append(x)
    return out


def ragged_views(spec, stor):
    """the entries' tensors inside the storages `stor` (any device): per array a list of views (None = absent)"""
    out = {a: [] for a in ARRAYS}
    for i, s in enumerate(spec):
        for j, a in enumerate(ARRAYS):
            st = stor[a][i]
            if st is None:
                out[a].append(None)
                continue
            v = st[s["off"][j]:s["off"][j] + s["n"]]
            if s["cl"]:
                N, C, H, W = s["cl"]
                v = v.as_strided((N, C, H, W), (C * H * W, 1, W * C, C), v.storage_offset())
            out[a].append(v)
    return out
