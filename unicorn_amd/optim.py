"""The tail of the reference's training iteration as ONE operator (uni_opt_step, include/unicorn_hip.h):

    self.scaler.step(self.optimizer)      # torch.optim.AdamW over every parameter (exp/unicorn_track.py:380-381)
    self.scaler.update()
    self.ema_model.update(self.model)     # utils/ema.py:50-63

`StepPlan` owns the two device tables of the operator (tensor table + block map) and their upload; `FusedAdamWEMA` is the optimizer-shaped
wrapper a trainer binds to; `unicorn_amd.ops.adamw_ema_step` is the functional form over lists of tensors.

Upload: the tables are built once.  Every step compares the current data_ptr()s with the uploaded ones; only when they differ (or a
group's factor / weight_decay changed) a new image goes through one of two pinned host buffers and an asynchronous copy on the current
stream.  A pinned buffer is reused only after the event recorded behind its copy has completed.  In steady state the host never waits on the
device and uploads nothing; the learning rate, the betas and the EMA decay travel as scalars of the call.  All steps of one plan are
expected on one stream.

Deviations from the three lines, both documented in the header: the gradients are left scaled (`p.grad` is not unscaled in place), and the
list shares ONE step word (torch keeps one per parameter; they differ only when a parameter has no gradient in some iterations)."""
import math

import numpy as np
import torch

from . import _lib as L

ENTRY = np.dtype([("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("e", "<u8"), ("n", "<i8"), ("lr_factor", "<f8"), ("wd", "<f4"),
                  ("flags", "<i4")])       # uni_opt_step's table entry, 64 bytes
BLOCK = np.dtype([("tensor", "<i4"), ("chunk", "<u4")])
HAS_GRAD = 1
assert ENTRY.itemsize == 64 and BLOCK.itemsize == 8


def _layout(t):
    """(shape, strides) over the dimensions of size > 1 when `t` is dense and non-overlapping, else None"""
    dims = sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz > 1)
    run = 1
    for st, sz in dims:
        if st != run:
            return None
        run *= sz
    return tuple((sz, st) for sz, st in zip(t.shape, t.stride()) if sz > 1)


def need_cuda(dev, what="adamw_ema_step"):
    if dev is not None and dev.type != "cuda":
        raise ValueError("%s needs HIP device tensors (got a CPU tensor); there is no CPU fallback" % what)


def check_entries(entries, what="adamw_ema_step", device_check=True):
    """entries: (p, g, m, v, e) tuples, g / m / v may be None.  Raises ValueError for everything the operator refuses; touches no library.
    -> the device"""
    names = ("p", "g", "m", "v", "e")
    devs, written = set(), []
    for i, ent in enumerate(entries):
        if len(ent) != 5 or ent[0] is None or ent[4] is None:
            raise ValueError("%s: entry %d needs a parameter and an EMA tensor" % (what, i))
        if ent[1] is not None and (ent[2] is None or ent[3] is None):
            raise ValueError("%s: entry %d has a gradient but no moments" % (what, i))
        ref = None
        for nm, t in zip(names, ent):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise ValueError("%s: entry %d: %s is not a tensor" % (what, i, nm))
            if t.dtype != torch.float32:
                raise ValueError("%s: entry %d: %s has dtype %s; only fp32 parameters, gradients, moments and EMA copies are supported" % (what, i, nm, t.dtype))
            if t.is_sparse or t.layout != torch.strided:
                raise ValueError("%s: entry %d: %s is not a strided tensor" % (what, i, nm))
            devs.add(t.device)
            lay = _layout(t) if t.numel() else ()
            if lay is None:
                raise ValueError("%s: entry %d: %s (shape %s, strides %s) is not dense and non-overlapping" % (what, i, nm, tuple(t.shape), t.stride()))
            if ref is None:
                ref = (tuple(t.shape), lay)
            elif (tuple(t.shape), lay) != ref:
                raise ValueError("%s: entry %d: %s (shape %s, strides %s) does not have the shape and strides of p (%s)"
                                 % (what, i, nm, tuple(t.shape), t.stride(), ref))
    if len(devs) > 1:
        raise ValueError("%s: tensors on different devices %s" % (what, sorted(str(d) for d in devs)))
    for i, ent in enumerate(entries):
        n = ent[0].numel()
        if n:
            for nm, t in zip(names, ent):
                if t is not None and (nm in ("m", "v", "e") or (nm == "p" and ent[1] is not None)):
                    written.append((t.data_ptr(), t.data_ptr() + 4 * n, i, nm))
    written.sort()
    for a, b in zip(written, written[1:]):
        if b[0] < a[1]:
            raise ValueError("%s: the same storage is listed twice (%s of entry %d and %s of entry %d overlap)" % (what, a[3], a[2], b[3], b[2]))
    dev = next(iter(devs)) if devs else None
    if device_check:
        need_cuda(dev, what)
    return dev


class StepPlan:
    """The device tables of uni_opt_step for one list of tensors, and their upload.  `uploads` counts the images sent."""

    def __init__(self):
        self.key = None
        self.uploads = 0
        self.device = None
        self._img = None
        self._pinned = [None, None]
        self._events = [None, None]
        self._turn = 0
        self._call = None        # (table ptr, table bytes, map ptr, map bytes, n tensors, vec chunks, total chunks)

    @staticmethod
    def image(cols, ch, table_bytes):
        """cols: dict of equal-length sequences p, g, m, v, e (addresses, 0 = absent), n, lr_factor, wd, has_grad -> (bytes, map offset,
        n tensors, vec chunks, total chunks).  Pure host arithmetic (tests/test_opt_step_cpu.py runs it without a device)."""
        N = len(cols["n"])
        tab = np.zeros(N, ENTRY)
        for k in ("p", "g", "m", "v", "e"):
            tab[k] = np.asarray(cols[k], dtype=np.uint64)
        tab["n"] = np.asarray(cols["n"], dtype=np.int64)
        tab["lr_factor"] = np.asarray(cols["lr_factor"], dtype=np.float64)
        tab["wd"] = np.asarray(cols["wd"], dtype=np.float32)
        full = np.asarray(cols["has_grad"], dtype=bool) & (tab["g"] != 0) & (tab["m"] != 0) & (tab["v"] != 0)
        tab["flags"] = np.where(full, HAS_GRAD, 0)
        al = tab["p"] & np.uint64(15)
        vec = ((tab["e"] & np.uint64(15)) == al) & ((al & np.uint64(3)) == 0)
        for k in ("g", "m", "v"):
            vec &= ~full | ((tab[k] & np.uint64(15)) == al)
        chunks = (tab["n"] + (ch - 1)) // ch
        order = np.concatenate([np.nonzero(vec)[0], np.nonzero(~vec)[0]]).astype(np.int64)
        cnt = chunks[order]
        total = int(cnt.sum())
        if total >= 1 << 31:
            raise ValueError("adamw_ema_step: %d chunks of %d elements exceed the grid limit" % (total, ch))
        bm = np.zeros(total, BLOCK)
        bm["tensor"] = np.repeat(order, cnt)
        bm["chunk"] = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        map_off = table_bytes(N, 0)
        img = np.zeros(table_bytes(N, total), np.uint8)
        img[:N * 64] = tab.view(np.uint8)
        img[map_off:map_off + total * 8] = bm.view(np.uint8)
        return img, map_off, N, int(chunks[vec].sum()), total

    def upload(self, key, cols, device):
        """build the image of `cols` and send it; afterwards `key` is what the device holds"""
        lib = L.lib()
        img, map_off, N, vec_chunks, total = self.image(cols, lib.uni_opt_chunk_elems(), lib.uni_opt_table_bytes)
        need = max(img.size, 256)
        with torch.cuda.device(device):
            if self._img is None or self._img.numel() < need or self._img.device != device:
                self._img = torch.empty(need, dtype=torch.uint8, device=device)
            slot, self._turn = self._turn, self._turn ^ 1
            if self._pinned[slot] is None or self._pinned[slot].numel() < need:
                self._pinned[slot] = torch.empty(need, dtype=torch.uint8).pin_memory()
                self._events[slot] = None
            ev = self._events[slot]
            if ev is not None and not ev.query():        # the copy out of this buffer is still in flight (two uploads in a row): wait for it
                ev.synchronize()
            self._pinned[slot].numpy()[:img.size] = img
            self._img[:img.size].copy_(self._pinned[slot][:img.size], non_blocking=True)       # hipMemcpyAsync on the current stream
            ev = torch.cuda.Event()
            ev.record()
            self._events[slot] = ev
        base = self._img.data_ptr()
        self._call = (base, N * 64, base + map_off, total * 8, N, vec_chunks, total)
        self.key, self.device = key, device
        self.uploads += 1

    def launch(self, step, scaler_words, lr, betas, eps, ema_decay, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        """scaler_words: None or (scale fp32, growth_tracker int32, found_inf fp32) device tensors"""
        tab, tab_bytes, bmap, map_bytes, N, vec_chunks, total = self._call
        sc = scaler_words or (None, None, None)
        with torch.cuda.device(self.device):
            L.check(L.lib().uni_opt_step(tab, tab_bytes, bmap, map_bytes, N, vec_chunks, total, L.ptr(step), L.ptr(sc[0]), L.ptr(sc[1]), L.ptr(sc[2]),
                                         float(lr), float(betas[0]), float(betas[1]), float(eps), float(ema_decay), float(growth_factor),
                                         float(backoff_factor), int(growth_interval), L.stream_ptr()), "uni_opt_step")


def check_state_words(step, scaler_words, device, what="adamw_ema_step"):
    if not isinstance(step, torch.Tensor) or step.dtype != torch.float32 or step.numel() != 1:
        raise ValueError("%s: step must be one fp32 device word (as torch.optim.AdamW keeps it)" % what)
    words = [("step", step, torch.float32)]
    if scaler_words is not None:
        if len(scaler_words) != 3:
            raise ValueError("%s: the scaler's words are (scale, growth_tracker, found_inf)" % what)
        words += [("scale", scaler_words[0], torch.float32), ("growth_tracker", scaler_words[1], torch.int32), ("found_inf", scaler_words[2], torch.float32)]
    for nm, t, dt in words:
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() != 1:
            raise ValueError("%s: %s must be one %s word" % (what, nm, dt))
        if device is not None and t.device != device:
            raise ValueError("%s: %s is on %s, the tensors on %s (different devices)" % (what, nm, t.device, device))


def ema_decay_at(decay, updates):
    """ModelEMA's ramp (utils/ema.py:46)"""
    return decay * (1 - math.exp(-updates / 2000))


class FusedAdamWEMA:
    """scaler.step(optimizer) + scaler.update() + ema_model.update(model) of the reference's trainer in one call, no host synchronisation.

    params_or_model   an nn.Module (one group of all its parameters, as exp/unicorn_track.py:380 builds it) or what torch.optim.AdamW takes
                      (an iterable of parameters or of group dicts with "params" and optionally "lr" / "factor" / "weight_decay")
    ema_model         the reference's ModelEMA object (`.ema`, `.updates`; its counter is kept up to date) or the EMA module itself
    model             needed with a parameter list when the EMA module has floating buffers: ModelEMA averages those too
    scaler            None, or dict(init_scale, growth_factor, backoff_factor, growth_interval) (torch.cuda.amp.GradScaler's arguments)

    Every floating entry of the EMA module's state_dict is averaged; parameters of the groups that require a gradient get AdamW; integer
    entries are left alone, as the reference leaves them.  fp32 only."""

    def __init__(self, params_or_model, ema_model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, ema_decay=0.9999, ema_updates=0,
                 scaler=None, model=None):
        if isinstance(params_or_model, torch.nn.Module):
            model = params_or_model
            groups = [{"params": [p for _, p in model.named_parameters()]}]
        else:
            groups = list(params_or_model)
            if not groups:
                raise ValueError("FusedAdamWEMA: empty parameter list")
            if not isinstance(groups[0], dict):
                groups = [{"params": groups}]
            groups = [dict(g, params=list(g["params"])) for g in groups]
        for g in groups:
            g.setdefault("lr", lr)
            g.setdefault("weight_decay", weight_decay)
            g.setdefault("betas", tuple(betas))
            g.setdefault("eps", eps)
            if tuple(g["betas"]) != tuple(betas) or g["eps"] != eps:
                raise ValueError("FusedAdamWEMA: betas and eps are scalars of the call; groups cannot differ in them")
        self.param_groups = groups
        self.betas, self.eps, self.ema_decay = (float(betas[0]), float(betas[1])), float(eps), float(ema_decay)
        self._ema_obj = ema_model if hasattr(ema_model, "ema") and hasattr(ema_model, "updates") else None
        ema_module = self._ema_obj.ema if self._ema_obj is not None else ema_model
        if not isinstance(ema_module, torch.nn.Module):
            raise ValueError("FusedAdamWEMA: ema_model is neither a ModelEMA object (.ema, .updates) nor a module")
        self.ema_updates = int(self._ema_obj.updates) if self._ema_obj is not None and not ema_updates else int(ema_updates)
        group_of = {}
        for gi, g in enumerate(groups):
            for p in g["params"]:
                if id(p) in group_of:
                    raise ValueError("FusedAdamWEMA: the same storage is listed twice (a parameter appears in two groups)")
                group_of[id(p)] = gi
        esd = ema_module.state_dict()
        if model is not None:
            msd = model.state_dict(keep_vars=True)
            pairs = [(msd[k], v) for k, v in esd.items() if v.dtype.is_floating_point]
        else:
            eparams = list(ema_module.parameters())
            flat = [p for g in groups for p in g["params"]]
            if len(eparams) != len(flat) or any(b.dtype.is_floating_point for b in ema_module.buffers()):
                raise ValueError("FusedAdamWEMA: pass model= with a parameter list: the EMA module has floating buffers (ModelEMA averages them) "
                                 "or a different number of parameters")
            pairs = list(zip(flat, eparams))
        missing = set(group_of) - {id(s) for s, _ in pairs}
        if missing:
            raise ValueError("FusedAdamWEMA: %d parameter(s) of the groups have no entry in the EMA module" % len(missing))
        # entries in the EMA state_dict's order; src = the model's tensor, AdamW candidates are the grouped parameters that require a gradient
        self._src = [s for s, _ in pairs]
        self._ema = [e.detach() for _, e in pairs]
        self._group = [group_of.get(id(s), -1) if getattr(s, "requires_grad", False) else -1 for s in self._src]
        self._m = [torch.zeros_like(s, memory_format=torch.preserve_format) if gi >= 0 else None for s, gi in zip(self._src, self._group)]
        self._v = [torch.zeros_like(s, memory_format=torch.preserve_format) if gi >= 0 else None for s, gi in zip(self._src, self._group)]
        check_entries([(s.detach(), None, m, v, e) for s, m, v, e in zip(self._src, self._m, self._v, self._ema)], "FusedAdamWEMA")
        dev = self._src[0].device if self._src else torch.device("cuda")
        self._step = torch.zeros((), dtype=torch.float32, device=dev)
        self.scaler = None
        self._words = None
        if scaler is not None:
            sc = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
            unknown = set(scaler) - set(sc)
            if unknown:
                raise ValueError("FusedAdamWEMA: unknown scaler argument(s) %s" % sorted(unknown))
            sc.update(scaler)
            self.scaler = sc
            self._words = (torch.full((), float(sc["init_scale"]), dtype=torch.float32, device=dev), torch.zeros((), dtype=torch.int32, device=dev),
                           torch.zeros((), dtype=torch.float32, device=dev))
        self._n = [s.numel() for s in self._src]
        self._mp = [0 if m is None else m.data_ptr() for m in self._m]
        self._vp = [0 if v is None else v.data_ptr() for v in self._v]
        self._factors = None
        self.plan = StepPlan()

    # -- the trainer's lines -------------------------------------------------------------------------------------------
    def scale(self, loss):
        """scaler.scale(loss): the product with the device scale word (no read-back)"""
        return loss if self._words is None else loss * self._words[0]

    def zero_grad(self, set_to_none=False):
        """zeroes in place by default: the gradients keep their addresses and the next step uploads nothing"""
        for s, gi in zip(self._src, self._group):
            if gi >= 0 and s.grad is not None:
                if set_to_none:
                    s.grad = None
                else:
                    s.grad.detach_()
                    s.grad.requires_grad_(False)
                    s.grad.zero_()

    def _lr_split(self):
        """-> (lr of the call, per-group factor): the group's learning rate is lr x factor.  A declared "factor" is used when the group's lr
        is consistent with it (the trainer writes lr * factor); otherwise the ratio to the first group, held to the uploaded value within 1e-12."""
        g0 = self.param_groups[0]
        base = g0["lr"] / g0.get("factor", 1.0) if g0.get("factor", 1.0) else g0["lr"]
        out = []
        for i, g in enumerate(self.param_groups):
            f = float(g.get("factor", 1.0))
            if abs(g["lr"] - base * f) > 1e-12 * abs(g["lr"]):
                f = g["lr"] / base if base else 0.0
                old = self._factors[i] if self._factors else None
                if old is not None and abs(f - old) <= 1e-12 * abs(old):
                    f = old
            out.append(f)
        return float(base), tuple(out)

    @torch.no_grad()
    def step(self):
        lr, factors = self._lr_split()
        wds = tuple(float(g["weight_decay"]) for g in self.param_groups)
        pp = [s.data_ptr() for s in self._src]
        gp = [s.grad.data_ptr() if gi >= 0 and s.grad is not None else 0 for s, gi in zip(self._src, self._group)]
        ep = [e.data_ptr() for e in self._ema]
        key = (pp, gp, ep, factors, wds)
        if key != self.plan.key:
            dev = check_entries([(s.detach(), s.grad if g_ else None, m, v, e) for s, g_, m, v, e in zip(self._src, gp, self._m, self._v, self._ema)],
                                "FusedAdamWEMA.step")
            check_state_words(self._step, self._words, dev, "FusedAdamWEMA.step")
            cols = dict(p=pp, g=gp, m=self._mp, v=self._vp, e=ep, n=self._n, lr_factor=[factors[gi] if gi >= 0 else 1.0 for gi in self._group],
                        wd=[wds[gi] if gi >= 0 else 0.0 for gi in self._group], has_grad=[gi >= 0 for gi in self._group])
            self.plan.upload(key, cols, dev)
            self._factors = factors
        self.ema_updates += 1
        if self._ema_obj is not None:
            self._ema_obj.updates = self.ema_updates
        sc = self.scaler or {}
        self.plan.launch(self._step, self._words, lr, self.betas, self.eps, ema_decay_at(self.ema_decay, self.ema_updates),
                         sc.get("growth_factor", 2.0), sc.get("backoff_factor", 0.5), sc.get("growth_interval", 2000))

    # -- checkpoints (the only place that reads back) --------------------------------------------------------------------
    def _adamw_params(self):
        """the grouped parameters in torch.optim's numbering -> {id(param): entry index}"""
        at = {id(s): i for i, s in enumerate(self._src)}
        return [[at[id(p)] for p in g["params"]] for g in self.param_groups]

    def state_dict(self):
        """torch.optim.AdamW's own format (state: step / exp_avg / exp_avg_sq per parameter index; param_groups with its keys)"""
        tmpl = torch.optim.AdamW([dict(g) for g in self.param_groups], lr=1e-3, betas=self.betas, eps=self.eps)
        sd = tmpl.state_dict()
        stepped = float(self._step.item())
        state, k = {}, 0
        for idx in self._adamw_params():
            for i in idx:
                if self._group[i] >= 0 and stepped > 0:
                    state[k] = {"step": torch.tensor(stepped, dtype=torch.float32), "exp_avg": self._m[i].clone(), "exp_avg_sq": self._v[i].clone()}
                k += 1
        sd["state"] = state
        return sd

    def load_state_dict(self, sd):
        """resumes from a torch.optim.AdamW state_dict (the reference checkpoint's "optimizer" entry)"""
        idx = self._adamw_params()
        if len(sd["param_groups"]) != len(idx) or any(len(g["params"]) != len(i) for g, i in zip(sd["param_groups"], idx)):
            raise ValueError("FusedAdamWEMA.load_state_dict: the groups of the state_dict do not fit the optimizer's")
        steps = {float(s["step"]) for s in sd["state"].values()}
        if len(steps) > 1:
            raise ValueError("FusedAdamWEMA.load_state_dict: per-parameter step counts differ (%s); the operator keeps one step" % sorted(steps))
        for g, mine, ii in zip(sd["param_groups"], self.param_groups, idx):
            if g.get("amsgrad") or g.get("maximize"):
                raise ValueError("FusedAdamWEMA.load_state_dict: amsgrad / maximize are not supported")
            if tuple(g.get("betas", self.betas)) != self.betas or g.get("eps", self.eps) != self.eps:
                raise ValueError("FusedAdamWEMA.load_state_dict: betas / eps differ from the optimizer's")
            for k in ("lr", "weight_decay", "factor", "initial_lr"):
                if k in g:
                    mine[k] = g[k]
            for k, i in zip(g["params"], ii):
                st = sd["state"].get(k)
                if self._group[i] < 0:
                    continue
                if st is None:
                    self._m[i].zero_()
                    self._v[i].zero_()
                else:
                    self._m[i].copy_(st["exp_avg"].reshape(self._m[i].shape))
                    self._v[i].copy_(st["exp_avg_sq"].reshape(self._v[i].shape))
        self._step.fill_(steps.pop() if steps else 0.0)

    def scaler_state_dict(self):
        """torch.cuda.amp.GradScaler.state_dict()'s keys"""
        if self.scaler is None:
            return {}
        return {"scale": float(self._words[0].item()), "growth_factor": self.scaler["growth_factor"], "backoff_factor": self.scaler["backoff_factor"],
                "growth_interval": self.scaler["growth_interval"], "_growth_tracker": int(self._words[1].item())}

    def load_scaler_state_dict(self, sd):
        if self.scaler is None or not sd:
            return
        for k in ("growth_factor", "backoff_factor", "growth_interval"):
            self.scaler[k] = sd[k]
        self._words[0].fill_(float(sd["scale"]))
        self._words[1].fill_(int(sd["_growth_tracker"]))
