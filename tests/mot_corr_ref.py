"""The MOT instance-contrastive loss (unicorn/models/unicorn.py:407-466) restated in torch, in two forms, plus the cases, the draws and the
fixture rule of tests/golden/mot_corr_*.npz (written by tests/golden/make_golden_mot_corr.py from the reference's own function).

  loss_loop        the shape of the reference: a Python loop over the id pairs, one grid_sample per instance, two cross-entropies
  loss_vectorised  a broadcast compare for the labels and one grid_sample per frame and sample

Both return the (B,) per-sample losses in the dtype of the embeddings; autograd gives the gradients.  The coordinates up to the normalised
grid value are fp32 whatever the dtype of the maps (targets are .float()), the grid is cast to the maps' dtype for grid_sample.  A sample
without an instance in one of its frames, where the reference raises, gives NaN (the operator's rule).

Fixture rule: no sampled coordinate within MARGIN px of an integer unless the clamp makes it exactly 0 or size-1; for grid_sample=False no
c / s within MARGIN of a half-integer unless it is exactly one."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-3

# tag -> B, C, H, W, M, bidirect, grid_sample, drawn as (the inputs of `unidir` are those of `plain`)
CASES = {
    "plain": (2, 128, 7, 11, 12, True, True, "plain"),
    "unidir": (2, 128, 7, 11, 12, False, True, "plain"),
    "nearest": (2, 32, 6, 9, 10, True, False, "nearest"),
    "edge": (1, 24, 5, 7, 10, True, True, "edge"),
    "crowd": (1, 128, 10, 16, 100, True, True, "crowd"),
    "nomatch": (3, 16, 5, 6, 6, True, True, "nomatch"),
}
S = 8
RESULTS = ("loss", "g_embed_0", "g_embed_1")
# An fp32 result has a rounding error of up to 2^-24 of its own size, 2^-25 on average over a binade.  A stored fp32-vs-fp64 deviation
# of the reference below that is an accident of rounding (a (1,) loss is ONE rounding), not the error of an fp32 evaluation, and no
# yardstick: such a draw lacks what every case needs and is redrawn.  Above 1e-5 something else than rounding is at work.
REF_ERR_MIN, REF_ERR_MAX = 2.0 ** -25, 1e-5


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "mot_corr_%s.npz" % tag)))


# ---------------------------------------------------------------------------------------------------------------- the two restatements
def _counts(targets):
    ids = targets.float()[..., 5]
    return ids, (ids != 0).sum(-1).tolist()                        # one read for the whole batch


def _grid(centres, H, W, s):
    """centres (n, 2) fp32 (cx, cy) in input pixels -> (n, 2) fp32 normalised grid"""
    c = centres / s - 0.5
    gx = (torch.clamp(c[:, 0], min=0, max=W - 1) / (W - 1) - 0.5) * 2.0
    gy = (torch.clamp(c[:, 1], min=0, max=H - 1) / (H - 1) - 0.5) * 2.0
    return torch.stack([gx, gy], dim=-1)


def _nearest(centres, H, W, s):
    c = centres / s
    return torch.round(torch.clamp(c[:, 0], min=0, max=W - 1)).long(), torch.round(torch.clamp(c[:, 1], min=0, max=H - 1)).long()


def _ce(sim, label):
    return F.cross_entropy(sim, label, ignore_index=-1)


def loss_loop(embed_0, embed_1, targets, s=S, bidirect=True, grid_sample=True):
    B, _, H, W = embed_0.shape
    t = targets.float()
    ids, n = _counts(t)
    dev = embed_0.device
    out = []
    for b in range(B):
        n0, n1 = n[b]
        if n0 == 0 or n1 == 0:
            out.append(embed_0.new_full((), float("nan")))
            continue
        id0, id1 = ids[b, 0].tolist(), ids[b, 1].tolist()
        row, col = [-1] * n0, [-1] * n1
        for i in range(n0):
            for j in range(n1):
                if id0[i] == id1[j]:
                    row[i] = j
                    col[j] = i
                    break
        feats = []
        for f, (emb, k) in enumerate(((embed_0, n0), (embed_1, n1))):
            rows = []
            for i in range(k):
                c = t[b, f, i:i + 1, 1:3]
                if grid_sample:
                    g = _grid(c, H, W, s).to(emb.dtype).view(1, 1, 1, 2)
                    rows.append(F.grid_sample(emb[b:b + 1], g, mode="bilinear", padding_mode="border", align_corners=False).reshape(-1))
                else:
                    x, y = _nearest(c, H, W, s)
                    rows.append(emb[b, :, y[0], x[0]])
            feats.append(torch.stack(rows))
        sim = feats[0] @ feats[1].t()
        lr = _ce(sim, torch.tensor(row, device=dev))
        out.append(0.5 * (lr + _ce(sim.t(), torch.tensor(col, device=dev))) if bidirect else lr)
    return torch.stack(out)


def labels_vectorised(id0, id1):
    """id0 (n0,), id1 (n1,) -> row (n0,), col (n1,) int64"""
    n0, n1 = id0.shape[0], id1.shape[0]
    a0, a1 = torch.arange(n0, device=id0.device), torch.arange(n1, device=id0.device)
    eq = id0[:, None] == id1[None, :]
    first = torch.where(eq, a1[None, :], torch.full_like(a1, n1)[None, :]).min(dim=1).values
    row = torch.where(first < n1, first, torch.full_like(first, -1))
    col = torch.where(row[:, None] == a1[None, :], a0[:, None], torch.full_like(a0, -1)[:, None]).max(dim=0).values
    return row, col


def sample_vectorised(emb_b, centres, s, grid_sample):
    """emb_b (1, C, H, W), centres (n, 2) -> (n, C)"""
    _, _, H, W = emb_b.shape
    if grid_sample:
        g = _grid(centres, H, W, s).to(emb_b.dtype).view(1, 1, -1, 2)
        return F.grid_sample(emb_b, g, mode="bilinear", padding_mode="border", align_corners=False)[0, :, 0].t()
    x, y = _nearest(centres, H, W, s)
    return emb_b[0][:, y, x].t()


def loss_vectorised(embed_0, embed_1, targets, s=S, bidirect=True, grid_sample=True):
    B = embed_0.shape[0]
    t = targets.float()
    ids, n = _counts(t)
    out = []
    for b in range(B):
        n0, n1 = n[b]
        if n0 == 0 or n1 == 0:
            out.append(embed_0.new_full((), float("nan")))
            continue
        row, col = labels_vectorised(ids[b, 0, :n0], ids[b, 1, :n1])
        e0 = sample_vectorised(embed_0[b:b + 1], t[b, 0, :n0, 1:3], s, grid_sample)
        e1 = sample_vectorised(embed_1[b:b + 1], t[b, 1, :n1, 1:3], s, grid_sample)
        sim = e0 @ e1.t()
        out.append(0.5 * (_ce(sim, row) + _ce(sim.t(), col)) if bidirect else _ce(sim, row))
    return torch.stack(out)


def loss_and_grads(fn, embed_0, embed_1, targets, grad_loss, bidirect, grid_sample, s=S):
    """-> {loss (B,), g_embed_0, g_embed_1} for upstream grad_loss; a NaN loss contributes the zero gradient autograd gives it"""
    e0, e1 = embed_0.detach().clone().requires_grad_(True), embed_1.detach().clone().requires_grad_(True)
    loss = fn(e0, e1, targets, s, bidirect, grid_sample)
    loss.backward(grad_loss.to(loss.dtype))
    z = torch.zeros_like
    return {"loss": loss.detach(), "g_embed_0": z(e0) if e0.grad is None else e0.grad, "g_embed_1": z(e1) if e1.grad is None else e1.grad}


# ---------------------------------------------------------------------------------------------------------------- draws and the rule
def _centres(g, k, size, inside):
    """k box centres along an axis of `size` map pixels.  Default: a 1/4 px raster shifted by 1/8 px inside the image (c / 8 - 0.5 is then an
    odd multiple of 1/64, which the scale size / (size - 1) rarely takes to an integer).  inside: the centre whose SAMPLED position is
    cell + 0.05 .. cell + 0.95, so that a large draw keeps the fixture rule by construction"""
    if not inside:
        return torch.randint(0, 4 * S * size, (k,), generator=g).float() / 4 + 0.125
    pos = torch.randint(0, size - 1, (k,), generator=g).double() + 0.05 + 0.9 * torch.rand(k, generator=g, dtype=torch.float64)
    return (S * ((pos + 0.5) * (size - 1) / size + 0.5)).float()


def _rows(g, ids, H, W, M, inside=False):
    """(M, 6) rows: the ids given, centres by _centres, zeros behind"""
    t = torch.zeros(M, 6)
    k = len(ids)
    t[:k, 5] = torch.tensor(ids, dtype=torch.float32)
    t[:k, 1] = _centres(g, k, W, inside)
    t[:k, 2] = _centres(g, k, H, inside)
    t[:k, 3:5] = 8 + torch.randint(0, 160, (k, 2), generator=g).float() / 4
    return t


def draw(kind, seed, shape=None):
    """-> embed_0, embed_1 (B, C, H, W), targets (B, 2, M, 6), grad_loss (B,), all fp32; shape: (B, C, H, W, M) for the kind `large`"""
    B, C, H, W, M = CASES[kind][:5] if shape is None else shape
    g = torch.Generator().manual_seed(seed)
    e0, e1 = 0.5 * torch.randn(B, C, H, W, generator=g), 0.5 * torch.randn(B, C, H, W, generator=g)
    grad_loss = torch.randn(B, generator=g)
    targets = torch.zeros(B, 2, M, 6)
    for b in range(B):
        if kind in ("plain", "nearest"):
            n0, n1 = (int(v) for v in torch.randint(7, 10, (2,), generator=g))
            pool = (torch.randperm(14, generator=g) + 1).tolist()
            id0, id1 = pool[:n0], pool[3:3 + n1]                                  # partly shared ids
            id1 = [id1[i] for i in torch.randperm(n1, generator=g).tolist()]
        elif kind == "large":                                                     # nearly full frames, most ids shared
            n0, n1 = (M - int(v) for v in torch.randint(0, M // 5 + 1, (2,), generator=g))
            pool = (torch.randperm(M + M // 4, generator=g) + 1).tolist()
            id0, id1 = pool[:n0], pool[M // 8:M // 8 + n1]
            id1 = [id1[i] for i in torch.randperm(n1, generator=g).tolist()]
        elif kind == "crowd":
            id0 = (torch.randperm(100, generator=g) + 1).tolist()
            id1 = (torch.randperm(110, generator=g) + 1).tolist()[:97]
        elif kind == "nomatch":
            id0, id1 = ([1, 2, 3, 4], [3, 9, 1]) if b != 1 else ([1, 2, 3], [4, 5, 6, 7])
        elif kind == "edge":
            # n0 = 6 (a zero id among the first six rows, the id 11 behind them is dropped, 5 repeated), n1 = 5 (9 repeated)
            id0, id1 = [3, 5, 0, 5, 7, 9, 11], [5, 3, 9, 9, 4]
        else:
            raise KeyError(kind)
        targets[b, 0], targets[b, 1] = _rows(g, id0, H, W, M, kind == "large"), _rows(g, id1, H, W, M, kind == "large")
        if kind == "nearest":                                                     # c / s exactly k + 0.5, k even and odd, both axes
            targets[b, 0, 0, 1:3] = torch.tensor([S * 2.5, S * 3.5])
            targets[b, 0, 1, 1:3] = torch.tensor([S * 5.5, S * 0.5])
            targets[b, 1, 0, 1:3] = torch.tensor([S * 1.5, S * 4.5])
            targets[b, 1, 1, 1:3] = torch.tensor([S * 6.5, S * 2.5])
        if kind == "edge":
            targets[b, 0, 0, 1:3] = torch.tensor([-20.25, 13.25])                 # left of the image
            targets[b, 0, 1, 1:3] = torch.tensor([S * W + 30.5, 21.75])           # right of it
            targets[b, 0, 3, 1:3] = torch.tensor([17.25, -9.5])                   # above
            targets[b, 1, 0, 1:3] = torch.tensor([25.75, S * H + 11.25])          # below
            targets[b, 1, 1, 1:3] = torch.tensor([-3.0, -7.0])                    # the top-left corner, both clamps
            targets[b, 1, 2, 1:3] = torch.tensor([30.25, 18.5])                   # two instances in one cell
            targets[b, 1, 3, 1:3] = torch.tensor([31.75, 19.25])
    return e0, e1, targets, grad_loss


def sampled_coordinates(targets, H, W, grid_sample, s=S):
    """the positions the instances are sampled at, in fp64 from the fp32 grid (grid_sample) or c / s in fp32 (otherwise): list of
    (b, f, i, x, y, clamped_x, clamped_y) for the instances in use"""
    t = targets.float()
    _, n = _counts(t)
    out = []
    for b, nb in enumerate(n):
        for f in range(2):
            for i in range(nb[f]):
                c = t[b, f, i:i + 1, 1:3]
                if grid_sample:
                    g = _grid(c, H, W, s).double()[0]
                    x, y = float(((g[0] + 1) * W - 1) / 2), float(((g[1] + 1) * H - 1) / 2)
                    cl = (x <= 0 or x >= W - 1, y <= 0 or y >= H - 1)             # the centre clamp or grid_sample's border clip acts
                    x, y = min(max(x, 0.0), W - 1.0), min(max(y, 0.0), H - 1.0)
                else:
                    q = c / s
                    x, y = float(q[0, 0]), float(q[0, 1])
                    cl = (x <= 0 or x >= W - 1, y <= 0 or y >= H - 1)
                out.append((b, f, i, x, y, cl[0], cl[1]))
    return out


def rule_violations(targets, H, W, grid_sample, s=S):
    """instances that break the fixture rule (empty list: the rule holds)"""
    bad = []
    for b, f, i, x, y, cx, cy in sampled_coordinates(targets, H, W, grid_sample, s):
        for v, clamped, size in ((x, cx, W), (y, cy, H)):
            if grid_sample:
                if abs(v - round(v)) < MARGIN and not (clamped and v in (0.0, size - 1.0)):
                    bad.append((b, f, i, v))
            else:
                h = v - 0.5
                if abs(h - round(h)) < MARGIN and h != round(h) and not clamped:
                    bad.append((b, f, i, v))
    return bad


def has_property(tag, targets, H, W):
    """what the case is there to show (a draw without it is redrawn)"""
    t = targets.float()
    ids, n = _counts(t)
    if tag in ("plain", "unidir"):
        ok = all(7 <= k <= 9 for nb in n for k in nb)
        for b, (n0, n1) in enumerate(n):
            shared = len(set(ids[b, 0, :n0].tolist()) & set(ids[b, 1, :n1].tolist()))
            ok = ok and 0 < shared < min(n0, n1)
        return ok
    if tag == "nearest":
        q = [(x, y) for _, _, _, x, y, _, _ in sampled_coordinates(targets, H, W, False)]
        halves = [v for xy in q for v in xy if v - 0.5 == round(v - 0.5)]
        return any(int(v - 0.5) % 2 == 0 for v in halves) and any(int(v - 0.5) % 2 == 1 for v in halves)
    if tag == "edge":
        pos = sampled_coordinates(targets, H, W, True)
        xs, ys = [p[3] for p in pos], [p[4] for p in pos]
        cells = [(p[0], p[1], int(p[3]), int(p[4])) for p in pos]
        return n[0] == [6, 5] and 0.0 in xs and W - 1.0 in xs and 0.0 in ys and H - 1.0 in ys and len(set(cells)) < len(cells)
    if tag == "crowd":
        pos = sampled_coordinates(targets, H, W, True)
        cells = [(p[1], int(p[3]), int(p[4])) for p in pos]
        return n[0] == [100, 97] and len(cells) - len(set(cells)) >= 20
    if tag == "nomatch":
        return [len(set(ids[b, 0, :n[b][0]].tolist()) & set(ids[b, 1, :n[b][1]].tolist())) > 0 for b in range(3)] == [True, False, True]
    raise KeyError(tag)
