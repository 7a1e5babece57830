"""Pure-torch restatement of the SimOTA label assignment (unicorn/models/unicorn_head_mask.py:754-983 get_assignments / get_in_boxes_info /
dynamic_k_matching with bboxes_iou of unicorn/utils/boxes.py:154-177), in the dtype and on the device of its inputs, with the tie rule of
uni_simota_assign made explicit (lower anchor index in both top-k passes, lower box index in the arg-min).  tests/test_simota_cpu.py pins
it to the fixtures the reference's own functions produced; the GPU tests and tools/simota_bench.py use it where no fixture exists.  A plain
module imported like tests/planted.py; it holds no fixture and changes no pytest setting."""
import os

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STRIDES = (8, 16, 32)
# tag -> (H, W, boxes per image, num_classes, reference mode); "batch" holds three images with 4 / 0 / 9 boxes in labels padded to M = 12
CASES = {"sot": (64, 96, (1,), 1, "sot"), "cls4": (64, 96, (5,), 4, "mot"), "small": (96, 160, (12,), 1, "mot"),
         "crowd": (96, 160, (70,), 1, "mot"), "edge": (72, 104, (6,), 8, "mot"), "tiny": (32, 32, (1,), 1, "sot"),
         "batch": (64, 96, (4, 0, 9), 2, "mot")}
BATCH_M = 12
INPUTS = ("bbox", "obj", "cls", "gt_bboxes", "gt_classes")
OUTPUTS = ("gt_matched_classes", "fg_mask", "pred_ious_this_matching", "matched_gt_inds", "num_fg")      # the reference's order
PENALTY = 100000.0
MARGIN = 8.0            # a decision gap must exceed MARGIN x max(fp32-vs-fp64 cost deviation, fp32 spacing at the larger cost)
MIN_DELTA = 1e-3        # px: no anchor centre closer than this to a box or centre-square edge


def anchors(H, W, device="cpu", dtype=torch.float32):
    """x_shifts, y_shifts, expanded_strides (A,) of the levels of strides 8 / 16 / 32 over an H x W image (grids of H // s x W // s cells)"""
    xs, ys, st = [], [], []
    for s in STRIDES:
        h, w = H // s, W // s
        yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        xs.append(xx.reshape(-1))
        ys.append(yy.reshape(-1))
        st.append(torch.full((h * w,), s))
    return tuple(torch.cat(t).to(device=device, dtype=dtype) for t in (xs, ys, st))


def load_case(tag):
    return dict(np.load(os.path.join(GOLD, "simota_%s.npz" % tag)))


def geometry(gt_bboxes, xs, ys, st, img_size, deltas=False):
    """-> in_box (G, A), in_ctr (G, A); deltas=True adds the (G, A, 8) tensor of the eight strict comparisons' left sides (a diagnostic of
    the fixture rule that the eager lines never build: only min_abs_delta asks for it)"""
    xc = (xs * st + 0.5 * st)[None]
    yc = (ys * st + 0.5 * st)[None]
    cx, cy, w, h = (gt_bboxes[:, i, None] for i in range(4))
    box = torch.stack([xc - (cx - 0.5 * w), yc - (cy - 0.5 * h), (cx + 0.5 * w) - xc, (cy + 0.5 * h) - yc], 2)
    qx, qy = torch.clamp(cx, min=0, max=img_size[1]), torch.clamp(cy, min=0, max=img_size[0])
    rad = 2.5 * st[None]
    ctr = torch.stack([xc - (qx - rad), yc - (qy - rad), (qx + rad) - xc, (qy + rad) - yc], 2)
    flags = (box.min(dim=-1).values > 0.0, ctr.min(dim=-1).values > 0.0)
    return flags + (torch.cat([box, ctr], 2),) if deltas else flags


def min_abs_delta(gt_bboxes, xs, ys, st, img_size):
    """The smallest NON-ZERO |delta| of the eight strict geometry comparisons over all (box, anchor) pairs, px (inf where there is none); an
    exact zero is no rounding hazard, see decision_margins.  Reads the result back: for fixtures and margins only, not part of assign()."""
    d = geometry(gt_bboxes, xs, ys, st, img_size, deltas=True)[2].abs()
    d = d[d > 0]
    return float(d.min()) if d.numel() else float("inf")


def pair_iou(gt, pred):
    """IoU of every ground-truth box with every prediction: (G, 4), (N, 4) boxes as cx, cy, w, h -> (G, N).  Each box becomes its four edges
    (centre -+ size / 2); the overlap of a pair is width x height of the common rectangle where both are strictly positive and zero elsewhere
    (the product is formed first and then gated, so a degenerate pair gives the same bits as the reference's function); IoU = overlap /
    (area of g + area of p - overlap), the areas being w x h of the inputs."""
    def edges(b):
        half_w, half_h = b[:, 2] / 2, b[:, 3] / 2
        return b[:, 0] - half_w, b[:, 1] - half_h, b[:, 0] + half_w, b[:, 1] + half_h
    g_left, g_top, g_right, g_bottom = (e[:, None] for e in edges(gt))
    p_left, p_top, p_right, p_bottom = (e[None, :] for e in edges(pred))
    left, right = torch.maximum(g_left, p_left), torch.minimum(g_right, p_right)
    top, bottom = torch.maximum(g_top, p_top), torch.minimum(g_bottom, p_bottom)
    overlapping = ((left < right) & (top < bottom)).to(gt.dtype)
    overlap = (right - left) * (bottom - top) * overlapping
    gt_area, pred_area = gt[:, 2] * gt[:, 3], pred[:, 2] * pred[:, 3]
    return overlap / (gt_area[:, None] + pred_area[None, :] - overlap)


def assign(bbox, obj, cls, gt_bboxes, gt_classes, xs, ys, st, img_size, num_classes, loop=False):
    """bbox (A, 4), obj (A, 1), cls (A, C), gt_bboxes (G, 4), gt_classes (G,), xs / ys / st (A,) -> dict with the reference's five outputs
    plus cand (A,) geometry candidates, cost / iou (G, n_cand), k (G,), selected (G, n_cand) before and matching (G, n_cand) after the
    conflict resolution.  loop=True selects with the reference's per-box topk loop and its host read-backs (the timing
    yardstick of tools/simota_bench.py); the default is the same selection without a loop, with the documented tie rule."""
    G, dev = gt_bboxes.shape[0], bbox.device
    in_box, in_ctr = geometry(gt_bboxes, xs, ys, st, img_size)
    cand = in_box.any(0) | in_ctr.any(0)
    both = in_box[:, cand] & in_ctr[:, cand]
    iou = pair_iou(gt_bboxes, bbox[cand])
    n = iou.shape[1]
    onehot = F.one_hot(gt_classes.to(torch.int64), num_classes).to(bbox.dtype)[:, None, :].expand(G, n, num_classes)
    p = (cls[cand].sigmoid() * obj[cand].reshape(-1, 1).sigmoid()).sqrt()
    cls_cost = F.binary_cross_entropy(p[None].expand(G, n, num_classes), onehot, reduction="none").sum(-1)
    cost = cls_cost + 3.0 * (-torch.log(iou + 1e-8)) + PENALTY * (~both)
    top = torch.topk(iou, min(10, n), dim=1).values                # sorted, largest first
    ksum = torch.zeros(G, dtype=bbox.dtype, device=dev)
    for j in range(top.shape[1]):                                  # largest first, in the dtype
        ksum = ksum + top[:, j]
    k = torch.clamp(ksum.int(), min=1)
    if loop:
        selected = torch.zeros_like(cost)
        for g in range(G):
            _, pos = torch.topk(cost[g], k=min(int(k[g].item()), n), largest=False)
            selected[g][pos] = 1.0
        selected = selected > 0
    else:
        order = torch.sort(cost, dim=1, stable=True).indices       # equal costs: the lower anchor first
        selected = torch.zeros_like(cost, dtype=torch.bool).scatter_(1, order, torch.arange(n, device=dev)[None] < k[:, None])
    contested = selected.sum(0) > 1
    rows = torch.arange(G, device=dev)[:, None]
    cheapest = torch.where(cost == cost.min(dim=0).values[None], rows, G).min(dim=0).values      # equal costs: the lower box
    matching = torch.where(contested[None], rows == cheapest[None], selected)
    fg_in = matching.any(0)
    fg_mask = torch.zeros_like(cand)
    fg_mask[cand] = fg_in
    inds = matching[:, fg_in].to(torch.uint8).argmax(0) if n else torch.zeros((0,), dtype=torch.int64, device=dev)
    return {"gt_matched_classes": gt_classes[inds], "fg_mask": fg_mask, "pred_ious_this_matching": (matching * iou).sum(0)[fg_in],
            "matched_gt_inds": inds, "num_fg": int(fg_in.sum()), "cand": cand, "both": both, "cost": cost, "iou": iou, "ksum": ksum, "k": k,
            "selected": selected, "matching": matching, "contested": contested}


def decision_margins(r32, r64, delta):
    """The distance of every decision of the fp64 restatement `r64` from its tipping point, against the deviation of the fp32 restatement
    `r32` of the same inputs (both from assign(); `delta` = the smaller min_abs_delta() of the two precisions).  -> dict: cost_dev E = max |cost32 - cost64| over costs < 5e4, iou_dev, min_gap_ratio =
    min over cost decisions of gap / max(E, fp32 spacing at the larger cost) (k-th against (k+1)-th cheapest of every box, cheapest against
    second cheapest in every contested column), ksum_margin = smallest distance of a top-10 IoU sum from the integer that would change k,
    min_abs_delta (the smallest NON-ZERO geometry delta), and ok: every decision outside the margins the fixtures demand.
    A delta that is exactly zero in fp64 is exempt from the 1e-3 px rule: with fp32 inputs the double evaluation is exact, so the true delta
    is zero, and a chain of correctly rounded subtractions whose exact result is representable gives zero in every precision -- `> 0` is
    false everywhere.  The clip path makes such zeros by construction: a centre clipped to 0 or to the image size, +- 2.5 strides, lands on
    anchor centres (0 + 2.5 x 8 = 20 = 2 x 8 + 4)."""
    c32, c64 = r32["cost"].double().cpu(), r64["cost"].double().cpu()
    if not (torch.equal(r32["cand"].cpu(), r64["cand"].cpu()) and torch.equal(r32["both"].cpu(), r64["both"].cpu())):
        return {"cost_dev": float("inf"), "iou_dev": float("inf"), "min_gap_ratio": 0.0, "ksum_margin": 0.0, "min_abs_delta": 0.0, "ok": False}
    low = c64 < 5e4
    E = float((c32 - c64)[low].abs().max()) if bool(low.any()) else 0.0
    iou_dev = float((r32["iou"].double().cpu() - r64["iou"].double().cpu()).abs().max()) if c64.numel() else 0.0
    G, n = c64.shape
    ratio = float("inf")

    def consider(lo, hi):
        nonlocal ratio
        unit = max(E, float(np.spacing(np.float32(hi))))
        ratio = min(ratio, (hi - lo) / unit)
    srt = torch.sort(c64, dim=1).values
    k = r64["k"].cpu()
    for g in range(G):
        kg = int(k[g])
        if kg < n:
            consider(float(srt[g, kg - 1]), float(srt[g, kg]))
    col = torch.sort(c64[:, r64["contested"].cpu()], dim=0).values
    for j in range(col.shape[1]):
        consider(float(col[0, j]), float(col[1, j]))
    ks = r64["ksum"].double().cpu()
    dist = torch.where(ks < 1, 1 - ks, torch.minimum(ks - ks.floor(), ks.floor() + 1 - ks))
    ksum_margin = float(dist.min()) if G else float("inf")
    ok = ratio > MARGIN and ksum_margin > MARGIN * 10 * iou_dev and delta > MIN_DELTA
    return {"cost_dev": E, "iou_dev": iou_dev, "min_gap_ratio": ratio, "ksum_margin": ksum_margin, "min_abs_delta": delta, "ok": bool(ok)}


def margins_of(bbox, obj, cls, gt_bboxes, gt_classes, xs, ys, st, img_size, num_classes):
    """decision_margins of fp32 inputs: the restatement in fp32 and in fp64 on the device of the inputs -> (margins, r32, r64)"""
    args = (bbox, obj, cls, gt_bboxes, gt_classes, xs, ys, st)
    r32 = assign(*args, img_size, num_classes)
    r64 = assign(*[t.double() for t in args], img_size, num_classes)
    delta = min(min_abs_delta(gt_bboxes, xs, ys, st, img_size), min_abs_delta(gt_bboxes.double(), xs.double(), ys.double(), st.double(), img_size))
    return decision_margins(r32, r64, delta), r32, r64


def draw(H, W, G, C, seed, kind="plain"):
    """A synthetic image of the assignment's inputs, fp32: G ground-truth boxes (`kind` says how they are placed) and A decoded predictions of
    which about half look at one of the boxes, so that the IoU sums give k of several anchors.  -> bbox, obj, cls, gt_bboxes, gt_classes"""
    g = torch.Generator().manual_seed(seed)

    def rnd(*s):
        return torch.rand(*s, generator=g)
    xs, ys, st = anchors(H, W)
    A = xs.shape[0]
    if kind == "small":                                            # 4 - 24 px boxes
        wh = 4 + 20 * rnd(G, 2)
        c = torch.stack([W * rnd(G), H * rnd(G)], 1)
    elif kind == "crowd":                                          # clustered at the centre of the image
        wh = torch.stack([0.15 * W + 0.25 * W * rnd(G), 0.15 * H + 0.3 * H * rnd(G)], 1)
        c = torch.stack([0.5 * W + 0.12 * W * (rnd(G) - 0.5), 0.5 * H + 0.12 * H * (rnd(G) - 0.5)], 1)
    elif kind == "edge":                                           # centres outside the image on every side: the clip path
        wh = torch.stack([0.2 * W + 0.4 * W * rnd(G), 0.2 * H + 0.4 * H * rnd(G)], 1)
        c = torch.stack([W * rnd(G), H * rnd(G)], 1)
        out = torch.tensor([[-0.06 * W, 0.3 * H], [1.05 * W, 0.6 * H], [0.4 * W, -0.08 * H], [0.7 * W, 1.07 * H], [-0.03 * W, -0.05 * H]])
        c[:min(G, 5)] = (out + rnd(5, 2))[:min(G, 5)]
    elif kind == "mot":                                            # a crowded street: upright boxes of 2 - 15 % of the image width
        wh = torch.stack([0.02 * W + 0.13 * W * rnd(G), 0.06 * H + 0.4 * H * rnd(G)], 1)
        c = torch.stack([W * rnd(G), H * (0.25 + 0.6 * rnd(G))], 1)
    elif kind == "tiny":                                           # centre beyond the corner: fewer than 10 candidates
        wh = 12 + 6 * rnd(G, 2)
        c = -1 - 2 * rnd(G, 2)
    else:
        wh = torch.stack([0.1 * W + 0.4 * W * rnd(G), 0.1 * H + 0.5 * H * rnd(G)], 1)
        c = torch.stack([W * (0.1 + 0.8 * rnd(G)), H * (0.1 + 0.8 * rnd(G))], 1)
    gt_bboxes = torch.cat([c, wh], 1).float()
    gt_classes = torch.randint(0, C, (G,), generator=g).float()
    centre = torch.stack([xs * st + 0.5 * st, ys * st + 0.5 * st], 1)
    bbox = torch.cat([centre + st[:, None] * (rnd(A, 2) - 0.5), st[:, None] * 4 * torch.exp(0.5 * torch.randn(A, 2, generator=g))], 1)
    if G:
        tgt = gt_bboxes[torch.randint(0, G, (A,), generator=g)]
        looks = rnd(A) < 0.5
        aimed = torch.cat([tgt[:, :2] + 0.2 * tgt[:, 2:] * (rnd(A, 2) - 0.5), tgt[:, 2:] * torch.exp(0.25 * torch.randn(A, 2, generator=g))], 1)
        bbox = torch.where(looks[:, None], aimed, bbox)
    obj = 2 * torch.randn(A, 1, generator=g) - 1
    cls = 2 * torch.randn(A, C, generator=g) - 1
    return bbox.float(), obj.float(), cls.float(), gt_bboxes, gt_classes
