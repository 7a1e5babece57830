"""The label-propagation parts of the SOT / VOS training losses (unicorn/models/unicorn.py:315-390 with get_label_map :521-533 and
dice_coefficient :509-519) restated in torch, plus the cases, the draws and the fixture rules of tests/golden/prop_loss_*.npz (written by
tests/golden/make_golden_prop_loss.py from the reference's own compute_loss_sot / compute_loss_vos).

The restatement works on any device and in the dtype of the embeddings.  It forms the HW x HW matrix like the reference, but not the
full-resolution label map: a stride-8 label is 0.25 x (how many of the rows 8y+3, 8y+4 lie in the box) x (the same for the columns).

What a test differentiates is the scalar the reference's training step would see with a head whose loss is linear in the priors:
    SOT   total = sum_l <w_l, p_l> + corr_loss
    VOS   total = (sum_l <w_l, p_l> + sum corr_loss) / max(sum num_matched, 1)            (average_dict over the matched instances)
with fixed random w8, w16, w32 of the priors' shapes.

Fixture rules: no box corner within MARGIN of a half-integer (rint must not depend on the precision of the corner); fp32 masks hold
multiples of 1/256, so the mean of four of them is exact in fp32 and fp64 and the labels are the same bits in both; every
<name>_fp32_ref_err lies inside (REF_ERR_MIN, REF_ERR_MAX).  The embeddings of a case are non-zero in `nz` of the 128 channels (drawn at
random positions; exact zeros elsewhere): the gradient in a zero channel is an exact zero, so the fp64 gradients, which do not compress,
keep every file below the size of the largest mot_corr / corr_backward fixture.  `vos_k9` has all 128 channels."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-3
REF_ERR_MIN, REF_ERR_MAX = 2.0 ** -25, 1e-5      # as tests/mot_corr_ref.py: below, an accident of rounding; above, not rounding
C = 128
EPS = 1e-5

# tag -> kind, B, H8, W8, M, nz (non-zero channels), max_inst, mask rate, mask dtype
CASES = {
    "sot_flat": ("sot", 1, 12, 20, 2, 64, None, 0, None),
    "sot_ragged": ("sot", 3, 13, 18, 2, 24, None, 0, None),
    "sot_edge": ("sot", 4, 9, 14, 2, 32, None, 0, None),
    "vos_box": ("vos", 2, 8, 12, 6, 64, None, 0, None),
    "vos_cap": ("vos", 2, 7, 10, 6, 64, 2, 0, None),
    "vos_k9": ("vos", 1, 8, 8, 12, 128, None, 0, None),
    "vos_mask_r2": ("vos", 2, 8, 12, 4, 64, None, 2, "uint8"),
    "vos_mask_r4": ("vos", 2, 6, 9, 4, 64, None, 4, "float32"),
    "vos_mask_r1": ("vos", 2, 8, 8, 4, 64, None, 1, "float32"),
}
FLOAT_RESULTS = ("corr_loss", "p8", "p16", "p32", "g_embed_0", "g_embed_1")
EXACT_RESULTS = ("gt0", "gt1", "matched", "num_matched")
INPUTS = ("embed_0", "embed_1", "targets", "w8", "w16", "w32")
FIXTURE_SIZE_LIMIT = 478359                       # tests/golden/corr_backward_batch.npz, the largest of the mot_corr_* / corr_backward_* files


def case_kc(tag):
    _, _, _, _, M, _, max_inst, _, _ = CASES[tag]
    return 1 if CASES[tag][0] == "sot" else (M if max_inst is None else min(M, max_inst))


def load_case(tag):
    return dict(np.load(os.path.join(GOLDEN, "prop_loss_%s.npz" % tag)))


# ---------------------------------------------------------------------------------------------------------------- labels
def box_spans(rows, H, W):
    """rows (n, 4) cx, cy, w, h -> list of (x1, x2, y1, y2): the pixels labels[y1:y2, x1:x2] selects, after get_label_map's max(0, start) and
    Python's slice rules for the end (negative: size + end; above the size: clipped); corners in fp32, rounded half to even"""
    r = rows.detach().float().cpu()
    cx, cy, w, h = r.unbind(-1)
    c = torch.round(torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)).int().tolist()
    out = []
    for x1, y1, x2, y2 in c:
        xs, ys = slice(max(0, x1), x2).indices(W), slice(max(0, y1), y2).indices(H)
        out.append((xs[0], max(xs[1], xs[0]), ys[0], max(ys[1], ys[0])))
    return out


def _hits(lo, hi, n8):
    """(n8,) how many of 8p+3, 8p+4 lie in [lo, hi)"""
    p = torch.arange(n8) * 8 + 3
    return ((p >= lo) & (p < hi)).long() + ((p + 1 >= lo) & (p + 1 < hi)).long()


def labels_from_boxes(rows, H, W, dtype, device):
    """rows (n, 4) -> (n, H/8 * W/8) = F.interpolate(get_label_map(rows), 1/8, bilinear).flatten(-2), without the full-resolution map"""
    out = []
    for x1, x2, y1, y2 in box_spans(rows, H, W):
        out.append((0.25 * (_hits(y1, y2, H // 8)[:, None] * _hits(x1, x2, W // 8)[None, :]).to(dtype)).reshape(-1))
    return torch.stack(out).to(device)


def labels_from_masks(m, r, dtype):
    """m (n, r H8, r W8) -> (n, H8 W8): the bilinear 1/r of the reference's init_with_mask lines"""
    m = m.to(dtype)
    if r == 1:
        return m.flatten(-2)
    o = 1 if r == 4 else 0
    a, b, c, d = m[:, o::r, o::r], m[:, o::r, o + 1::r], m[:, o + 1::r, o::r], m[:, o + 1::r, o + 1::r]
    return (0.5 * (0.5 * a + 0.5 * b) + 0.5 * (0.5 * c + 0.5 * d)).flatten(-2)


def match_table(targets, Kc):
    """the double loop of compute_loss_vos (:352-361) -> matched (B, Kc, 2) int32 (-1 in unused slots), num_matched (B,) int32"""
    ids = targets.detach().float()[..., 5].cpu()
    B = ids.shape[0]
    matched, num = torch.full((B, Kc, 2), -1, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)
    for b in range(B):
        id_r, id_c = ids[b, 0].tolist(), ids[b, 1].tolist()
        n = 0
        for i, r in enumerate(id_r):
            if n == Kc:
                break
            if r != 0:
                for j, c in enumerate(id_c):
                    if c != 0 and c == r:
                        matched[b, n, 0], matched[b, n, 1] = i, j
                        n += 1
                        break
        num[b] = n
    return matched, num


# ---------------------------------------------------------------------------------------------------------------- the restatement
def propagate(embed_0, embed_1, gt0):
    simi = torch.bmm(embed_0.flatten(-2).transpose(-1, -2), embed_1.flatten(-2))
    return torch.bmm(gt0, torch.softmax(simi, dim=1))


def pyramid(p8):
    H8, W8 = p8.shape[-2:]
    a = p8[..., :H8 // 2 * 2, :W8 // 2 * 2]
    p16 = 0.25 * ((a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2]))
    c = p8[..., :H8 // 4 * 4, :W8 // 4 * 4]
    p32 = 0.25 * ((c[..., 1::4, 1::4] + c[..., 1::4, 2::4]) + (c[..., 2::4, 1::4] + c[..., 2::4, 2::4]))
    return p16, p32


def dice(x, t):
    inter = (x * t).sum()
    union = (x ** 2.0).sum() + (t ** 2.0).sum() + EPS
    return 1. - (2 * inter / union)


def sot_loss(embed_0, embed_1, targets, img_size):
    B, _, H8, W8 = embed_0.shape
    H, W = img_size
    t = targets.detach().float()
    gt0 = labels_from_boxes(t[:, 0, 0, 1:5], H, W, embed_0.dtype, embed_0.device)[:, None]
    gt1 = labels_from_boxes(t[:, 1, 0, 1:5], H, W, embed_0.dtype, embed_0.device)[:, None]
    p8 = propagate(embed_0, embed_1, gt0).view(B, 1, H8, W8)
    p16, p32 = pyramid(p8)
    matched = torch.zeros((B, 1, 2), dtype=torch.int32)
    return {"corr_loss": dice(p8.flatten(-2), gt1), "p8": p8, "p16": p16, "p32": p32, "gt0": gt0, "gt1": gt1, "matched": matched,
            "num_matched": torch.ones(B, dtype=torch.int32)}


def vos_loss(embed_0, embed_1, targets, img_size, masks=None, max_inst=None):
    B, _, H8, W8 = embed_0.shape
    H, W = img_size
    t = targets.detach().float()
    M = t.shape[2]
    Kc = M if max_inst is None else min(M, max_inst)
    dt, dev = embed_0.dtype, embed_0.device
    matched, num = match_table(t, Kc)
    gt0, gt1 = torch.zeros((B, Kc, H8 * W8), dtype=dt, device=dev), torch.zeros((B, Kc, H8 * W8), dtype=dt, device=dev)
    for b in range(B):
        n = int(num[b])
        if n == 0:
            continue
        i, j = matched[b, :n, 0].long(), matched[b, :n, 1].long()
        if masks is None:
            gt0[b, :n], gt1[b, :n] = labels_from_boxes(t[b, 0, i, 1:5], H, W, dt, dev), labels_from_boxes(t[b, 1, j, 1:5], H, W, dt, dev)
        else:
            r = masks.shape[3] // H8
            gt0[b, :n], gt1[b, :n] = labels_from_masks(masks[b, 0, i.to(dev)], r, dt), labels_from_masks(masks[b, 1, j.to(dev)], r, dt)
    p8 = propagate(embed_0, embed_1, gt0).view(B, Kc, H8, W8)
    p16, p32 = pyramid(p8)
    live = (torch.arange(Kc)[None, :] < num[:, None]).to(dev)
    x, g = p8.flatten(-2), gt1
    loss = 1. - 2 * (x * g).sum(-1) / ((x ** 2.0).sum(-1) + (g ** 2.0).sum(-1) + EPS)
    return {"corr_loss": torch.where(live, loss, torch.zeros_like(loss)), "p8": p8, "p16": p16, "p32": p32, "gt0": gt0, "gt1": gt1,
            "matched": matched, "num_matched": num}


def total_of(kind, res, w8, w16, w32):
    """the scalar a training step with a prior-linear head would differentiate (see the module text); res: corr_loss, p8, p16, p32, num_matched"""
    dt = res["p8"].dtype
    lin = sum((w.to(dt) * p).sum() for w, p in zip((w8, w16, w32), (res["p8"], res["p16"], res["p32"])))
    if kind == "sot":
        return lin + res["corr_loss"]
    n = res["num_matched"].sum().clamp(min=1).to(device=res["p8"].device, dtype=dt)
    return (lin + res["corr_loss"].sum()) / n


def loss_and_grads(kind, embed_0, embed_1, targets, img_size, w8, w16, w32, masks=None, max_inst=None, fn=None):
    """-> the result dict of the restatement (or of fn, an operator wrapper with the same result keys) plus g_embed_0, g_embed_1 of total_of"""
    e0, e1 = embed_0.detach().clone().requires_grad_(True), embed_1.detach().clone().requires_grad_(True)
    if fn is not None:
        res = fn(e0, e1)
    elif kind == "sot":
        res = sot_loss(e0, e1, targets, img_size)
    else:
        res = vos_loss(e0, e1, targets, img_size, masks, max_inst)
    total_of(kind, res, w8, w16, w32).backward()
    out = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in res.items()}
    out["g_embed_0"], out["g_embed_1"] = e0.grad, e1.grad
    return out


# ---------------------------------------------------------------------------------------------------------------- draws and the rules
def _box_rows(g, n, H, W):
    """n rows cx, cy, w, h on a 1/4 px raster shifted by 1/8 px with w, h multiples of 1/2: every corner is 1/8 px off the nearest half-integer"""
    cx = torch.randint(4 * 8, 4 * (W - 8), (n,), generator=g).float() / 4 + 0.125
    cy = torch.randint(4 * 8, 4 * (H - 8), (n,), generator=g).float() / 4 + 0.125
    w = torch.randint(2 * 12, 2 * (W // 2), (n,), generator=g).float() / 2
    h = torch.randint(2 * 12, 2 * (H // 2), (n,), generator=g).float() / 2
    return torch.stack([cx, cy, w, h], dim=-1)


EDGE_BOXES = {      # sot_edge, 72 x 112 images: (sample, frame) -> cx, cy, w, h of row 0
    (0, 0): (10.125, 8.125, 40.5, 30.5),          # crosses the left and the top border
    (0, 1): (100.125, 60.125, 40.5, 40.5),        # crosses the right and the bottom border: both rounded ends above the size
    (1, 0): (-30.125, 30.125, 20.5, 20.5),        # left of the image: x2 = -20, a NEGATIVE end, which the slice reads as 112 - 20
    (1, 1): (50.125, -20.125, 30.5, 10.5),        # above the image: y2 = -15 -> 72 - 15
    (2, 0): (40.125, 30.125, 0.5, 20.5),          # x1 = x2 = 40: empty
    (2, 1): (50.125, 30.125, -10.5, 20.5),        # negative width: x2 < x1, empty
    (3, 0): (60.125, 40.125, 30.5, 20.5),         # an ordinary box
    (3, 1): (56.125, 36.125, 150.5, 100.5),       # covers the whole image, beyond every border
}


def draw(tag, seed):
    """-> dict of fp32 / uint8 inputs: embed_0, embed_1 (B, 128, H8, W8), targets (B, 2, M, 6), w8, w16, w32, and masks for the mask cases"""
    kind, B, H8, W8, M, nz, max_inst, r, mdt = CASES[tag]
    Kc, H, W = case_kc(tag), 8 * H8, 8 * W8
    g = torch.Generator().manual_seed(seed)
    out = {}
    for n in ("embed_0", "embed_1"):
        e = torch.zeros(B, C, H8, W8)
        ch = torch.randperm(C, generator=g)[:nz]
        e[:, ch] = 0.5 * torch.randn(B, nz, H8, W8, generator=g)
        out[n] = e
    t = torch.zeros(B, 2, M, 6)
    t[..., 1:5] = _box_rows(g, B * 2 * M, H, W).view(B, 2, M, 4)
    t[..., 0] = torch.randint(0, 3, (B, 2, M), generator=g).float()
    if tag == "sot_edge":
        for (b, f), row in EDGE_BOXES.items():
            t[b, f, 0, 1:5] = torch.tensor(row)
    if kind == "sot":
        t[..., 5] = torch.randint(0, 4, (B, 2, M), generator=g).float()           # ids play no part in the SOT branch
    elif tag == "vos_box":
        t[0, 0, :, 5], t[0, 1, :, 5] = torch.tensor([3., 0, 5, 7, 5, 9]), torch.tensor([5., 7, 5, 0, 3, 8])
        t[1, 0, :, 5], t[1, 1, :, 5] = torch.tensor([1., 2, 0, 0, 0, 0]), torch.tensor([3., 4, 0, 0, 0, 0])
    elif tag == "vos_cap":
        t[0, 0, :, 5], t[0, 1, :, 5] = torch.tensor([4., 2, 0, 6, 8, 1]), torch.tensor([8., 6, 4, 2, 0, 0])
        t[1, 0, :, 5], t[1, 1, :, 5] = torch.tensor([0., 5, 3, 0, 0, 0]), torch.tensor([7., 0, 3, 0, 0, 0])
    elif tag == "vos_k9":
        t[0, 0, :, 5] = torch.tensor([2., 11, 0, 7, 5, 20, 9, 1, 4, 0, 3, 6])
        t[0, 1, :, 5] = torch.tensor([9., 1, 2, 3, 0, 4, 5, 6, 30, 7, 11, 0])
    else:                                                                          # the mask cases: three and two matches
        t[0, 0, :, 5], t[0, 1, :, 5] = torch.tensor([6., 2, 9, 4]), torch.tensor([4., 6, 0, 2])
        t[1, 0, :, 5], t[1, 1, :, 5] = torch.tensor([0., 7, 1, 3]), torch.tensor([3., 5, 7, 0])
    out["targets"] = t
    for n, s in (("w8", 1), ("w16", 2), ("w32", 4)):
        out[n] = torch.randn(B, Kc, H8 // s, W8 // s, generator=g)
    if r:
        Hm, Wm = r * H8, r * W8
        m = torch.zeros(B, 2, M, Hm, Wm)
        for b in range(B):
            for f in range(2):
                for i in range(M):                                                 # a random rectangle with a soft or a hard inside
                    y0, x0 = int(torch.randint(0, Hm // 2, (1,), generator=g)), int(torch.randint(0, Wm // 2, (1,), generator=g))
                    y1, x1 = y0 + 2 + int(torch.randint(0, Hm // 2, (1,), generator=g)), x0 + 2 + int(torch.randint(0, Wm // 2, (1,), generator=g))
                    if mdt == "uint8":
                        m[b, f, i, y0:y1, x0:x1] = (torch.rand(y1 - y0, x1 - x0, generator=g) < 0.85).float()
                    else:
                        m[b, f, i, y0:y1, x0:x1] = torch.randint(0, 257, (y1 - y0, x1 - x0), generator=g).float() / 256
        out["masks"] = m.to(torch.uint8) if mdt == "uint8" else m
    return out


def rule_violations(targets):
    """box corners within MARGIN of a half-integer (empty list: the rule holds)"""
    t = targets.float().double()
    cx, cy, w, h = t[..., 1], t[..., 2], t[..., 3], t[..., 4]
    bad = []
    for name, v in (("x1", cx - 0.5 * w), ("y1", cy - 0.5 * h), ("x2", cx + 0.5 * w), ("y2", cy + 0.5 * h)):
        d = ((v - 0.5) - torch.round(v - 0.5)).abs()
        for idx in (d < MARGIN).nonzero().tolist():
            bad.append((name, tuple(idx), float(v[tuple(idx)])))
    return bad


def has_property(tag, ins):
    """what the case is there to show"""
    kind, B, H8, W8, M, nz, max_inst, r, mdt = CASES[tag]
    t = ins["targets"]
    H, W = 8 * H8, 8 * W8
    if r:
        m = ins["masks"]
        if str(m.dtype) != "torch." + mdt:
            return False
        if mdt == "float32" and not torch.equal(m * 256, torch.round(m * 256)):
            return False
    if tag == "sot_edge":
        sp = {k: box_spans(t[k[0], k[1], 0:1, 1:5], H, W)[0] for k in EDGE_BOXES}
        raw = {k: torch.round(torch.tensor([v[0] - 0.5 * v[2], v[1] - 0.5 * v[3], v[0] + 0.5 * v[2], v[1] + 0.5 * v[3]])).int().tolist()
               for k, v in EDGE_BOXES.items()}
        return (raw[(0, 0)][0] < 0 and raw[(0, 0)][1] < 0 and raw[(0, 1)][2] > W and raw[(0, 1)][3] > H
                and raw[(1, 0)][2] < 0 and sp[(1, 0)][:2] == (0, W + raw[(1, 0)][2]) and raw[(1, 1)][3] < 0 and sp[(1, 1)][2:] == (0, H + raw[(1, 1)][3])
                and sp[(2, 0)][0] == sp[(2, 0)][1] and raw[(2, 1)][2] < raw[(2, 1)][0] and sp[(2, 1)][0] == sp[(2, 1)][1]
                and sp[(3, 1)] == (0, W, 0, H))
    if kind == "sot":
        return True
    matched, num = match_table(t, case_kc(tag))
    if tag == "vos_box":
        return num.tolist() == [4, 0] and matched[0, :4].tolist() == [[0, 4], [2, 0], [3, 1], [4, 0]]
    if tag == "vos_cap":
        full = match_table(t, M)[1].tolist()
        return full == [4, 1] and num.tolist() == [2, 1] and matched[0].tolist() == [[0, 2], [1, 3]] and matched[1].tolist() == [[2, 2], [-1, -1]]
    if tag == "vos_k9":
        return num.tolist() == [9]
    return num.tolist() == [3, 2]
