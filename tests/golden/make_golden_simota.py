"""Golden vectors for the SimOTA label assignment (uni_simota_assign, ops.simota_assign / simota_assign_batch), produced by EXECUTING the
reference's own UnicornHeadMask.get_assignments (unicorn/models/unicorn_head_mask.py:754-983, with get_in_boxes_info, dynamic_k_matching
and bboxes_iou) on the CPU in fp32.  The head is made with __new__: the three methods read only mode, num_classes and num_classes_sot.
`cost` and `pair_wise_ious` are recorded by wrapping dynamic_k_matching.  No reference text is stored.

No fixture holds a decision that fp32 rounding could tip (tests/simota_ref.py decision_margins): with E = max |cost_fp32 - cost_fp64| over
costs < 5e4 (fp64 = the restatement in double), every cost decision -- the k-th against the (k+1)-th cheapest anchor of every box, the
cheapest against the second cheapest box in every contested column -- has a gap > 8 max(E, fp32 spacing at the larger cost); every top-10
IoU sum is farther than 8 x 10 x max |iou_fp32 - iou_fp64| from the integer that would change k; every geometry delta has |delta| > 1e-3 px
or is exactly zero (a true zero is zero in every precision; the clip path produces them by construction, see decision_margins).
A draw that fails, or that lacks the property its case is there for, is redrawn with the next seed, never filtered.

    python tests/golden/make_golden_simota.py        -> tests/golden/simota_<case>.npz
"""
import os
import sys

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import simota_ref as R  # noqa: E402

KIND = {"small": "small", "crowd": "crowd", "edge": "edge", "tiny": "tiny"}


def reference_assign(mode, C, bbox, obj, cls, gt_bboxes, gt_classes, xs, ys, st, img_size):
    """the reference's get_assignments on the CPU -> its five outputs (its order) + the cost and IoU matrices it handed to dynamic_k_matching"""
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.unicorn_head_mask import UnicornHeadMask
    head = UnicornHeadMask.__new__(UnicornHeadMask)
    nn.Module.__init__(head)
    head.mode, head.num_classes, head.num_classes_sot = mode, C, C
    seen = {}
    inner = head.dynamic_k_matching

    def recording(cost, pair_wise_ious, *rest):
        seen["cost"], seen["iou"] = cost.clone(), pair_wise_ious.clone()
        return inner(cost, pair_wise_ious, *rest)
    head.dynamic_k_matching = recording
    A, G = bbox.shape[0], gt_bboxes.shape[0]
    imgs = torch.zeros(1, 3, img_size[0], img_size[1])
    out = head.get_assignments(0, G, A, gt_bboxes, gt_classes, bbox, st[None], xs[None], ys[None], cls[None], bbox[None], obj[None], None, imgs)
    res = dict(zip(R.OUTPUTS, out))
    res.update(seen)
    return res


def properties(tag, r):
    """the property a case is there for, from the restatement's result"""
    contested = int(r["contested"].sum())
    cheapest_did_not_select = int((r["matching"] & ~r["selected"]).any(0).sum())
    penalised = int((r["selected"] & (r["cost"] >= 5e4)).any(1).sum())
    ok = {"cls4": contested >= 1, "small": penalised >= 1, "crowd": contested >= 30 and cheapest_did_not_select >= 1,
          "tiny": int(r["cand"].sum()) < 10}.get(tag, True)
    return ok, {"contested": contested, "won_without_selecting": cheapest_did_not_select, "boxes_selecting_penalised": penalised,
                "candidates": int(r["cand"].sum())}


def one_image(tag, H, W, G, C, mode, seed):
    xs, ys, st = R.anchors(H, W)
    first = seed
    while True:
        assert seed < first + 60, "no draw of %s passes: the case's recipe is wrong, not the seeds" % tag
        ins = R.draw(H, W, G, C, seed, KIND.get(tag, "plain"))
        m, r32, r64 = R.margins_of(*ins, xs, ys, st, (H, W), C)
        ok, props = properties(tag, r64)
        if m["ok"] and ok:
            break
        print("%-6s seed %d: margins %s, properties %s -- redrawing" % (tag, seed, {k: ("%.3g" % v if isinstance(v, float) else v) for k, v in m.items()}, props))
        seed += 1
    ref = reference_assign(mode, C, *ins, xs, ys, st, (H, W))
    res = {n: t.numpy() for n, t in zip(R.INPUTS, ins)}
    for n in R.OUTPUTS:
        res[n] = np.asarray(ref[n].numpy() if isinstance(ref[n], torch.Tensor) else ref[n])
    res["cost"], res["iou"] = ref["cost"].numpy(), ref["iou"].numpy()
    for n in ("cost_dev", "iou_dev", "min_gap_ratio", "ksum_margin", "min_abs_delta"):
        res["margin_" + n] = np.float64(m[n])
    res["seed"] = np.int64(seed)
    for n, v in props.items():
        res["prop_" + n] = np.int64(v)
    print("%-6s seed %d  A %d G %d C %d  num_fg %d  k %s  E %.3g (%.0f spacings at cost 8)  iou_dev %.3g  gap/unit %.3g  ksum margin %.3g  "
          "min |delta| %.3g  %s" % (tag, seed, xs.shape[0], G, C, int(res["num_fg"]), r64["k"].tolist()[:12], m["cost_dev"],
                                    m["cost_dev"] / float(np.spacing(np.float32(8))), m["iou_dev"], m["min_gap_ratio"], m["ksum_margin"],
                                    m["min_abs_delta"], props))
    return res


def main():
    for k, (tag, (H, W, Gs, C, mode)) in enumerate(R.CASES.items()):
        if len(Gs) == 1:
            res = one_image(tag, H, W, Gs[0], C, mode, 100 * k)
        else:                                                       # padded labels (B, M, 5) and outputs (B, A, 5 + C); results per image
            res, seed, outs, labels = {}, 100 * k, [], torch.zeros(len(Gs), R.BATCH_M, 5)
            for b, G in enumerate(Gs):
                if G:
                    img = one_image(tag, H, W, G, C, mode, seed)
                    seed = int(img["seed"]) + 1
                    labels[b, :G] = torch.cat([torch.from_numpy(img["gt_classes"])[:, None], torch.from_numpy(img["gt_bboxes"])], 1)
                    assert bool((labels[b, :G].sum(1) > 0).all()), "a box row that the reference's nlabel would not count"
                    res.update({"%s_%d" % (n, b): v for n, v in img.items()})
                else:
                    img = {n: t.numpy() for n, t in zip(R.INPUTS, R.draw(H, W, 0, C, seed))}
                    seed += 1
                outs.append(np.concatenate([img["bbox"], img["obj"], img["cls"]], 1))
            res["outputs"], res["labels"] = np.stack(outs), labels.numpy()
        res["shape"] = np.array([H, W, C] + list(Gs), dtype=np.int64)
        path = os.path.join(HERE, "simota_%s.npz" % tag)
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
