"""Golden vectors for the differentiable label propagation (uni_corr_softmax_pv_lse / _bwd), produced by EXECUTING the reference's own
source lines under autograd: unicorn/models/unicorn.py:321-322 (simi_mat, trans_mat_01) are read from /root/reference, dedented and
exec'd; the product of :326, `torch.bmm(gt_lbs_0, trans_mat_01)`, is applied without that line's `.view(bs, 1, H_d, W_d)` (which fixes
K = 1).  Everything in fp64; lse = torch.logsumexp(simi_mat, dim=1).  Per tensor, fp32_ref_err = max|fp32 - fp64| / max|fp64| of the
same lines run in fp32 on the CPU: the yardstick of the fp32 GPU test (no figure comes from the kernel).  No reference text is stored.

One file per case (fp64 gradients of random data do not compress; together the cases exceed the 1 MiB limit of a committed file):

    python tests/golden/make_golden_corr_backward.py        -> tests/golden/corr_backward_<case>.npz
"""
import os
import textwrap

import numpy as np
import torch

REF = "/root/reference/unicorn/models/unicorn.py"
HERE = os.path.dirname(os.path.abspath(__file__))

# tag -> (B, R, Q, K, embedding scale, seed)
CASES = {
    "flat": (1, 160, 130, 1, 0.3, 0),        # flat softmax
    "ragged": (1, 97, 203, 3, 0.3, 1),       # not multiples of 32
    "peaky": (1, 130, 110, 9, 1.0, 2),       # median column maximum about 0.85
    "batch": (2, 64, 96, 2, 0.5, 3),
}
D = 128


def reference_lines():
    src = open(REF).read().split("\n")
    lines = src[320:322]                                      # 1-based 321..322
    assert "simi_mat = torch.bmm(embed_0.flatten(-2).transpose(-1, -2), embed_1.flatten(-2))" in lines[0], lines[0]
    assert "trans_mat_01 = torch.softmax(simi_mat, dim=1)" in lines[1], lines[1]
    assert "pred_lbs1 = torch.bmm(gt_lbs_0, trans_mat_01).view(bs, 1, H_d, W_d)" in src[325], src[325]
    return textwrap.dedent("\n".join(lines))


def evaluate(code, embed_0, embed_1, gt_lbs_0, grad_out):
    """the three lines under autograd in the dtype of the inputs -> out, lse, gradients"""
    e0 = embed_0.clone().requires_grad_(True)
    e1 = embed_1.clone().requires_grad_(True)
    lb = gt_lbs_0.clone().requires_grad_(True)
    ns = {"torch": torch, "embed_0": e0.unsqueeze(2), "embed_1": e1.unsqueeze(2)}      # (B, C, 1, HW): the reference's maps are (B, C, H/8, W/8)
    exec(code, ns)
    out = torch.bmm(lb, ns["trans_mat_01"])                                               # :326 without the .view
    lse = torch.logsumexp(ns["simi_mat"], dim=1)
    out.backward(grad_out)
    return {"out": out.detach(), "lse": lse.detach(), "g_embed_0": e0.grad, "g_embed_1": e1.grad, "g_labels": lb.grad}


def main():
    code = reference_lines()
    for tag, (B, R, Q, K, scale, seed) in CASES.items():
        g = torch.Generator().manual_seed(seed)
        embed_0 = (scale * torch.randn(B, D, R, generator=g)).float()
        embed_1 = (scale * torch.randn(B, D, Q, generator=g)).float()
        labels = torch.rand(B, K, R, generator=g).float()
        grad_out = torch.randn(B, K, Q, generator=g).float()
        res = {"shape": np.array([B, R, Q, K], dtype=np.int64), "scale": np.float64(scale)}
        ref = evaluate(code, embed_0.double(), embed_1.double(), labels.double(), grad_out.double())
        f32 = evaluate(code, embed_0, embed_1, labels, grad_out)
        for n, t in (("embed_0", embed_0), ("embed_1", embed_1), ("labels", labels), ("grad_out", grad_out)):
            res[n] = t.numpy()
        for n, t in ref.items():
            res[n] = t.numpy()
            err = float((f32[n].double() - t).abs().max() / t.abs().max())
            res[n + "_fp32_ref_err"] = np.float64(err)
            print("%-7s %-10s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(t.abs().max()), err))
        P = torch.softmax(torch.bmm(embed_0.double().transpose(1, 2), embed_1.double()), dim=1)
        print("%-7s median column maximum %.3f" % (tag, float(P.max(dim=1).values.median())))
        path = os.path.join(HERE, "corr_backward_%s.npz" % tag)
        np.savez_compressed(path, **res)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
