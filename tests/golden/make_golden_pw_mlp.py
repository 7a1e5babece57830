"""Golden vectors for the recomputing pwconv1-GELU-pwconv2 operator (uni_pw_mlp_act_fwd / _bwd, ops.pw_mlp), produced by EXECUTING the
reference's own ConvNeXt Block (unicorn/models/backbone/convnext.py:19-54) on the CPU: a Block of the case's width C is built, its pwconv1,
act and pwconv2 get the drawn parameters, and the three lines of its forward that the operator replaces are run on the block's own modules,

    x = blk.pwconv1(x)                                               # convnext.py:46
    x = blk.act(x)                                                   # :47
    x = blk.pwconv2(x)                                               # :48

under autograd with a drawn upstream gradient, in fp64 for the results and in fp32 for the yardstick.  The reference Block fixes Hd = 4 C and
Co = C; the case `h100` (Hd = 5 C, Co != C) re-creates the block's two Linears through their own class (type(blk.pwconv1)) at the case's
widths and keeps the block's own act.  Per result, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same lines in fp32: the bound of
the fp32 GPU test is 4 x that (or 4 x the eager deviation on the device, whichever is larger; no figure comes from the kernel).  It must be
> 0.  The hidden maps a = act(pwconv1(x)) and grad_h = the gradient at pwconv1's output are too large to store; their yardsticks
a_fp32_ref_err and grad_h_fp32_ref_err are stored for the kernel-level tests, which rebuild the maps with tests/pw_mlp_ref.py.  Inputs are
stored as fp32, results as fp64.  No reference text is stored.

    python tests/golden/make_golden_pw_mlp.py        -> tests/golden/pw_mlp_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import pw_mlp_ref as R  # noqa: E402

MAX_BYTES = 360 * 1024


def reference_block(C, Hd, Co, w1, b1, w2, b2, dtype):
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.backbone.convnext import Block
    blk = Block(dim=C, drop_path=0.0)
    assert isinstance(blk.pwconv1, torch.nn.Linear) and isinstance(blk.pwconv2, torch.nn.Linear) and isinstance(blk.act, torch.nn.GELU)
    assert getattr(blk.act, "approximate", "none") == "none"
    if (Hd, Co) != (blk.pwconv1.out_features, blk.pwconv2.out_features):
        blk.pwconv1, blk.pwconv2 = type(blk.pwconv1)(C, Hd), type(blk.pwconv2)(Hd, Co)
    blk = blk.to(dtype)
    with torch.no_grad():
        blk.pwconv1.weight.copy_(w1.to(dtype)), blk.pwconv1.bias.copy_(b1.to(dtype))
        blk.pwconv2.weight.copy_(w2.to(dtype)), blk.pwconv2.bias.copy_(b2.to(dtype))
    return blk


def evaluate(t, w1, b1, w2, b2, grad_out, dtype):
    blk = reference_block(t.shape[-1], w1.shape[0], w2.shape[0], w1, b1, w2, b2, dtype)
    x = t.detach().to(dtype).clone().requires_grad_(True)
    h = blk.pwconv1(x)
    a = blk.act(h)
    y = blk.pwconv2(a)
    h.retain_grad()
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_t": x.grad, "g_w1": blk.pwconv1.weight.grad, "g_b1": blk.pwconv1.bias.grad, "g_w2": blk.pwconv2.weight.grad,
            "g_b2": blk.pwconv2.bias.grad, "a": a.detach(), "grad_h": h.grad}


def main():
    for k, tag in enumerate(R.CASES):
        nhw, C, Hd, Co = R.CASES[tag]
        seed = 100 * k + 11
        ins = R.draw(tag, seed)
        ref = evaluate(*ins, torch.float64)
        f32 = evaluate(*ins, torch.float32)
        res = {"shape": np.array(list(nhw) + [C, Hd, Co], dtype=np.int64), "seed": np.int64(seed)}
        for n, t in zip(R.INPUTS, ins):
            assert t.dtype == torch.float32
            res[n] = t.numpy()
        for n in R.RESULTS + ("a", "grad_h"):
            assert ref[n].dtype == torch.float64 and f32[n].dtype == torch.float32 and torch.isfinite(ref[n]).all()
            if n in R.RESULTS:
                res[n] = ref[n].numpy()
            err = res[n + "_fp32_ref_err"] = np.float64(R.rel_err(f32[n], ref[n]))
            assert err > 0, (tag, n, err)
            print("%-8s %-8s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(ref[n].abs().max()), err))
        path = os.path.join(HERE, "pw_mlp_%s.npz" % tag)
        np.savez_compressed(path, **res)
        size = os.path.getsize(path)
        print("%-8s seed %d  %s %d bytes" % (tag, seed, path, size))
        assert size <= MAX_BYTES, "fixture of %d bytes" % size


if __name__ == "__main__":
    main()
