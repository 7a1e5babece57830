"""Golden vectors for the differentiable downsample layers (uni_down_train_*, uni_patch4_*, ops.downsample_ln, ops.stem_conv), produced by
EXECUTING the reference's own layers on the CPU: ConvNeXt(in_chans, depths=[1, 1, 1, 1], dims=[C, Co, 4, 4]).downsample_layers[0] (the stem:
Conv2d 4/4, LayerNorm -- the convolution alone is run) and .downsample_layers[1] (LayerNorm eps 1e-6 channels_first, Conv2d 2/2, padding 0)
(unicorn/models/backbone/convnext.py:77-87) get the drawn parameters and are run under autograd with a drawn upstream gradient, in fp64 for
the results and in fp32 for the yardstick.  Per result, <name>_fp32_ref_err = max|fp32 - fp64| / max|fp64| of the same layer in fp32: the
bound of the fp32 GPU test is 4 x that (no figure comes from the kernel) and it must be > 0.  Inputs are stored as fp32, results as fp64.  No
reference text is stored.

    python tests/golden/make_golden_down_train.py        -> tests/golden/down_train_<case>.npz, tests/golden/stem_conv_<case>.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "oracle"))
sys.path.insert(0, os.path.join(HERE, ".."))

import down_train_ref as R  # noqa: E402

MAX_BYTES = 360 * 1024


def reference_layers(in_chans, C, Co, dtype):
    import ref_bootstrap
    ref_bootstrap.boot()
    from unicorn.models.backbone.convnext import ConvNeXt
    net = ConvNeXt(in_chans=in_chans, depths=[1, 1, 1, 1], dims=[C, Co, 4, 4])
    stem, down = net.downsample_layers[0].to(dtype), net.downsample_layers[1].to(dtype)
    conv4, norm, conv2 = stem[0], down[0], down[1]
    assert isinstance(conv4, torch.nn.Conv2d) and conv4.kernel_size == conv4.stride == (4, 4) and conv4.padding == (0, 0)
    assert isinstance(conv2, torch.nn.Conv2d) and conv2.kernel_size == conv2.stride == (2, 2) and conv2.padding == (0, 0)
    assert norm.data_format == "channels_first" and norm.eps == R.EPS and tuple(norm.weight.shape) == (C,)
    return conv4, down


def evaluate(ins, dtype):
    x, ln_weight, ln_bias, weight, bias, grad_out = ins
    _, down = reference_layers(3, x.shape[1], weight.shape[0], dtype)
    with torch.no_grad():
        down[0].weight.copy_(ln_weight.to(dtype)), down[0].bias.copy_(ln_bias.to(dtype))
        down[1].weight.copy_(weight.to(dtype)), down[1].bias.copy_(bias.to(dtype))
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    y = down(xl)
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_x": xl.grad, "g_ln_weight": down[0].weight.grad, "g_ln_bias": down[0].bias.grad, "g_weight": down[1].weight.grad,
            "g_bias": down[1].bias.grad}


def evaluate_stem(ins, dtype):
    x, weight, bias, grad_out = ins
    conv4, _ = reference_layers(x.shape[1], weight.shape[0], 4, dtype)
    with torch.no_grad():
        conv4.weight.copy_(weight.to(dtype)), conv4.bias.copy_(bias.to(dtype))
    xl = x.detach().to(dtype).clone().requires_grad_(True)
    y = conv4(xl)
    y.backward(grad_out.to(dtype))
    return {"y": y.detach(), "g_x": xl.grad, "g_weight": conv4.weight.grad, "g_bias": conv4.bias.grad}


def write(tag, seed, shape, ins, names, results, ev):
    ref, f32 = ev(ins, torch.float64), ev(ins, torch.float32)
    res = {"shape": np.array(shape, dtype=np.int64), "seed": np.int64(seed)}
    for n, t in zip(names, ins):
        assert t.dtype == torch.float32
        res[n] = t.numpy()
    for n in results:
        assert ref[n].dtype == torch.float64 and f32[n].dtype == torch.float32 and torch.isfinite(ref[n]).all()
        res[n] = ref[n].numpy()
        err = res[n + "_fp32_ref_err"] = np.float64(R.rel_err(f32[n], ref[n]))
        assert 0 < err < 1e-3, (tag, n, err)
        print("%-10s %-12s max|ref| %.4g  fp32_ref_err %.3g" % (tag, n, float(ref[n].abs().max()), err))
    path = os.path.join(HERE, R.fixture_name(tag))
    np.savez_compressed(path, **res)
    size = os.path.getsize(path)
    print("%-10s seed %d  %s %d bytes" % (tag, seed, path, size))
    assert size <= MAX_BYTES, "fixture of %d bytes" % size


def main():
    for k, tag in enumerate(R.CASES):
        shape, Co = R.CASES[tag]
        seed = 100 * k + 17
        write(tag, seed, shape + (Co,), R.draw(tag, seed), R.INPUTS, R.RESULTS, evaluate)
    for k, tag in enumerate(R.STEM_CASES):
        shape, Co = R.STEM_CASES[tag]
        seed = 100 * k + 19
        write(tag, seed, shape + (Co,), R.draw_stem(tag, seed), R.STEM_INPUTS, R.STEM_RESULTS, evaluate_stem)


if __name__ == "__main__":
    main()
