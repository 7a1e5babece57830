"""The four downsample layers of the ConvNeXt backbone in training (unicorn/models/backbone/convnext.py:77-87), forward + backward with all
gradients, at their sites in unicorn_track_large at 800 x 1280 with the two frames of one sample: the stem (2, 3, 800, 1280) -> 192 and the
three norm + 2x2 / stride-2 convolutions (2, 192, 200, 320) -> 384, (2, 384, 100, 160) -> 768, (2, 768, 50, 80) -> 1536; fp32 and fp16 autocast.

Part 1, the operator against what the parent path runs at that site in a model fused with fuse_model: ops.layernorm_cf on the channels-last
x that ops.block_tail wrote, the eager Conv2d, and the .contiguous(memory_format=channels_last) that the next block's ops.dwconv7_ln performs
on the NCHW map the convolution returns; for the stem the eager Conv2d and ops.layernorm_cf on its output.  The fused path is
ops.downsample_ln alone; for the stem ops.stem_conv and ops.layernorm_cf.
Part 2, a stand-in stage: the downsample layer + three blocks (tests/block_tail_ref.py StandInBlock) + output norm with fuse_model_down
against fuse_model.

HIP events around every call, 3 warm-up calls, two alternating windows in the same run, median of the timed calls (both windows are printed:
their spread is the margin); kernel launches of one call and the sum of their device times from torch.profiler (a run of its own; copies and
fills left out); peak memory of one call; bytes allocated between forward and backward (the output included).  Part 0 lists registers, LDS
and scratch of every kernel variant of unicorn_amd/csrc/down_train.hip from the compiler's kernel-resource-usage remarks.

    python tools/down_train_bench.py [--runs 20] [--out profiles/down_train.txt] [--remarks FILE]

--remarks: the stderr of `hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -c down_train.hip`; without it the
tool runs that compile itself.
"""
import argparse
import copy
import os
import re
import subprocess
import sys
import tempfile

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import down_train_ref as R  # noqa: E402
from block_tail_bench import device_of  # noqa: E402
from block_tail_ref import StandInBlock  # noqa: E402
from dwln_train_bench import peak_of, timed  # noqa: E402
from lncf_ref import StandInNorm  # noqa: E402
from unicorn_amd import nn as unn, ops  # noqa: E402

CL = torch.channels_last
# (site, (N, C, H, W), Co)
SITES = (("stem", (2, 3, 800, 1280), 192), ("downsample 1", (2, 192, 200, 320), 384), ("downsample 2", (2, 384, 100, 160), 768),
         ("downsample 3", (2, 768, 50, 80), 1536))


def variant_name(mangled):
    """`_Z12ln_cl_kernelIfDF16_Li8ELi3ELi0E6DownIOEv...` -> `ln_cl_kernel<f32,f16,8,3,0,DownIO>` (the few Itanium codes these kernels use)"""
    m = re.match(r"_Z(\d+)", mangled)
    if not m:
        return mangled
    end = m.end() + int(m.group(1))
    name, rest, args = mangled[m.end():end], mangled[end:], []
    if not rest.startswith("I"):
        return name
    rest = rest[1:]
    codes = (("DF16_", "f16"), ("DF16b", "bf16"), ("f", "f32"), ("d", "f64"))
    while rest and not rest.startswith("E"):
        lit = re.match(r"L[ib](\d+)E", rest)
        if lit:
            args.append(lit.group(1))
            rest = rest[lit.end():]
            continue
        named = re.match(r"(\d+)", rest)                           # a class that is no template: the policy of ln_cl_kernel
        if named:
            end = named.end() + int(named.group(1))
            args.append(rest[named.end():end])
            rest = rest[end:]
            continue
        for code, text in codes:
            if rest.startswith(code):
                args.append(text)
                rest = rest[len(code):]
                break
        else:
            return mangled
    return "%s<%s>" % (name, ",".join(args))


def resources(say, remarks):
    csrc = os.path.join(ROOT, "unicorn_amd", "csrc")
    if remarks:
        text = open(remarks).read()
    else:
        with tempfile.TemporaryDirectory() as tmp:
            text = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wno-unused-result",
                                   "-Rpass-analysis=kernel-resource-usage", "-c", "down_train.hip", "-o", os.path.join(tmp, "down_train.o")],
                                  cwd=csrc, stderr=subprocess.PIPE, check=True).stderr.decode()
    kernels, cur = [], None
    for line in text.splitlines():
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"name": m.group(2)}
            kernels.append(cur)
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    names = [variant_name(k["name"]) for k in kernels]
    say("kernel variants of down_train.hip (gfx950, -O3): VGPRs / AGPRs / SGPRs, LDS bytes per block (static; the backward with partials adds")
    say("16 C bytes of dynamic LDS), scratch bytes per lane, waves per SIMD.  Template arguments: <T, XT, V, NV, MODE, policy> (csrc/ln_cl.h; MODE 0")
    say("forward and rebuild, 1 backward) and <XT, AT, SCATTER>.")
    for k, n in zip(kernels, names):
        short = n
        say("  %-48s VGPR %3s AGPR %3s SGPR %3s  LDS %5s  scratch %s  occupancy %s"
            % (short, k.get("VGPRs"), k.get("AGPRs"), k.get("TotalSGPRs"), k.get("LDS Size"), k.get("ScratchSize"), k.get("Occupancy")))
    spill = [n for k, n in zip(kernels, names) if k.get("ScratchSize") != "0"]
    say("%d variants; variants that use scratch: %s" % (len(kernels), ", ".join(spill) or "none"))


def windows(a, b, runs):
    """medians of a and b in two alternating windows each -> ((a1, a2), (b1, b2))"""
    a1, b1 = timed(a, runs)[1], timed(b, runs)[1]
    a2, b2 = timed(a, runs)[1], timed(b, runs)[1]
    return (a1, a2), (b1, b2)


def held_of(fwd):
    """bytes allocated by one forward and still alive before its backward (the output included), in MB"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    y = fwd()
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    del y
    return held / 1e6


def line(say, what, mode, tf, tp, fused, parent, held, slower, slower_dev, key):
    (lf, df), (lp, dp) = device_of(fused), device_of(parent)
    mf, mp = sum(tf) / 2, sum(tp) / 2
    flag = ""
    if mp < mf:
        flag += "   SLOWER"
        slower.append(key)
    if dp < df:
        flag += "   SLOWER ON THE DEVICE"
        slower_dev.append(key)
    say("  %-13s %-13s fused %7.3f / %7.3f ms call, %7.3f ms device in %2d launches, peak %7.1f MB, held %7.1f MB   parent %7.3f / %7.3f ms call, "
        "%7.3f ms device in %2d launches, peak %7.1f MB, held %7.1f MB   parent / fused %.2f x call, %.2f x device%s"
        % (what, mode, tf[0], tf[1], df, lf, peak_of(fused), held[0], tp[0], tp[1], dp, lp, peak_of(parent), held[1], mp / mf, dp / df, flag))


def operator_part(say, runs):
    slower, slower_dev = [], []
    for site, shape, Co in SITES:
        N, C, H, W = shape
        stem = site == "stem"
        k = 4 if stem else 2
        g = torch.Generator().manual_seed(C)
        x = torch.randn(shape, generator=g).cuda()
        cw = (torch.randn(Co, C, k, k, generator=g) / (k * k * C) ** 0.5).cuda().requires_grad_(True)
        cb = (0.1 * torch.randn(Co, generator=g)).cuda().requires_grad_(True)
        Cn = Co if stem else C
        lw = (1.0 + 0.1 * torch.randn(Cn, generator=g)).cuda().requires_grad_(True)
        lb = (0.1 * torch.randn(Cn, generator=g)).cuda().requires_grad_(True)
        if not stem:
            x = x.contiguous(memory_format=CL).requires_grad_(True)
        go = torch.randn(N, Co, H // k, W // k, generator=g).cuda().contiguous(memory_format=CL)
        for autocast in (False, True):
            def clear():
                x.grad = cw.grad = cb.grad = lw.grad = lb.grad = None

            def fwd_fused():
                with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                    if stem:
                        return ops.layernorm_cf(ops.stem_conv(x, cw, cb), lw, lb, R.EPS)
                    return ops.downsample_ln(x, lw, lb, cw, cb, R.EPS)

            def fwd_parent():
                with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                    if stem:
                        return ops.layernorm_cf(F.conv2d(x, cw, cb, stride=4), lw, lb, R.EPS)
                    return F.conv2d(ops.layernorm_cf(x, lw, lb, R.EPS), cw, cb, stride=2).contiguous(memory_format=CL)

            def fused():
                clear()
                y = fwd_fused()
                y.backward(go.to(y.dtype))

            def parent():
                clear()
                y = fwd_parent()
                y.backward(go.to(y.dtype))

            tf, tp = windows(fused, parent, runs)
            mode = "fp16 autocast" if autocast else "fp32"
            line(say, site, mode, tf, tp, fused, parent, (held_of(fwd_fused), held_of(fwd_parent)), slower, slower_dev, (site, mode))
    say()
    say("operator slower than the parent path by call time at: %s" % ("; ".join("%s %s" % s for s in slower) or "no measured case"))
    say("operator slower than the parent path by device time at: %s" % ("; ".join("%s %s" % s for s in slower_dev) or "no measured case"))


def stage_part(say, runs):
    slower, slower_dev = [], []
    for site, shape, Co in SITES:
        N, C, H, W = shape
        stem = site == "stem"
        k = 4 if stem else 2
        torch.manual_seed(Co)
        if stem:
            down = nn.Sequential(nn.Conv2d(C, Co, kernel_size=4, stride=4), StandInNorm(Co, data_format="channels_first"))
        else:
            down = nn.Sequential(StandInNorm(C, data_format="channels_first"), nn.Conv2d(C, Co, kernel_size=2, stride=2))
        proto = nn.Sequential(down, *(StandInBlock(Co) for _ in range(3)), StandInNorm(Co, data_format="channels_first")).cuda().train()
        x = torch.randn(shape, device="cuda")
        if not stem:
            x = x.contiguous(memory_format=CL)                     # the output of the stage before
        t = torch.randn(N, Co, H // k, W // k, device="cuda")
        for autocast in (False, True):
            a, b = copy.deepcopy(proto), copy.deepcopy(proto)
            assert unn.fuse_model_down(a)[-1] == 1
            unn.fuse_model(b)

            def step(net):
                def fn():
                    net.zero_grad(set_to_none=True)
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        out = net(x)
                    (out * t).sum().backward()
                return fn

            def fwd(net):
                def fn():
                    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
                        return net(x)
                return fn

            fused, parent = step(a), step(b)
            tf, tp = windows(fused, parent, runs)
            mode = "fp16 autocast" if autocast else "fp32"
            line(say, "stage " + site, mode, tf, tp, fused, parent, (held_of(fwd(a)), held_of(fwd(b))), slower, slower_dev, (site, mode))
            del a, b
    say()
    say("stage with fuse_model_down slower than with fuse_model by call time at: %s" % ("; ".join("%s %s" % s for s in slower) or "no measured case"))
    say("stage with fuse_model_down slower than with fuse_model by device time at: %s" % ("; ".join("%s %s" % s for s in slower_dev) or "no measured case"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--remarks", default=None)
    ap.add_argument("--part", choices=("resources", "operator", "stage", "all"), default="all")
    args = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    if args.part in ("resources", "all"):
        resources(say, args.remarks)
        say()
    if args.part != "resources":
        assert torch.cuda.is_available(), "the measurement needs a HIP device"
        say("Downsample layers, training (forward + backward, all gradients) -- tools/down_train_bench.py on %s" % torch.cuda.get_device_name(0))
        say("fused = ops.downsample_ln (stem: ops.stem_conv + ops.layernorm_cf); parent = ops.layernorm_cf + eager Conv2d + the channels-last conversion of")
        say("the next block (stem: eager Conv2d + ops.layernorm_cf).  HIP events, 3 warm-up calls, median of %d calls in each of two alternating windows" % args.runs)
        say("(both printed; the ratio is of their means).  held: MB allocated by the forward and alive before the backward, the output included.")
    if args.part in ("operator", "all"):
        say()
        operator_part(say, args.runs)
    if args.part in ("stage", "all"):
        say()
        stage_part(say, args.runs)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
