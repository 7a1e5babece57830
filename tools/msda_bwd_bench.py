"""MSDeformAttn forward + backward at Unicorn's geometry (maps (50,80) x 2 = 800x1280 at stride 16, M=8, D=32, Lq=8000, P=4), fp32,
N = 1 and N = 16: the HIP operator (unicorn_amd.ops.MSDeformAttnFunction: uni_msda_fwd / uni_msda_bwd) against what a user falls back
to without it, a torch-autograd statement of the op on F.grid_sample, on the same GPU and the same inputs.

Timing: device events around windows of back-to-back calls after a warm-up of every shape; REPS windows per variant, the two variants
alternating; min and median of the per-call time are reported.  Also written: the atomic bytes of one backward (every in-map corner of
every sample adds one D*4-byte row: N*Lq*M*L*P*4*D*4 when nothing leaves the map; counted exactly from the inputs too) and the floor
they set at the chip-wide float-atomic rate of ~1.3 TB/s of added bytes.

    python tools/msda_bwd_bench.py [--out profiles/msda_backward.txt] [--batches 1 16]

Exit status 1 when the HIP backward is slower than the fallback's at any batch size (the one condition the kernel has to meet)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from unicorn_amd.ops import MSDeformAttnFunction

SHAPES = [(50, 80), (50, 80)]
M, D, LQ, P = 8, 32, 8000, 4
ATOMIC_RATE = 1.3e12          # added bytes / s, chip-wide, global_atomic_add_f32 in 256-byte / 2 x 128-byte wave instructions
REPS = 7


def grid_sample_msda(value, shapes, loc, attn):
    """The op as bilinear grid sampling per level (zero padding, pixel centres at (i + 0.5) / n, i.e. align_corners=False) followed by
    the attention-weighted sum over levels and points."""
    N, S, Mh, Dh = value.shape
    Lq, L, Pn = loc.shape[1], loc.shape[3], loc.shape[4]
    start, sampled = 0, []
    for lvl, (H, W) in enumerate(shapes):
        v = value[:, start:start + H * W].permute(0, 2, 3, 1).reshape(N * Mh, Dh, H, W)
        start += H * W
        grid = (2 * loc[:, :, :, lvl] - 1).permute(0, 2, 1, 3, 4).reshape(N * Mh, Lq, Pn, 2)
        sampled.append(F.grid_sample(v, grid, mode="bilinear", padding_mode="zeros", align_corners=False))   # (N*M, D, Lq, P)
    w = attn.permute(0, 2, 1, 3, 4).reshape(N * Mh, 1, Lq, L * Pn)
    out = (torch.cat(sampled, -1) * w).sum(-1)                                   # (N*M, D, Lq)
    return out.view(N, Mh * Dh, Lq).transpose(1, 2).contiguous()


def atomic_rows(loc, shapes):
    """corner rows inside the map over all samples that pass the -1 < x < W, -1 < y < H rule = atomic row adds of one backward"""
    n = 0
    for lvl, (H, W) in enumerate(shapes):
        x = loc[:, :, :, lvl, :, 0].double() * W - 0.5
        y = loc[:, :, :, lvl, :, 1].double() * H - 0.5
        ok = (x > -1) & (y > -1) & (x < W) & (y < H)
        x0, y0 = torch.floor(x), torch.floor(y)
        for dy in (0, 1):
            for dx in (0, 1):
                n += int((ok & (y0 + dy >= 0) & (y0 + dy < H) & (x0 + dx >= 0) & (x0 + dx < W)).sum())
    return n


def windows(fns, iters):
    """REPS windows of `iters` calls per function, the functions alternating; per-call ms of every window"""
    res = [[] for _ in fns]
    for _ in range(REPS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters[i]):
                fn()
            e1.record()
            torch.cuda.synchronize()
            res[i].append(e0.elapsed_time(e1) / iters[i])
    return res


def one_batch(N, lines):
    g = torch.Generator().manual_seed(100 + N)
    S = sum(h * w for h, w in SHAPES)
    L = len(SHAPES)
    value = torch.randn(N, S, M, D, generator=g).cuda().requires_grad_(True)
    loc = (torch.rand(N, LQ, M, L, P, 2, generator=g) * 1.1 - 0.05).cuda().requires_grad_(True)
    attn = torch.softmax(torch.randn(N, LQ, M, L * P, generator=g), -1).view(N, LQ, M, L, P).cuda().requires_grad_(True)
    gout = torch.randn(N, LQ, M * D, generator=g).cuda()
    shp = torch.as_tensor(SHAPES, dtype=torch.long)
    lsi = torch.cat((shp.new_zeros((1,)), shp.prod(1).cumsum(0)[:-1]))
    ins = (value, loc, attn)

    def hip_fwd():
        return MSDeformAttnFunction.apply(value, shp, lsi, loc, attn, 64)

    def torch_fwd():
        return grid_sample_msda(value, SHAPES, loc, attn)

    def fwd_bwd(fwd):
        def run():
            torch.autograd.grad(fwd(), ins, gout)
        return run

    def bwd_only(fwd):
        out = fwd()

        def run():
            torch.autograd.grad(out, ins, gout, retain_graph=True)
        return run

    # the two statements agree (fp32, different operation order): a timing of different results would be worthless
    gh = torch.autograd.grad(hip_fwd(), ins, gout)
    gt = torch.autograd.grad(torch_fwd(), ins, gout)
    agree = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(gh, gt)]
    del gh, gt
    fns = [fwd_bwd(hip_fwd), fwd_bwd(torch_fwd), bwd_only(hip_fwd), bwd_only(torch_fwd)]
    for fn in fns:                                                                # warm-up of every shape
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    iters = []
    for fn in fns:                                                                # windows of ~0.25 s
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        iters.append(max(3, min(400, int(250.0 / max(e0.elapsed_time(e1), 1e-3)))))
    res = windows(fns, iters)
    rows = atomic_rows(loc.detach().cpu(), SHAPES)
    abytes, full = rows * D * 4, N * LQ * M * L * P * 4 * D * 4
    floor_ms = abytes / ATOMIC_RATE * 1e3
    names = ["HIP forward+backward", "torch grid_sample forward+backward", "HIP backward", "torch grid_sample backward"]
    lines.append("N = %d  (value %s, %d samples)" % (N, tuple(value.shape), N * LQ * M * L * P))
    for name, r, it in zip(names, res, iters):
        lines.append("  %-36s min %9.4f ms   median %9.4f ms   (%d windows of %d calls)" % (name, min(r), statistics.median(r), REPS, it))
    hb, tb = statistics.median(res[2]), statistics.median(res[3])
    lines.append("  atomic bytes per backward            %d (%.1f MB; %d if no corner left the map)" % (abytes, abytes / 1e6, full))
    lines.append("  floor at 1.3 TB/s of added bytes     %9.4f ms   -> HIP backward (median) = %.2f x the floor" % (floor_ms, hb / floor_ms))
    lines.append("  torch backward / HIP backward        %.2f x (median);  forward+backward %.2f x" %
                 (tb / hb, statistics.median(res[1]) / statistics.median(res[0])))
    lines.append("  max |HIP - torch| / max |torch|      grad_value %.2e, grad_sampling_loc %.2e, grad_attn_weight %.2e" % tuple(agree))
    return hb <= tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "msda_backward.txt"))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("msda_bwd_bench: needs a GPU (a CPU timing says nothing about the kernel)")
    lines = ["MSDeformAttn backward, fp32, maps (50,80) x 2, M=8, D=32, Lq=8000, P=4 -- tools/msda_bwd_bench.py on %s"
             % torch.cuda.get_device_name(0),
             "times: device events, warm-up of every shape, %d alternating windows per variant, per-call min / median" % REPS, ""]
    ok = True
    for N in a.batches:
        ok = one_batch(N, lines) and ok
        lines.append("")
    lines.append("condition (HIP backward not slower than the torch fallback at every batch size): %s" % ("holds" if ok else "VIOLATED"))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
