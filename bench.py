#!/usr/bin/env python
"""bench.py - frames/s of Unicorn's per-frame step on MI355X (BASELINE.json metric).

A "step" = NB consecutive frames of one video stream through the hot path (SURVEY.md §8d unit of work): ConvNeXt+PAFPN on
the current frames, ref<->cur deformable interaction, 2x embedding upsample, dense HWxHW correlation + prior propagation,
prior pyramid, unified head.  The reference-frame backbone is cached (computed once, external/lib/test/tracker/
unicorn_sot.py:49) and is outside the timed region, as are H2D copies: frames are resident in HBM before timing starts.
Weights: synthetic (oracle/synth.py), data: synthetic clip.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--precision f16x2|bf16|fp32] [--model ...] [--task sot|mot|vos]
                    [--dump-outputs DIR] [--full]

A plain run sets up, runs W warm-up steps, times exactly K steps, writes the outputs of the last timed step if --dump-outputs
is given, and prints one JSON line (`value` = frames/s, `ms_per_step` = milliseconds of one timed step).  Everything else
(roofline / per-kernel-class leg, single-frame leg, CPU baseline + in-run parity, golden margin log, other precisions and
configs, clock / power sensor, the N > 1 RLE gather check) runs only with --full; the --no-* / --with-* switches select
within --full.

HEADLINE = precision "f16x2" (fp32-equivalent split-f16 MFMA operands): the fastest mode that meets the parity bar of
BASELINE.json:north_star (box/mask IoU >= 0.999, embedding cosine within 1e-4), checked in a --full run against the CPU
oracle ("parity" key).  The bf16 mode (1 MFMA per product, misses box IoU with 8 operand bits) is reported next to it under
"modes", the other BASELINE configs under "configs".

--gpus N > 1 without a torchrun environment re-launches itself as `python -m torch.distributed.run --nproc-per-node N`:
one process per GPU, one independent video stream per rank (streams shard one-per-GPU, no data-path
collective; RCCL all_gather only for the result rows, external/lib/test/evaluation/running.py:111-120).
"""
import argparse
import contextlib
import json
import os
import socket
import subprocess
import sys
import time

# torch's OpenMP team spin-waits after every parallel CPU region; inside a CPU-quota'd container those spinning threads can
# exhaust the quota and freeze the HIP dispatch thread for tens of ms (measured: periodic 45 ms GPU-idle gaps).  The timed
# path has no large CPU tensor ops, and the oracle leg is bracketed by set_num_threads; passive waiting removes the rest.
os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")
ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model", default="unicorn_track_large")
    ap.add_argument("--task", default="sot", choices=["sot", "mot", "vos", "mix"],
                    help="mix = BASELINE.json configs[4]: rank r runs the MOT loop (evaluate_omni) if r < N/2, the SOT step otherwise")
    ap.add_argument("--gather-every", type=int, default=4, help="steps between the in-run RCCL gathers of the result rows (N > 1)")
    ap.add_argument("--precision", default="f16x2", choices=["f16x2", "bf16", "fp32"])
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--batch", type=int, default=16, help="frames of the stream processed per step (time-batched: the SOT step of a "
                    "frame depends only on the cached reference frame, unicorn_sot.py:78-108, so consecutive frames are independent)")
    ap.add_argument("--corr-precision", type=int, default=2, choices=[0, 1, 2, 3],
                    help="0 = fp32 MFMA correlation, 1 = fp32-equivalent bf16x3 split, 2 = fp32-equivalent f16x2 split (default), "
                         "3 = the reference driver's fp16 arithmetic class (not a parity mode)")
    ap.add_argument("--cpu-frames", type=int, default=4, help="frames of the CPU baseline / in-run parity leg (min / median / mean reported)")
    ap.add_argument("--rccl-probe", action="store_true", help=argparse.SUPPRESS)      # child process of init_dist(): RCCL rendezvous + collectives, then exit
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the oracle leg (cpu_baseline AND in-run parity)")
    ap.add_argument("--no-extras", action="store_true", help="headline + roofline only (no modes / configs sub-results)")
    ap.add_argument("--no-single-frame", action="store_true", help="skip the one-frame-per-call leg (clean per-kernel averages under rocprofv3)")
    ap.add_argument("--with-bf16", action="store_true", help="also time the bf16 operand mode (1 MFMA per product).  Retired from the default line: it "
                    "misses the box-IoU bar with the synthetic AND the trained-like weight ensembles (profiles/r04_precision_budget_trained_like_*.json)")
    ap.add_argument("--no-torch-rocm-port", dest="torch_rocm_port", action="store_false", help="skip the PyTorch-ROCm port leg: by default the cpu_baseline leg also "
                    "times the oracle port through PLAIN PyTorch-ROCm (eager MIOpen / rocBLAS ops) on this GPU, in a child process with a timeout (~20 s); reported "
                    "inside cpu_baseline as context (what the hand-written path is worth next to the framework's own kernels) -- never `value`")
    ap.add_argument("--torch-rocm-port", dest="torch_rocm_port", action="store_true", help=argparse.SUPPRESS)      # (round-6 scripts pass it explicitly)
    ap.set_defaults(torch_rocm_port=True)
    ap.add_argument("--torch-rocm-port-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-pmc", action="store_true", help="do not collect the HBM-side traffic of the dominant kernel class in this run (two child passes of "
                    "`rocprofv3 --kernel-trace --pmc FETCH_SIZE | WRITE_SIZE` over a 3-step run of this script, ~70 s; N = 1 and without --no-extras only); "
                    "`roofline.traffic` then replays the committed passes under profiles/")
    ap.add_argument("--launch-check", action="store_true", help="only rendezvous (gloo on CPU, RCCL on GPUs) and report the world size")
    ap.add_argument("--full", action="store_true", help="also run every leg beyond the headline: roofline (+ HBM traffic passes), single-frame, CPU "
                    "baseline + in-run parity (+ PyTorch-ROCm port), golden margin log, other precisions / configs, clock / power sensor, N > 1 RLE "
                    "gather check")
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed step returned as DIR/<name>.npy "
                    "(float32 / float64; rank 0; at most 64 MB: an output too large for its share is stored as a fixed seeded sample, <name>_sample.npy)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def self_launch(args):
    """--gpus N > 1 outside torchrun: one process per GPU (running.py:111-120), rendezvous on 127.0.0.1."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def torch_rocm_port_child(args):
    """`bench.py --torch-rocm-port-child`: the oracle (oracle/unicorn_oracle.py, the pinned restatement of the reference's fp32 PyTorch path; MSDA through
    the reference's pure-PyTorch grid_sample formulation, ops/functions/ms_deform_attn_func.py:41-61) executed by PyTorch-ROCm's own eager kernels on cuda:0:
    the same SOT step, same synthetic weights and frames, fp32 and (if it runs) with .half() weights / inputs like `tools/track.py --fp16`.  The reference
    tree itself cannot travel to the GPU box; this is its port on the framework's kernels.  Baseline leg only (never the product path).  Prints one JSON line."""
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import synth
    import unicorn_oracle as uo
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    cfg = uo.CONFIGS[args.model]
    P32 = {k: v.to(dev) for k, v in synth.synth_state_dict(cfg).items()}
    frames, box = synth.synth_clip(H, W, 4, seed=1)
    out = {"model": args.model, "size": [H, W], "torch": torch.__version__, "device": torch.cuda.get_device_name(0)}
    fr32 = [f.to(dev) for f in frames]

    def timed(fn):
        with torch.no_grad(), torch.device(dev):
            t0 = time.perf_counter()
            for i in range(2):
                fn(i)
            torch.cuda.synchronize()
            warm = time.perf_counter() - t0
            ts = []
            for i in range(args.cpu_frames + 2):
                t1 = time.perf_counter()
                r = fn(i)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t1)
        ts.sort()
        return r, {"ms_per_frame_min": round(1e3 * ts[0], 2), "ms_per_frame_median": round(1e3 * ts[len(ts) // 2], 2), "fps": round(1.0 / ts[len(ts) // 2], 2),
                   "frames": len(ts), "warmup_s_incl_kernel_selection": round(warm, 1)}
    # (1) the SOT step (unicorn_sot.py:78-108), fp32 -- the reference SOT driver keeps the model in fp32 (only the correlation is cast to fp16)
    try:
        with torch.no_grad(), torch.device(dev):
            st = uo.sot_init(P32, cfg, fr32[0], box.to(dev))
        r, out["sot_step_fp32"] = timed(lambda i: uo.sot_step(P32, cfg, st, fr32[1 + i % 3]))
        hd = r["head"][0] if cfg.mask else r["head"]
        out["sot_step_fp32"]["finite"] = bool(torch.isfinite(hd.float()).all())
    except Exception as e:                      # noqa: BLE001
        out["sot_step_fp32"] = {"error": repr(e)[:300]}
    # (2) mode="whole" (backbone + FPN + head: the MOT entry, mot_evaluator.py:199), fp32 and with .half() weights / inputs = `tools/track.py --fp16`
    # (mot_evaluator.py:126-128; the interaction is never run in half by the reference: its MSDA op dispatches float / double only)
    for name, cast in (("whole_fp32", lambda t: t), ("whole_half", lambda t: t.half() if torch.is_floating_point(t) else t)):
        try:
            P = {k: cast(v) for k, v in P32.items()}
            fr = [cast(f) for f in fr32]
            r, out[name] = timed(lambda i: uo.mot_whole(P, cfg, fr[1 + i % 3]))
            hd = r[0][0] if cfg.mask else r[0]
            out[name]["finite"] = bool(torch.isfinite(hd.float()).all())
        except Exception as e:                  # noqa: BLE001 -- e.g. an op without a half kernel: reported, not fatal
            out[name] = {"error": repr(e)[:300]}
    print(json.dumps(out), flush=True)
    sys.exit(0)


def measure_pmc_traffic(args, H, W):
    """HBM-side bytes per launch of the GEMM class of `args.precision`, measured by THIS run: two SEPARATE `rocprofv3 --kernel-trace --pmc <counter>` passes
    (FETCH_SIZE, WRITE_SIZE; MI355X_MICROARCH.md: separate passes, KiB units, FETCH_SIZE doubled on gfx950) over a 3-step child run of this script, aggregated per
    kernel class exactly like tools/pmc_traffic.py.  -> (bytes per launch | None, detail dict)"""
    import glob
    import shutil
    import sqlite3
    import tempfile
    if not shutil.which("rocprofv3"):
        return None, {"error": "rocprofv3 not on PATH"}
    base = tempfile.mkdtemp(prefix="uni_pmc_", dir="/tmp")
    per, t0 = {}, time.perf_counter()
    try:
        for tag, ctr in (("fetch", "FETCH_SIZE"), ("write", "WRITE_SIZE")):
            d = os.path.join(base, tag)
            cmd = ["rocprofv3", "--kernel-trace", "--pmc", ctr, "-d", d, "-o", "p", "--", sys.executable, os.path.abspath(__file__), "--steps", "3", "--warmup", "1",
                   "--full", "--no-cpu-baseline", "--no-extras", "--no-single-frame", "--no-pmc", "--model", args.model, "--height", str(H), "--width", str(W),
                   "--batch", str(args.batch), "--precision", args.precision, "--task", args.task]
            cp = subprocess.run(cmd, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True,
                                timeout=float(os.environ.get("UNI_BENCH_PMC_TIMEOUT", "240")))
            dbs = glob.glob(d + "/**/*results.db", recursive=True)
            if cp.returncode != 0 or not dbs:
                return None, {"error": "rocprofv3 pass %s failed (rc %d): %s" % (ctr, cp.returncode, (cp.stderr or cp.stdout)[-200:])}
            tot, n = 0.0, 0
            for f in dbs:
                for name, cname, val in sqlite3.connect(f).execute("select kernel_name, counter_name, value from counters_collection"):
                    k = name.split("(")[0]
                    hit = ("gemm_h2" in k or "mlp_fused" in k) if args.precision == "f16x2" else ("gemm_bf16" in k if args.precision == "bf16" else "gemm_f32" in k)
                    if cname == ctr and hit:
                        tot += float(val) * 1024.0 * (2.0 if tag == "fetch" else 1.0)
                        n += 1
            per[tag] = (tot / max(n, 1), n)
    except Exception as e:                          # noqa: BLE001 -- a measurement aid must not take the bench line down
        return None, {"error": repr(e)[:200]}
    finally:
        shutil.rmtree(base, ignore_errors=True)
    if not per.get("fetch", (0, 0))[1] or not per.get("write", (0, 0))[1]:
        return None, {"error": "no GEMM-class rows in the counter passes"}
    return round(per["fetch"][0] + per["write"][0]), {"fetch_bytes_per_launch": round(per["fetch"][0]), "write_bytes_per_launch": round(per["write"][0]),
                                                      "launches_counted": [per["fetch"][1], per["write"][1]], "seconds": round(time.perf_counter() - t0, 1),
                                                      "method": "two separate child passes: rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE -- bench.py --steps 3 --warmup 1 "
                                                                "(FETCH_SIZE x 2: gfx950 correction; KiB units)"}


def rccl_probe_child():
    """`bench.py --rccl-probe` (spawned by init_dist, one per rank, own rendezvous port): the first contact with RCCL happens in a
    process that may hang or crash without taking the bench down.  all_reduce + all_gather on device tensors; prints RCCL_PROBE_OK."""
    import datetime
    import torch
    import torch.distributed as dist
    rank, world, lr = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("UNI_BENCH_PROBE_FAIL"):       # test hook: a probe that dies
        sys.exit(3)
    gpu = torch.cuda.is_available()
    if gpu:
        torch.cuda.set_device(lr % torch.cuda.device_count())
    dist.init_process_group("nccl" if gpu else "gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    dev = "cuda" if gpu else "cpu"
    t = torch.ones(1 << 16, device=dev)
    dist.all_reduce(t)
    parts = [torch.zeros(8, 8, device=dev) for _ in range(world)]
    dist.all_gather(parts, torch.full((8, 8), float(rank), device=dev))
    if gpu:
        torch.cuda.synchronize()
    ok = float(t[0]) == world and all(float(p_[0, 0]) == r_ for r_, p_ in enumerate(parts))
    dist.destroy_process_group()
    print("RCCL_PROBE_OK" if ok else "RCCL_PROBE_BAD_DATA", flush=True)
    sys.exit(0 if ok else 4)


class _StdoutToStderr:
    """fd-level redirect of stdout to stderr while a C++ library chats (gloo prints "[Gloo] Rank r is connected to ..." on fd 1 when a
    group forms): the driver reads ONE JSON line from stdout."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *a):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def init_dist(rank, local_rank, world, gpu):
    """Control plane = gloo (CPU tensors, always works, every collective has a timeout); data plane (result-row / RLE gathers) = RCCL
    when a child-process probe succeeded ON EVERY RANK, gloo on host copies otherwise -- the first RCCL contact of this code is the
    driver's scaling run, so a failing or hanging RCCL must degrade the gather, not lose the measurement (the per-frame path has no
    data-path collective).  -> (dist module, data group | None, info dict)"""
    import datetime
    import torch
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL / cross-process device memory needs it on this host driver
    os.environ.setdefault("NCCL_DEBUG", "WARN")
    with _StdoutToStderr():
        dist.init_process_group(backend="gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=900))
        dist.barrier()          # forms the gloo connections (and their chatter) here, not at the first collective of the run
    info = {"control": "gloo", "data": "gloo", "rccl_probe": None, "env": {"NCCL_DEBUG": os.environ.get("NCCL_DEBUG"),
            "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY")}}
    want = os.environ.get("UNI_BENCH_BACKEND") or ("nccl" if gpu else "gloo")
    if want != "nccl" and not os.environ.get("UNI_BENCH_PROBE"):
        return dist, None, info
    ndev = torch.cuda.device_count() if gpu else 0
    if want == "nccl" and ndev < world and not os.environ.get("UNI_BENCH_FORCE_PROBE"):
        # one-GPU-visible guard: RCCL needs ONE device per rank ("Duplicate GPU detected" otherwise); with fewer visible GPUs than ranks
        # (UNI_BENCH_SHARE_GPU plumbing runs on a 1-GPU box) the probe cannot succeed -- skip it and SAY why, the gathers run over gloo
        why = ("RCCL skipped: %d rank(s) but %d visible GPU(s) -- RCCL binds one device per rank; result-row / RLE gathers run over gloo on host copies"
               % (world, ndev))
        print("[bench] " + why, file=sys.stderr, flush=True)
        info["rccl_probe"] = {"ok_all_ranks": False, "ok_this_rank": False, "seconds": 0.0, "msg": None, "why": why, "skipped": True}
        return dist, None, info
    port = torch.zeros(1, dtype=torch.int64)
    if rank == 0:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port[0] = s.getsockname()[1]
    dist.broadcast(port, 0)
    # torchrun marks its workers as clients of the agent's store (TORCHELASTIC_USE_AGENT_STORE): the probe group needs its own store on
    # its own port, created by its rank 0
    env = {k: v for k, v in os.environ.items() if not k.startswith("TORCHELASTIC_") and k != "TORCH_NCCL_ASYNC_ERROR_HANDLING"}
    env.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(int(port[0])), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(local_rank))
    t0 = time.perf_counter()
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rccl-probe"], env=env, stdout=subprocess.PIPE,
                             stderr=subprocess.STDOUT, text=True)
    try:
        out, _ = child.communicate(timeout=float(os.environ.get("UNI_BENCH_PROBE_TIMEOUT", "240")))
        ok, msg = child.returncode == 0 and "RCCL_PROBE_OK" in out, out[-400:]
    except subprocess.TimeoutExpired:
        child.kill()                                   # this exact child only
        out, _ = child.communicate()
        ok, msg = False, "timeout; " + (out or "")[-300:]
    flag = torch.tensor([1 if ok else 0], dtype=torch.int64)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    info["rccl_probe"] = {"ok_all_ranks": bool(int(flag[0])), "ok_this_rank": ok, "seconds": round(time.perf_counter() - t0, 1),
                          "msg": None if ok else msg, "skipped": False,
                          "why": None if int(flag[0]) else ("RCCL probe failed on %s: gathers run over gloo on host copies"
                                                            % ("this rank" if not ok else "another rank"))}
    group = None
    if int(flag[0]) and want == "nccl":
        try:
            with _StdoutToStderr():
                group = dist.new_group(backend="nccl", timeout=datetime.timedelta(seconds=300))
                w = torch.ones(1, device="cuda")
                dist.all_reduce(w, group=group)
                torch.cuda.synchronize()
            info["data"] = "nccl"
        except Exception as e:                       # noqa: BLE001 -- anything RCCL throws here degrades to the gloo gather
            info["rccl_probe"]["msg"] = "new_group(nccl) failed after a good probe: %r" % (e,)
            group = None
    return dist, group, info


def rank_task(task, model, rank, world):
    """BASELINE.json configs[4] ("MOT+SOT mix"): with --task mix the first half of the ranks run the MOT loop (evaluate_omni on the
    MOT17-style model, num_classes = 1), the second half the SOT step; a single rank runs SOT.  -> (task, model) of this rank."""
    if task != "mix":
        return task, model
    t = "mot" if rank < world // 2 else "sot"
    if t == "mot" and model == "unicorn_track_large":
        model = "unicorn_track_large_mot_challenge"
    return t, model


def make_gather(rank, stat, group=None):
    """in-run result gather of one step: two RCCL (gloo in the CPU tests / when the RCCL probe failed) all_gathers of fixed-stride rows
    (unicorn_amd/parallel.py)"""
    from unicorn_amd.parallel import gather_result_rows

    def gather(streams):
        import torch
        rows = torch.cat([r_ for s_ in streams for r_ in s_.pending_rows] or [streams[0].last_rows[:0]], 0).clone()
        for s_ in streams:
            s_.pending_rows = []
        rows[:, 0] = rank
        table = gather_result_rows(rows, group=group)
        own = int(((table[:, 0] == rank).sum()).item()) if table.shape[0] else 0
        stat["lost_rows"] = stat.get("lost_rows", 0) + abs(own - int(rows.shape[0]))      # reported, not raised: a raise on one rank would hang the others
        stat["calls"] += 1
        stat["rows"] += int(table.shape[0])
        return int(table.shape[0])
    return gather


class GpuSensor:
    """Shader clock (hwmon freq1_input) and board power (power1_input) of THIS process's GPU, sampled from sysfs by a background thread
    while a timed region runs: the f16x2 GEMMs are power-limited on random operands, so the roofline block also
    reports the achieved rate against the MFMA peak at the clock the chip actually sustained.  Every sample carries its time stamp:
    `summary(window=(t0, t1))` keeps only the samples BETWEEN THE TWO BARRIERS of the timed steps (warm-up and ramp excluded) and
    reports median / p10 / p90 -- a mean over warm-up + ramp cannot tell a power-limited run from a clock that never left the ramp
    (VERDICT r04 #3)."""

    def __init__(self, dev_index, period=0.005):
        import glob
        import threading
        self.paths, self.samples, self.period = None, [], period
        self._stop, self._th = threading.Event(), None
        try:
            import torch
            pr = torch.cuda.get_device_properties(dev_index)
            want = "%04x:%02x:%02x.0" % (getattr(pr, "pci_domain_id", 0), pr.pci_bus_id, pr.pci_device_id)
            for d in glob.glob("/sys/class/drm/card*/device"):
                if os.path.basename(os.path.realpath(d)) != want:
                    continue
                for h in glob.glob(d + "/hwmon/hwmon*"):
                    if os.path.exists(h + "/freq1_input") and os.path.exists(h + "/power1_input"):
                        self.paths = (h + "/freq1_input", h + "/power1_input", h + "/power1_cap")
        except Exception:                           # noqa: BLE001 -- no sensor, no block
            self.paths = None

    def __enter__(self):
        import threading
        self.samples = []
        self._stop.clear()
        if self.paths:
            def loop():
                while not self._stop.is_set():
                    try:
                        self.samples.append((int(open(self.paths[0]).read()) / 1e6, int(open(self.paths[1]).read()) / 1e6, time.perf_counter()))
                    except Exception:               # noqa: BLE001
                        pass
                    time.sleep(self.period)
            self._th = threading.Thread(target=loop, daemon=True)
            self._th.start()
        return self

    def __exit__(self, *a):
        self._stop.set()
        if self._th is not None:
            self._th.join()

    def summary(self, window=None):
        sm = [x for x in self.samples if window is None or (window[0] <= x[2] <= window[1])]
        if not sm:
            return None
        f = sorted(x[0] for x in sm)
        w = sorted(x[1] for x in sm)
        cap = None
        try:
            cap = int(open(self.paths[2]).read()) / 1e6
        except Exception:                           # noqa: BLE001
            pass

        def q(v, p):
            return v[min(len(v) - 1, int(p * (len(v) - 1) + 0.5))]
        return {"sclk_mhz_median": q(f, 0.5), "sclk_mhz_p10": q(f, 0.1), "sclk_mhz_p90": q(f, 0.9), "sclk_mhz_mean": round(sum(f) / len(f), 1),
                "sclk_mhz_min": f[0], "sclk_mhz_max": f[-1],
                "power_w_median": q(w, 0.5), "power_w_p10": q(w, 0.1), "power_w_p90": q(w, 0.9), "power_w_mean": round(sum(w) / len(w), 1),
                "power_w_max": w[-1], "power_cap_w": cap,
                "frac_samples_within_3pct_of_power_cap": round(sum(1 for x in w if x >= 0.97 * cap) / len(w), 4) if cap else None,
                "samples": len(f), "window": "between the two barriers of the timed steps" if window is not None else "whole sensor context",
                "source": "sysfs hwmon freq1_input / power1_input of this GPU, %.0f ms period" % (1e3 * self.period)}


def box_iou_pairs(a, b):
    import torch
    ax1, ay1, ax2, ay2 = a[:, 0] - a[:, 2] / 2, a[:, 1] - a[:, 3] / 2, a[:, 0] + a[:, 2] / 2, a[:, 1] + a[:, 3] / 2
    bx1, by1, bx2, by2 = b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2
    iw = (torch.min(ax2, bx2) - torch.max(ax1, bx1)).clamp(min=0)
    ih = (torch.min(ay2, by2) - torch.max(ay1, by1)).clamp(min=0)
    inter = iw * ih
    return inter / (a[:, 2] * a[:, 3] + b[:, 2] * b[:, 3] - inter)


def golden_sample(t, max_full=1 << 15):
    """the fixed strided sample tests/golden/make_golden.py stores for large tensors (NCHW order)"""
    import numpy as np
    a = t.detach().float().cpu().contiguous().numpy().reshape(-1)
    return a if a.size <= max_full else a[np.linspace(0, a.size - 1, max_full).astype(np.int64)]


def dump_outputs(out_dir, outputs, budget_bytes=60 << 20):
    """--dump-outputs: every tensor in `outputs` (nested dicts / tuples / lists; None skipped) -> out_dir/<name>.npy, float32 (float64
    stays float64, integer and bool tensors become float64).  Smallest tensor first, each gets an even share of the budget still left
    (60 MiB in all: the files stay under 64 MB); a tensor larger than its share is stored as a sample at sorted indices drawn from a
    generator seeded with 0 (the same positions for the same shapes in every run and every build), named <name>_sample.npy.
    -> {file name: stored shape}"""
    import numpy as np
    import torch

    def walk(name, v):
        if torch.is_tensor(v):
            yield name, v
        elif isinstance(v, (dict, tuple, list)):
            for k, x in (v.items() if isinstance(v, dict) else enumerate(v)):
                yield from walk("%s_%s" % (name, k) if name else str(k), x)
    arrs = sorted(walk("", outputs), key=lambda a: a[1].numel())
    os.makedirs(out_dir, exist_ok=True)
    left, written = budget_bytes, {}
    for k, (name, t) in enumerate(arrs):
        dt = torch.float64 if (t.dtype == torch.float64 or not t.is_floating_point()) else torch.float32
        share = left // (len(arrs) - k) // (8 if dt == torch.float64 else 4)
        flat = t.detach().reshape(-1)
        if flat.numel() > share:
            idx = np.sort(np.random.default_rng(0).integers(0, flat.numel(), share))
            flat, name = flat[torch.from_numpy(idx).to(flat.device)], name + "_sample"
        a = flat.to(dt).cpu().numpy().reshape(t.shape if flat.numel() == t.numel() else (-1,))
        np.save(os.path.join(out_dir, name + ".npy"), a)
        left -= a.nbytes
        written[name + ".npy"] = list(a.shape)
    return written


class Stream:
    """One video stream on one GPU: model + resident frames + the per-step closure of a task."""

    def __init__(self, model_name, precision, task, H, W, NB, dev, seed, corr_prec, P=None, n_frames=4):
        import torch
        import synth
        import unicorn_oracle as uo
        from unicorn_amd.models import Unicorn
        from unicorn_amd.ops import label_map_s8
        self.torch, self.task, self.NB, self.dev, self.corr_prec = torch, task, NB, dev, corr_prec
        self.cfg = uo.CONFIGS[model_name]
        self.P = P if P is not None else synth.synth_state_dict(self.cfg)
        self.model = Unicorn(model_name, precision=precision).cuda(dev.index)
        self.model.load_state_dict(self.P)
        # a time batch holds NB DISTINCT consecutive frames of the stream (rounds 1-5 cycled 4 frames through a 16-frame batch: harmless for
        # dense kernels, but not what "16 consecutive frames" says); the n_frames batches are rotations of the same pool
        pool = max(n_frames, NB)
        fr, self.box = synth.synth_clip(H, W, pool + 1, seed=seed)
        self.frames = [f.to(dev) for f in fr]
        self.H, self.W = H, W
        self.distinct_frames_per_batch = min(NB, pool)
        self.batches = [torch.cat([self.frames[1 + (k + t) % pool] for t in range(NB)], 0) for k in range(n_frames)]
        with torch.no_grad():
            _, self.d_pre = self.model(imgs=self.frames[0], mode="backbone")              # reference frame: once, untimed
        self.lbs = label_map_s8(self.box, H, W, dev)
        self.results = torch.zeros((4096, 8), device=dev)
        self.last_rows = torch.zeros((0, 8), device=dev)
        self.pending_rows = []          # result rows of the steps since the last gather
        self.keep_outputs = False       # --dump-outputs: step() keeps references to what it returned (no copy, no sync)
        self.last_out = None
        self.seed = seed
        self._gen = None
        if task == "mot":     # evaluate_omni loop (mot_evaluator.py:991-1045) with the native QuasiDense association
            from unicorn_amd.tracker import OmniMOTFrame, QuasiDenseEmbedTracker
            # synthetic weights give obj * cls ~ 1e-4: the score thresholds are set from the score distribution of one frame so that
            # ~200 candidates reach the NMS and the association (documented in DESIGN.md); tracker thresholds follow
            with torch.no_grad():
                o, _ = self.model(self.frames[1])
                o = o[0] if self.cfg.mask else o
                sc = (o[0, :, 4] * o[0, :, 5:].max(1)[0]).sort(descending=True)[0]
            self.score_thr = float((sc[199] + sc[200]) / 2)
            # QuasiDense thresholds at the same relative places of the score distribution as the defaults (0.8 / 0.5) have on a trained
            # detector: ~30 detections may start a track, ~100 take part in the association (the rest are backdrops)
            kw = dict(init_score_thr=float(sc[30]), obj_score_thr=float(sc[100]), match_score_thr=0.5, memo_tracklet_frames=10,
                      memo_backdrop_frames=1, memo_momentum=0.8, nms_conf_thr=float(sc[100]), nms_backdrop_iou_thr=0.3,
                      nms_class_iou_thr=0.7, with_cats=True, match_metric="bisoftmax")
            self.omni = OmniMOTFrame(self.model, QuasiDenseEmbedTracker(**kw), (H, W), num_classes=self.cfg.num_classes,
                                     confthre=self.score_thr, nmsthre=0.7, embed_score_thr=self.score_thr)
        if task == "vos":
            from unicorn_amd.tracker import UnicornVOSTrack
            self.trk = UnicornVOSTrack(self.model, input_size=(H, W), d_rate=self.cfg.d_rate)
            b = self.box
            boxes = {"1": b, "2": torch.tensor([W * 0.55, H * 0.1, W * 0.9, H * 0.45]), "3": torch.tensor([W * 0.1, H * 0.55, W * 0.4, H * 0.95])}
            self.vos_boxes = boxes
            self.trk.initialize(self.frames[0], {"init_object_ids": list(boxes), "init_bbox": {
                k: [float(v[0]), float(v[1]), float(v[2] - v[0]), float(v[3] - v[1])] for k, v in boxes.items()}})
        torch.cuda.synchronize()

    def frames_per_step(self):
        return 1 if self.task == "vos" else self.NB

    def sot_batch(self, img):
        """unicorn_sot.py:78-108 for a batch of current frames against the cached reference frame"""
        from unicorn_amd.ops import corr_softmax_pv, corr_softmax_pv_batched, prior_pyramid
        torch, m = self.torch, self.model
        B = img.shape[0]
        fpn, d_cur = m(imgs=img, mode="backbone")
        f_pre, f_cur = m(seq_dict0=self.d_pre, seq_dict1=d_cur, mode="interaction")
        e_pre = m(feat=f_pre, mode="upsample")
        e_cur = m(feat=f_cur, mode="upsample")
        if B > 1 and not os.environ.get("UNI_BENCH_CORR_PER_FRAME"):      # one launch for the frames of the step (A/B switch: per-frame launches)
            pred = corr_softmax_pv_batched(e_pre, e_cur, self.lbs, precision=self.corr_prec)
        else:
            pred = torch.cat([corr_softmax_pv(e_pre[b].flatten(-2), e_cur[b].flatten(-2), self.lbs, precision=self.corr_prec) for b in range(B)], 0)
        coarse = pred.view(1, B, d_cur["h"] * 2, d_cur["w"] * 2)
        pri = tuple(t.transpose(0, 1).contiguous() for t in prior_pyramid(coarse))
        out = m.head(fpn, pri, mode="sot")
        return dict(fpn=fpn, e_pre=e_pre, e_cur=e_cur, coarse=coarse, head=out)

    def step(self, i):
        torch, m = self.torch, self.model
        with torch.no_grad():
            if self.task == "sot":
                r = self.sot_batch(self.batches[i % len(self.batches)])
                out = r["head"][0] if self.cfg.mask else r["head"]
                best = torch.argmax(out[:, :, 4] * out[:, :, 5], 1)       # result rows (top-1 per frame stays on the device, no sync)
                B = out.shape[0]
                rows = torch.zeros((B, 8), device=self.dev)
                rows[:, 1] = i * B + torch.arange(B, device=self.dev)
                rows[:, 3:7] = out[torch.arange(B, device=self.dev), best, :4]
                rows[:, 7] = out[torch.arange(B, device=self.dev), best, 4]
                self.last_rows = rows
                self.pending_rows = (self.pending_rows + [rows])[-64:]
                self.results[i % 4096] = rows[0]
                if self.keep_outputs:
                    self.last_out = dict(r, rows=rows)
            elif self.task == "mot":      # the evaluate_omni loop body over NB consecutive frames (unicorn_amd/tracker/omni.py)
                img = self.batches[i % len(self.batches)]
                if os.environ.get("UNI_BENCH_NO_PIPELINE"):
                    res = self.omni.run_batch(img, (self.H, self.W))
                else:      # software-pipelined over the launch stream (OmniMOTFrame.run_stream): step i collects batch i while the GPU runs
                    if self._gen is None:          # `whole` of the batches admitted ahead; every step still enqueues one A and one B stage
                        import itertools
                        self._gen = self.omni.run_stream((self.batches[k % len(self.batches)] for k in itertools.count(i)), (self.H, self.W))
                    res = next(self._gen)
                rows = []
                for bi, (bb, ids) in enumerate(res):
                    if bb is not None:
                        for k in range(bb.shape[0]):
                            rows.append([0.0, float(i * img.shape[0] + bi), float(ids[k])] + [float(v) for v in bb[k, :5]])
                self.last_rows = torch.tensor(rows, dtype=torch.float32).reshape(-1, 8).to(self.dev)
                self.pending_rows = (self.pending_rows + [self.last_rows])[-64:]
                if self.keep_outputs:
                    self.last_out = {"rows": self.last_rows}
            else:                         # VOS: K = 3 objects, head per object, CondInst masks + postprocess (unicorn_vos.py:71-200)
                res, _ = self.trk.step(self.frames[1 + i % (len(self.frames) - 1)])
                if self.keep_outputs:
                    self.last_out = {"obj": res}
                d = res["1"][0]
                if d is not None:
                    self.results[i % 4096, :7] = d
                    self.last_rows = self.results[i % 4096:i % 4096 + 1].clone()
                    self.pending_rows = (self.pending_rows + [self.last_rows])[-64:]


def timed(streams, steps, warmup, barrier, gather=None, gather_every=1, errs=None, window=None):
    """W warm-up steps, barrier + sync, exactly K timed steps, barrier + sync.  `gather` (N > 1): the in-run RCCL gather of the
    result rows every `gather_every` steps (external/lib/test/evaluation/running.py collects per sequence; here per step).
    `errs` (N > 1): a list; an exception in this rank's step is appended there and the rank keeps calling the collectives (with the
    rows it has) so that the other ranks never hang on it.
    `window`: a list that receives [t0, t1], the perf_counter stamps of the two barriers (GpuSensor.summary keeps the samples between).
    Returns (wall seconds between the barriers, this rank's own busy seconds, gathered row count)."""
    import torch
    sync = torch.cuda.synchronize if torch.cuda.is_available() else (lambda: None)      # (the CPU tests drive this loop with fake streams)

    def do(i):
        if errs:                                   # this rank already failed: collectives only
            return
        try:
            for s in streams:
                s.step(i)
        except Exception as e:                     # noqa: BLE001
            if errs is None:
                raise
            errs.append("step %d: %r" % (i, e))

    for i in range(warmup):
        do(i)
        if gather is not None and (i + 1) % gather_every == 0:
            gather(streams)
    barrier()
    t0 = time.perf_counter()
    nrows, own, ta = 0, 0.0, t0
    for i in range(steps):
        do(warmup + i)
        if gather is not None and (i + 1) % gather_every == 0:
            sync()               # this rank's own work up to here (the collective below waits for the slowest rank)
            own += time.perf_counter() - ta
            nrows += gather(streams)
            ta = time.perf_counter()
    sync()
    own += time.perf_counter() - ta
    barrier()
    t1 = time.perf_counter()
    if window is not None:
        window[:] = [t0, t1]
    return t1 - t0, own, nrows


def main():
    args = parse()
    if args.rccl_probe:
        rccl_probe_child()
    if args.torch_rocm_port_child:
        torch_rocm_port_child(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))
    import torch
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == args.gpus, "launched with WORLD_SIZE=%d but --gpus %d" % (world, args.gpus)
    dist, dgroup, dinfo = None, None, None
    if torch.cuda.is_available():
        # the rank's GPU must be current BEFORE any RCCL communicator is created (a communicator binds to the current device: with the
        # default device every rank would sit on GPU 0 and RCCL reports "Duplicate GPU detected")
        if os.environ.get("UNI_BENCH_SHARE_GPU"):      # plumbing test of the N > 1 path on a one-GPU box: all ranks on GPU 0
            local_rank = local_rank % torch.cuda.device_count()
        torch.cuda.set_device(local_rank)
    if world > 1:          # N = 1 (also under torchrun) never touches torch.distributed: same code path as the plain run
        dist, dgroup, dinfo = init_dist(rank, local_rank, world, torch.cuda.is_available())
        assert dist.get_world_size() == args.gpus
    if args.launch_check:
        ldev = "cuda:%d" % local_rank if (torch.cuda.is_available() and dinfo and dinfo["data"] == "nccl") else "cpu"
        n = torch.ones(1, device=ldev)
        tasks, grows, nstr = [rank_task(args.task, args.model, 0, 1)[0]], 0, 0
        if dist is not None:
            dist.all_reduce(n, group=dgroup)
            # the multi-rank plumbing of the timed run with synthetic rows: task per rank, ragged row gather, byte-string gather
            from unicorn_amd.parallel import gather_byte_strings
            t_, _ = rank_task(args.task, args.model, rank, world)
            code = torch.tensor([1.0 if t_ == "mot" else 0.0], device=ldev)
            codes = [torch.zeros_like(code) for _ in range(world)]
            dist.all_gather(codes, code, group=dgroup)
            tasks = [("mot" if float(c_) > 0.5 else ("sot" if args.task == "mix" else args.task)) for c_ in codes]

            class _S:
                last_rows = torch.zeros((3 + rank, 8), device=ldev)          # ragged: MOT ranks return a varying number of rows
                pending_rows = [last_rows]
            st_ = {"calls": 0, "rows": 0}
            grows = make_gather(rank, st_, dgroup)([_S])
            strs = gather_byte_strings([bytes([48 + rank]) * (5 + rank)] * (1 + rank % 2), group=dgroup)
            nstr = sum(len(x) for x in strs)
            assert strs[rank] == [bytes([48 + rank]) * (5 + rank)] * (1 + rank % 2)
        if rank == 0:
            print(json.dumps({"launch_check": True, "n_gpus": int(n.item()), "backend": "none" if dist is None else dinfo["data"],
                              "dist": dinfo, "tasks": tasks, "gathered_rows": grows, "gathered_strings": nstr}))
        if dist is not None:
            dist.destroy_process_group()
        return
    assert torch.cuda.is_available(), "bench.py needs an MI355X (no CPU fallback for the measured path)"
    dev = torch.device("cuda", local_rank)

    import synth
    import unicorn_oracle as uo
    from unicorn_amd import _lib as L

    H, W, NB = args.height, args.width, max(1, args.batch)

    def barrier():
        if dist is not None:
            dist.barrier()                          # gloo control group (timeout 900 s: a dead rank raises instead of hanging forever)
        torch.cuda.synchronize()

    # BASELINE.json configs[4]: "8 independent 800x1280 streams (MOT+SOT mix), one stream per GPU, RCCL gather": the first half of the
    # ranks run the MOT loop (evaluate_omni on the MOT17-style model, num_classes = 1), the second half the SOT step
    task, model_name = rank_task(args.task, args.model, rank, world)
    errs = [] if dist is not None else None        # N > 1: a failing rank reports instead of hanging the others; N = 1: exceptions propagate
    main_s = None
    try:
        main_s = Stream(model_name, args.precision, task, H, W, NB, dev, seed=1 + rank, corr_prec=args.corr_precision)
    except Exception as e:                          # noqa: BLE001
        if errs is None:
            raise
        errs.append("setup: %r" % (e,))
    gather, gstat = None, {"calls": 0, "rows": 0}
    if dist is not None:
        from unicorn_amd.parallel import gather_byte_strings
        gather_rows = make_gather(rank, gstat, dgroup)

        class _Empty:                               # what a failed rank contributes to the gathers
            last_rows = torch.zeros((0, 8), device=dev)
            pending_rows = []

        def gather(streams):
            return gather_rows(streams if not errs else [_Empty])
    if main_s is not None and args.dump_outputs and rank == 0:
        main_s.keep_outputs = True
    sensor, win = (GpuSensor(local_rank) if args.full else None), []
    with sensor if sensor is not None else contextlib.nullcontext():
        dt, own_dt, _ = timed([main_s] if main_s is not None else [], args.steps, args.warmup, barrier, gather, max(1, args.gather_every), errs,
                              window=win)
    clocks = sensor.summary(window=win or None) if sensor is not None else None
    if main_s is not None and main_s.last_out is not None and not errs:      # before any other leg steps the stream again
        written = dump_outputs(args.dump_outputs, main_s.last_out)
        main_s.keep_outputs, main_s.last_out = False, None
        print("[bench] outputs of the last timed step -> %s: %s" % (args.dump_outputs, written), file=sys.stderr, flush=True)
    fps_frames = args.steps * main_s.frames_per_step() if (main_s is not None and not errs) else 0
    per_rank, rank_errors = None, None
    if dist is not None:
        t = torch.tensor([dt, float(fps_frames)], dtype=torch.float64)
        tmax = t.clone()
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)                      # control group (gloo, CPU tensors)
        dist.all_reduce(t, op=dist.ReduceOp.SUM)
        dt, total_frames = float(tmax[0]), float(t[1])
        # per-rank rate (own busy time between the barriers) and the task each rank ran
        mine = torch.tensor([fps_frames / own_dt if own_dt > 0 else 0.0, 1.0 if task == "mot" else 0.0], dtype=torch.float64)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        per_rank = [{"rank": r_, "task": "mot" if float(v[1]) > 0.5 else ("sot" if args.task in ("mix", "sot") else args.task), "fps": round(float(v[0]), 2)}
                    for r_, v in enumerate(allr)]
        # every rank's own clock / power between the barriers and its busy seconds (eight GPUs at ~1.3 kW each may meet a NODE power
        # budget: a scaling curve has to be explainable from its own line); control group, a few numbers per rank
        mine_hw = {"busy_s": round(own_dt, 4)}        # this rank's own work between the barriers (the line's ms_per_step is the MAX over ranks)
        if clocks:
            mine_hw.update({k_: clocks[k_] for k_ in ("sclk_mhz_median", "sclk_mhz_p10", "power_w_median", "power_w_p90", "power_cap_w",
                                                      "frac_samples_within_3pct_of_power_cap")})
        all_hw = [None] * world
        dist.all_gather_object(all_hw, mine_hw)
        for r_, hw_ in enumerate(all_hw):
            per_rank[r_].update(hw_ or {})
        all_errs = [None] * world
        dist.all_gather_object(all_errs, list(errs))                    # a few short strings, control group
        rank_errors = {str(r_): e_ for r_, e_ in enumerate(all_errs) if e_} or None
        if args.full:
            # variable-length gather (mask RLE strings, unicorn_amd/parallel.py:gather_byte_strings): every rank encodes the box of its last
            # result row as a mask with the device RLE kernel; rank 0 decodes every string and checks the round trip
            hm, wm = 135, 240
            strs, mk = [], None
            try:
                if errs:
                    raise RuntimeError("rank failed earlier")
                from unicorn_amd.ops import rle_encode
                rr = main_s.last_rows[:4] if main_s.last_rows.shape[0] else torch.zeros((1, 8), device=dev)
                mk = torch.zeros((rr.shape[0], hm, wm), device=dev, dtype=torch.uint8)
                bx = (rr[:, 3:7] / 8.0).clamp(min=0).long().cpu().tolist()
                for k_, (x1, y1, x2, y2) in enumerate(bx):
                    mk[k_, min(y1, hm - 1):min(max(y2, y1 + 1), hm), min(x1, wm - 1):min(max(x2, x1 + 1), wm)] = 1
                strs = rle_encode(mk)
            except Exception as e:                      # noqa: BLE001
                if not errs:
                    errs.append("rle: %r" % (e,))
            allstr = gather_byte_strings(strs, group=dgroup)
            gstat["rle_own_ok"] = bool(len(allstr) == world and allstr[rank] == strs)
            if rank == 0:
                from unicorn_amd.utils.masks import rle_string_to_mask
                nstr, nbad = 0, 0
                for r_ in range(world):
                    for b_ in allstr[r_]:
                        try:
                            rle_string_to_mask(b_, hm, wm)      # raises unless the runs cover the hm x wm mask exactly
                        except ValueError:
                            nbad += 1
                        nstr += 1
                gstat["rle_strings"], gstat["rle_undecodable"] = nstr, nbad
                if strs and mk is not None:
                    gstat["rle_round_trip_ok"] = bool((torch.as_tensor(rle_string_to_mask(strs[0], hm, wm)) == mk[0].cpu()).all())
        gstat["dist"] = dinfo
    else:
        total_frames = float(fps_frames)
    fps = total_frames / dt
    if main_s is None or errs:                       # this rank has nothing more to measure; rank 0 still prints what the others did
        if rank == 0:
            print(json.dumps({"metric": "frames/sec @ %dx%d %s" % (H, W, args.model), "value": round(fps, 3), "unit": "frames/s", "n_gpus": world,
                              "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / max(args.steps, 1), 4),
                              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "data": "synthetic",
                              "config": {"workload": "rank 0 failed; value counts the frames of the surviving ranks", "rank_tasks": per_rank, "gather": gstat},
                              "rank_errors": rank_errors}))
        if dist is not None:
            dist.destroy_process_group()
        return

    # ---------------- roofline leg: per-kernel-class HIP-event timing on the launch stream (rank 0) ----------------
    roof, extra = None, {}
    if rank == 0 and args.full:
        import ctypes as C
        model = main_s.model
        prof_steps = 3
        buf = (C.c_double * 16)()
        L.check(L.lib().uni_prof_begin(model._ctx), "prof_begin")
        for i in range(prof_steps):
            main_s.step(i)
        L.check(L.lib().uni_prof_end(model._ctx, buf), "prof_end")
        v = list(buf)
        names = ["gemm", "dwconv7_ln", "gn_apply", "layernorm", "misc"]
        pf = prof_steps * main_s.frames_per_step()
        cls = {n: dict(ms=v[3 * i] / pf, work=v[3 * i + 1] / pf, launches=v[3 * i + 2] / prof_steps) for i, n in enumerate(names)}
        g = cls["gemm"]
        g["bytes"] = v[15] / prof_steps
        nf = main_s.frames_per_step()
        # dense 16-bit MFMA peak 2500 TFLOP/s (MI355X_MICROARCH.md).  The f16x2 format issues 3 f16 MFMAs per fp32-equivalent product,
        # so the MFMA roofline of this dtype is 2500 / 3 (same convention as the 2500 / 6 of the bf16x3 correlation); exact fp32: 157.3
        mfma_per_product = {"bf16": 1, "f16x2": 3, "fp32": 1}[args.precision]
        peak = {"bf16": 2500.0, "f16x2": round(2500.0 / 3, 1), "fp32": 157.3}[args.precision]
        ach = g["work"] / (g["ms"] * 1e-3) / 1e12 if g["ms"] > 0 else 0.0
        traffic, tsrc = None, None
        try:    # HBM-side bytes per launch from separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (tools/pmc_traffic.py)
            want = "_%s_pmc_hbm_traffic.json" % args.precision
            tsrc = sorted(f for f in os.listdir(os.path.join(ROOT, "profiles")) if f.endswith(want))[-1]
            tj = json.load(open(os.path.join(ROOT, "profiles", tsrc)))
            t = tj.get("gemm_h2_kernel" if args.precision == "f16x2" else "gemm_bf16_kernel") or tj["gemm"]
            traffic = round(t["fetch_bytes_per_launch"] + t["write_bytes_per_launch"])
        except Exception:
            tsrc = None
        pmc_live = None
        if world == 1 and not args.no_pmc and not args.no_extras:      # measured by this run (the replayed value stays as `traffic_replayed`)
            torch.cuda.synchronize()
            live, pmc_live = measure_pmc_traffic(args, H, W)
            if live is not None:
                pmc_live["replayed_from_profiles"] = {"bytes_per_launch": traffic, "source": tsrc}
                traffic, tsrc = live, "this run"
        kname = {"bf16": "gemm_bf16_kernel / gemm_bf16_p44_kernel", "f16x2": "gemm_h2q_kernel / gemm_h2_kernel", "fp32": "gemm_f32_kernel"}[args.precision]
        roof = {"kernel": kname + " (all instantiations)", "bound": "mfma", "achieved": round(ach, 2), "peak": peak,
                "unit": "TFLOP/s", "frac": round(ach / peak, 4),
                # the same achieved rate against the other two peaks SURVEY.md 8(d) names: the raw dense 16-bit MFMA peak (what a 1-MFMA
                # bf16 product would be priced at) and the exact-fp32 MFMA peak (what the fp32 reference arithmetic would cost on MFMA)
                "frac_vs_f16_peak": round(ach / 2500.0, 4), "frac_vs_fp32_mfma": round(ach / 157.3, 3),
                # sustained shader clock / board power during the timed loop (sysfs) and the same rate against the MFMA peak AT THAT CLOCK
                "clocks": clocks,
                "frac_vs_peak_at_sustained_clock": round(ach / (peak * clocks["sclk_mhz_median"] / 2400.0), 4) if clocks else None,
                "traffic": traffic, "traffic_source": tsrc, "traffic_measured_in_run": tsrc == "this run", "traffic_detail": pmc_live,
                "traffic_note": ("HBM-side bytes per launch of the GEMM class from two separate rocprofv3 --pmc passes spawned by this run" if tsrc == "this run" else
                                 "HBM bytes per launch replayed from the committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (profiles/), not collected in this run"),
                "peak_note": "dense 16-bit MFMA 2500 TFLOP/s / %d MFMAs per fp32-equivalent product" % mfma_per_product if mfma_per_product > 1 else "dense MFMA peak of the dtype",
                "mfma_per_product": mfma_per_product, "mfma_issue_TFLOPs": round(ach * mfma_per_product, 1),
                "algorithmic_bytes_per_launch": round(g["bytes"] / max(g["launches"], 1)),
                "avg_launch_us": round(1e3 * g["ms"] * nf / max(g["launches"], 1), 2), "launches_per_step": g["launches"],
                "flops_per_frame": g["work"], "flops_per_launch": round(g["work"] * nf / max(g["launches"], 1))}
        for n in ("dwconv7_ln", "gn_apply", "layernorm"):
            c_ = cls[n]
            extra[n] = {"ms_per_frame": round(c_["ms"], 4), "GBps": round(c_["work"] / (c_["ms"] * 1e-3) / 1e9, 1) if c_["ms"] > 0 else 0,
                        "launches": c_["launches"]}
        # HBM-bound kernel classes against the 8.0 TB/s HBM3E peak (algorithmic bytes = input + output once)
        extra["hbm"] = {n: {"bound": "hbm", "achieved": extra[n]["GBps"], "peak": 8000.0, "unit": "GB/s", "frac": round(extra[n]["GBps"] / 8000.0, 4),
                            "share_of_frame": round(cls[n]["ms"] / max(sum(c_["ms"] for c_ in cls.values()), 1e-9), 4)}
                        for n in ("dwconv7_ln", "gn_apply", "layernorm")}
        extra["gemm_share_of_frame"] = round(g["ms"] / max(sum(c_["ms"] for c_ in cls.values()), 1e-9), 4)
        extra["gemm_ms_per_frame"] = round(g["ms"], 4)
        extra["misc_ms_per_frame"] = round(cls["misc"]["ms"], 4)
        if task == "sot":   # correlation kernel alone (torch events on the current stream == launch stream)
            from unicorn_amd.ops import corr_softmax_pv
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            with torch.no_grad():
                r = main_s.sot_batch(main_s.frames[1])
                a, b = r["e_pre"][0].flatten(-2), r["e_cur"][0].flatten(-2)
                corr_softmax_pv(a, b, main_s.lbs, precision=args.corr_precision)
                ev[0].record()
                for _ in range(5):
                    corr_softmax_pv(a, b, main_s.lbs, precision=args.corr_precision)
                ev[1].record()
                torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / 5
            n = a.shape[1]
            # precision 1 / 2 issue 6 / 3 MFMA terms per fp32-equivalent product: effective peak = 2500 / 6 or 2500 / 3 TFLOP/s
            extra["corr_fp32"] = {"ms": round(ms, 4), "TFLOPs": round(2.0 * n * n * 128 / (ms * 1e-3) / 1e12, 2),
                                  "peak_effective": [157.3, round(2500.0 / 6, 1), round(2500.0 / 3, 1), 2500.0][args.corr_precision],
                                  "mode": ["fp32 MFMA", "bf16x3 split (6 exact partial products, fp32 accumulate)",
                                           "f16x2 split (3 partial products, fp32 accumulate)",
                                           "fp16 single pass (the reference driver's arithmetic class, not a parity mode)"][args.corr_precision]}

    # ---------------- single-frame leg: ONE (1,3,H,W) frame per call, host-synchronised per frame = the reference drivers' call pattern
    # (external/lib/test/tracker/unicorn_sot.py:57-76), with its own roofline block ----------------
    single = None
    if rank == 0 and args.full and task == "sot" and not args.no_single_frame:
        import ctypes as C
        with torch.no_grad():
            for _ in range(3):
                main_s.sot_batch(main_s.frames[1])
            torch.cuda.synchronize()
            lats = []
            sens1 = GpuSensor(local_rank)
            with sens1:
                for i in range(20):
                    t1 = time.perf_counter()
                    main_s.sot_batch(main_s.frames[1 + i % 4])
                    torch.cuda.synchronize()
                    lats.append(time.perf_counter() - t1)
            buf1 = (C.c_double * 16)()
            L.check(L.lib().uni_prof_begin(main_s.model._ctx), "prof_begin")
            for i in range(3):
                main_s.sot_batch(main_s.frames[1 + i % 4])
            L.check(L.lib().uni_prof_end(main_s.model._ctx, buf1), "prof_end")
        lats.sort()
        lat = sum(lats) / len(lats)
        v1 = list(buf1)
        g_ms, g_work, g_n = v1[0] / 3, v1[1] / 3, v1[2] / 3
        ach1 = g_work / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
        peak1 = {"bf16": 2500.0, "f16x2": round(2500.0 / 3, 1), "fp32": 157.3}[args.precision]
        hb1 = {}
        for i_, n_ in ((1, "dwconv7_ln"), (2, "gn_apply"), (3, "layernorm")):
            ms_1 = v1[3 * i_] / 3
            hb1[n_] = {"ms_per_frame": round(ms_1, 4), "GBps": round(v1[3 * i_ + 1] / 3 / (ms_1 * 1e-3) / 1e9, 1) if ms_1 > 0 else 0,
                       "frac": round(v1[3 * i_ + 1] / 3 / (ms_1 * 1e-3) / 8e12, 4) if ms_1 > 0 else 0, "launches": v1[3 * i_ + 2] / 3}
        single = {"ms": round(1e3 * lat, 3), "ms_min": round(1e3 * lats[0], 3), "ms_median": round(1e3 * lats[len(lats) // 2], 3),
                  "fps": round(1.0 / lat, 2), "frames_per_step": 1, "precision": args.precision,
                  "note": "one (1,3,%d,%d) frame per call, host-synchronised per frame (mean of 20)" % (H, W),
                  "roofline": {"kernel": "GEMM class at one frame per call (gemm_h2d_kernel deep-pipeline tiles, gemm_h2q_kernel, mlp_fused16_kernel)",
                               "bound": "mfma", "achieved": round(ach1, 2), "peak": peak1, "unit": "TFLOP/s", "frac": round(ach1 / peak1, 4),
                               "frac_vs_f16_peak": round(ach1 / 2500.0, 4), "gemm_ms_per_frame": round(g_ms, 4), "launches": g_n,
                               "avg_launch_us": round(1e3 * g_ms / max(g_n, 1), 2),
                               "note": "kernel time by HIP events with the head levels serialised (profiling mode); whole-call fp32-equivalent rate = "
                                       "%.1f TFLOP/s" % (g_work / lat / 1e12)},
                  "hbm": hb1, "misc_ms_per_frame": round(v1[12] / 3, 4), "clocks": sens1.summary()}

    # ---------------- CPU baseline (the oracle = port of the reference, host cores, bounded sample) + in-run parity ----------------
    cpu, parity = None, None
    if rank == 0 and args.full and not args.no_cpu_baseline:
        cores = min(os.cpu_count() or 1, 16)
        torch.set_num_threads(cores)
        P, cfg = main_s.P, main_s.cfg
        ncpu = max(1, min(args.cpu_frames, len(main_s.frames) - 1)) if world == 1 else 1      # N > 1: one frame (the other ranks wait)
        cf = [f.cpu() for f in main_s.frames[:1 + ncpu]]
        ious, coss, prs, cts = [], [], [], []
        with torch.no_grad():
            st = uo.sot_init(P, cfg, cf[0], main_s.box)
            cdt = 0.0
            for i in range(ncpu):
                t1 = time.perf_counter()
                if task == "mot":
                    o_out, _, _ = uo.mot_whole(P, cfg, cf[1 + i])
                    o = None
                else:
                    o = uo.sot_step(P, cfg, st, cf[1 + i])
                cts.append(time.perf_counter() - t1)
                cdt += cts[-1]
                if task == "sot":     # parity of the TIMED configuration (same model object, same precision, same frames)
                    r = main_s.sot_batch(main_s.frames[1 + i])
                    ho = o["head"][0] if cfg.mask else o["head"]
                    hh = (r["head"][0] if cfg.mask else r["head"]).cpu()
                    score = ho[0, :, 4] * ho[0, :, 5]
                    top = torch.argsort(score, descending=True)[:500]
                    ious.append(box_iou_pairs(hh[0, top, :4], ho[0, top, :4]))
                    ea, eb = r["e_cur"].cpu().flatten(2)[0].double(), o["embed_cur"].flatten(2)[0].double()
                    coss.append((ea * eb).sum(0) / (ea.norm(dim=0) * eb.norm(dim=0)).clamp_min(1e-30))
                    prs.append(float((r["coarse"].cpu().reshape(-1) - o["coarse"].reshape(-1)).abs().max()))
        torch.set_num_threads(1)           # the remaining legs are GPU work: no OpenMP team next to the HIP dispatch thread
        cts_ = sorted(cts)
        cpu = {"value": round(ncpu / cdt, 4), "unit": "frames/s", "cores": cores, "kind": "port",
               "frames": ncpu, "s_per_frame_min": round(cts_[0], 3), "s_per_frame_median": round(cts_[len(cts_) // 2], 3),
               "s_per_frame_max": round(cts_[-1], 3),
               "sample": "%d frames of the same %s %s step at %dx%d, fp32, torch CPU on %d threads (oracle/unicorn_oracle.py = the pinned port; "
                         "the reference tree itself does not exist on the GPU box)" % (ncpu, args.model, task, H, W, cores)}
        if args.torch_rocm_port and world == 1:      # context: the same port on PyTorch-ROCm's own kernels, this GPU (child process, bounded; N = 1 only: the other ranks would wait)
            import subprocess
            torch.cuda.synchronize()
            try:
                cp = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-rocm-port-child", "--model", args.model, "--height", str(H), "--width", str(W),
                                     "--cpu-frames", str(args.cpu_frames)], capture_output=True, text=True, timeout=float(os.environ.get("UNI_BENCH_PORT_TIMEOUT", "300")))
                ln = [l for l in cp.stdout.splitlines() if l.startswith("{")]
                cpu["torch_rocm_port"] = json.loads(ln[-1]) if ln else {"error": (cp.stderr or cp.stdout)[-300:]}
            except subprocess.TimeoutExpired:
                cpu["torch_rocm_port"] = {"error": "timeout"}
            if isinstance(cpu["torch_rocm_port"], dict):
                cpu["torch_rocm_port"]["note"] = ("oracle port executed by PyTorch-ROCm eager kernels on the same MI355X (context for `value`; kind = port: the "
                                                  "reference tree cannot travel to the GPU box)")
        if ious:
            iou = torch.cat(ious)
            parity = {"vs": "CPU oracle (fp32), %d frames of the timed stream, top-500 anchors by oracle score" % ncpu,
                      "precision": args.precision, "box_iou_min": round(float(iou.min()), 6), "box_iou_mean": round(float(iou.mean()), 6),
                      "embed_cos_min": round(float(torch.cat(coss).min()), 8), "prior_max_abs": max(prs), "mask_iou_min": None,
                      "bar": "box/mask IoU >= 0.999, embedding cosine within 1e-4 (BASELINE.json north_star)",
                      "pass": bool(iou.min() >= 0.999 and torch.cat(coss).min() >= 1 - 1e-4),
                      # third-party arithmetic on rows 0 / N1 / N2 that is restated from published sources and has NO real-library fixture
                      # (the libraries are absent offline); everything else is pinned to the real reference
                      "parity_unpinned": ["cv2.resize", "torchvision.nms", "pycocotools.rle", "lap.lapjv", "cython_bbox.bbox_overlaps"]}

    # ---------------- margin log: box IoU min of the timed precision against every REAL-REFERENCE golden (tests/golden/*.npz, the cases
    # of tests/test_model_gpu.py::test_tiny_320_vs_reference_golden), so that a drift towards the 0.999 bar shows in the bench line before
    # a test flips.  Committed fixtures only: nothing here reads the reference tree. ----------------
    if rank == 0 and world == 1 and parity is not None and not args.no_extras and args.precision in ("f16x2", "fp32"):
        import numpy as np
        gold = {}
        gdir = os.path.join(ROOT, "tests", "golden")
        for gname, gh, gw in (("unicorn_track_tiny", 320, 320), ("unicorn_track_large", 320, 320), ("unicorn_track_large_mask", 320, 320),
                              ("unicorn_track_large_mot_challenge", 320, 320), ("unicorn_track_tiny_mask", 320, 512)):
            gp = os.path.join(gdir, "%s_%dx%d.npz" % (gname, gh, gw))
            if not os.path.exists(gp):
                continue
            try:
                g = np.load(gp)
                gs = Stream(gname, args.precision, "sot", gh, gw, 1, dev, seed=1, corr_prec=args.corr_precision,
                            P=main_s.P if gname == args.model else None, n_frames=1)
                with torch.no_grad():
                    r = gs.sot_batch(gs.frames[1])
                hg = torch.from_numpy(g["head_out"]).reshape(tuple(g["head_out__shape"]))[0]
                hh = (r["head"][0] if gs.cfg.mask else r["head"])[0].cpu()
                top = torch.argsort(hg[:, 4] * hg[:, 5], descending=True)[:200]
                iou = box_iou_pairs(hh[top, :4], hg[top, :4])
                gold["%s_%dx%d" % (gname, gh, gw)] = {"box_iou_min_top200": round(float(iou.min()), 6),
                                                      "embed_rel_l2": float("%.3g" % (np.linalg.norm(golden_sample(r["e_cur"]) - g["embed_cur"])
                                                                                      / np.linalg.norm(g["embed_cur"])))}
                del gs
            except Exception as e:                  # noqa: BLE001 -- a margin log must not take the bench line down
                gold["%s_%dx%d" % (gname, gh, gw)] = {"error": repr(e)[:200]}
        # the HEADLINE size itself: vectors of the real reference at 800 x 1280 (tests/golden/make_golden.py:run_headline; the 500 best raw head rows)
        for gname in ("unicorn_track_large", "unicorn_track_large_mask"):
            gp = os.path.join(gdir, "%s_%dx%d.npz" % (gname, 800, 1280))
            if not os.path.exists(gp) or (H, W) != (800, 1280):
                continue
            try:
                g = np.load(gp)
                mf = int(g["__max_full"][0])
                gs = main_s if gname == args.model else Stream(gname, args.precision, "sot", 800, 1280, 1, dev, seed=1, corr_prec=args.corr_precision, n_frames=1)
                with torch.no_grad():
                    r = gs.sot_batch(gs.frames[1])
                hh = (r["head"][0] if gs.cfg.mask else r["head"])[0].cpu()
                top, ref = torch.from_numpy(g["head_top_idx"]), torch.from_numpy(g["head_top_rows"])
                iou = box_iou_pairs(hh[top, :4], ref[:, :4])
                gold["%s_800x1280" % gname] = {"box_iou_min_top200": round(float(iou[:200].min()), 6), "box_iou_min_top500": round(float(iou.min()), 6),
                                               "embed_rel_l2": float("%.3g" % (np.linalg.norm(golden_sample(r["e_cur"], mf) - g["embed_cur"])
                                                                               / np.linalg.norm(g["embed_cur"]))),
                                               "coarse_maxabs": float("%.3g" % np.abs(golden_sample(r["coarse"], mf) - g["coarse"]).max())}
                if gs is not main_s:
                    del gs
            except Exception as e:                  # noqa: BLE001
                gold["%s_800x1280" % gname] = {"error": repr(e)[:200]}
        parity["golden_vs_real_reference"] = gold
        vals = [v["box_iou_min_top200"] for v in gold.values() if "box_iou_min_top200" in v] + \
               [v["box_iou_min_top500"] for v in gold.values() if "box_iou_min_top500" in v]
        parity["golden_box_iou_min"] = min(vals) if vals else None
        parity["margin_to_bar"] = round(min([parity["box_iou_min"]] + vals) - 0.999, 6)
        torch.cuda.empty_cache()

    # ---------------- sub-results: other precision modes, single-frame latency, the other BASELINE configs ----------------
    modes, configs = {}, {}
    if rank == 0 and args.full and world == 1 and not args.no_extras:
        def quick(model_name, precision, task, nb, steps=4, warmup=1, P=None, keep=False):
            s = Stream(model_name, precision, task, H, W, nb, dev, seed=1, corr_prec=args.corr_precision, P=P)
            d = timed([s], steps, warmup, barrier)[0]
            f = steps * s.frames_per_step() / d
            r = {"fps": round(f, 2), "ms_per_frame": round(1e3 / f, 4), "frames_per_step": s.frames_per_step(), "precision": precision}
            if not keep:      # one extra context (weights + workspace) alive at a time
                del s
                s = None
                torch.cuda.empty_cache()
            return s, r
        Pm = main_s.P
        for prec in (("bf16", "f16x2") if args.with_bf16 else ("f16x2",)):
            if prec == args.precision:
                modes[prec] = {"fps": round(fps, 2), "ms_per_frame": round(1e3 / fps, 4), "frames_per_step": main_s.frames_per_step(), "precision": prec}
            else:
                _, modes[prec] = quick(model_name, prec, task, NB, P=Pm)
        if "bf16" in modes:
            modes["bf16"]["parity_note"] = ("bf16 operands miss the box-IoU bar: min 0.56 with the synthetic weights (profiles/r02_precision_budget.json), 0.89-0.91 "
                                            "with the trained-like ensemble (profiles/r04_precision_budget_trained_like_*.json); f16 single-pass 0.987")
        modes["retired"] = {"bf16": "not timed by default (--with-bf16): no 1-MFMA operand format meets box IoU >= 0.999, see DESIGN.md section 2"}
        if single is not None:
            configs["single_frame_latency"] = {k: single[k] for k in ("ms", "fps", "frames_per_step", "precision", "note")}
        torch.cuda.empty_cache()
        # BASELINE.json configs[1..3]
        _, configs["tiny_sot"] = quick("unicorn_track_tiny", args.precision, "sot", NB)
        if args.with_bf16:
            _, configs["tiny_sot_bf16"] = quick("unicorn_track_tiny", "bf16", "sot", NB)
        ms_, configs["large_mot_challenge_step"] = quick("unicorn_track_large_mot_challenge", args.precision, "mot", NB, keep=True)
        configs["large_mot_challenge_step"]["note"] = ("evaluate_omni loop body over %d consecutive frames: whole -> uni_postprocess (~200 candidates) -> interaction -> "
                                                       "upsample -> instance embeddings -> native QuasiDense match" % NB)
        # ---- tracker-level numbers (the reference drivers' own call pattern: one frame per call, host-synchronised), per-stage GPU ms
        from unicorn_amd.tracker import OmniMOTSFrame, QuasiDenseEmbedTracker, UnicornSOTTrack
        from unicorn_amd.utils.timing import NoTimer as NoTimer_
        from unicorn_amd.utils.timing import StageTimer
        g_ = torch.Generator().manual_seed(3)
        raw = [torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, generator=g_).pin_memory() for _ in range(4)]

        def ctx_roofline(model, fn, n=3):
            """roofline block of a CONFIG (not only the SOT step): `fn(i)` = one call of the config's loop body; the engine's
            per-launch HIP events (uni_prof_begin / uni_prof_end on the model's context, head levels serialised while profiling) give the
            GEMM-class time and FLOPs and the HBM-bound classes' time and algorithmic bytes per call"""
            import ctypes as C
            buf = (C.c_double * 16)()
            fn(0)
            torch.cuda.synchronize()
            L.check(L.lib().uni_prof_begin(model._ctx), "prof_begin")
            for i in range(n):
                fn(1 + i)
            torch.cuda.synchronize()
            L.check(L.lib().uni_prof_end(model._ctx, buf), "prof_end")
            v = list(buf)
            g_ms, g_work, g_n = v[0] / n, v[1] / n, v[2] / n
            ach = g_work / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0
            pk = {"bf16": 2500.0, "f16x2": round(2500.0 / 3, 1), "fp32": 157.3}[args.precision]
            hb = {}
            for i_, n_ in ((1, "dwconv7_ln"), (2, "gn_apply"), (3, "layernorm")):
                ms_1 = v[3 * i_] / n
                hb[n_] = {"ms_per_call": round(ms_1, 4), "GBps": round(v[3 * i_ + 1] / n / (ms_1 * 1e-3) / 1e9, 1) if ms_1 > 0 else 0,
                          "frac": round(v[3 * i_ + 1] / n / (ms_1 * 1e-3) / 8e12, 4) if ms_1 > 0 else 0, "launches": v[3 * i_ + 2] / n}
            return {"kernel": "GEMM class of this config (gemm_h2q / gemm_h2d / gemm_h2 / mlp_fused16 instantiations)", "bound": "mfma",
                    "achieved": round(ach, 2), "peak": pk, "unit": "TFLOP/s", "frac": round(ach / pk, 4), "frac_vs_f16_peak": round(ach / 2500.0, 4),
                    "gemm_ms_per_call": round(g_ms, 4), "gemm_launches_per_call": g_n, "flops_per_call": g_work,
                    "avg_launch_us": round(1e3 * g_ms / max(g_n, 1), 2), "hbm": hb, "misc_ms_per_call": round(v[12] / n, 4),
                    "note": "engine HIP events per launch (profiling mode: head levels and mask branch serialised); peak = 2500 / 3 MFMAs per f16x2 product"}

        def staged(run, timer, n=12, warm=2, stream=None, set_timer=None):
            """(1) one frame per call, host-synchronised per frame, with per-stage GPU / host ms (the reference loops' own pattern);
            (2) `stream(k)`: the same k frames through the pipelined generator API (run_stream / track_stream: frame t+1 is enqueued
            before the host blocks on frame t, the host association runs under the next frame's GPU work) -> ms_per_frame."""
            for i in range(warm):
                run(i)
            torch.cuda.synchronize()
            timer.summary()
            t1_ = time.perf_counter()
            for i in range(n):
                timer.start()
                run(warm + i)
            torch.cuda.synchronize()
            wall = (time.perf_counter() - t1_) / n
            gpu_ms, host_ms = timer.summary(per=n)
            r_ = {"ms_per_frame": round(1e3 * wall, 3), "fps": round(1.0 / wall, 2), "ms_per_frame_sync_each_frame": round(1e3 * wall, 3),
                  "stages_gpu_ms": {k: round(v, 3) for k, v in gpu_ms.items()}, "stages_host_ms": {k: round(v, 3) for k, v in host_ms.items()}}
            if stream is not None:
                from unicorn_amd.utils.timing import NoTimer
                set_timer(NoTimer())               # stage marks interleave across frames in the pipelined order: wall time only
                stream(4)
                torch.cuda.synchronize()
                k_ = 3 * n
                t1_ = time.perf_counter()
                got = stream(k_)
                torch.cuda.synchronize()
                wp = (time.perf_counter() - t1_) / k_
                assert got == k_, (got, k_)
                gsum = sum(gpu_ms.values())
                r_.update({"ms_per_frame": round(1e3 * wp, 3), "fps": round(1.0 / wp, 2), "pipelined": True,
                           "gpu_ms_sum_of_stages": round(gsum, 3),
                           "host_ms_hidden_under_gpu_work": round(1e3 * (wall - wp), 3)})
            return r_

        with torch.no_grad():
            if task == "sot" and not main_s.cfg.mask:      # (a) UnicornSOTTrack.track on raw 1080p uint8 RGB frames (pinned host memory)
                o_ = main_s.sot_batch(main_s.frames[1])["head"]
                sc_ = (o_[0, :, 4] * o_[0, :, 5]).sort(descending=True)[0]
                trk = UnicornSOTTrack(main_s.model, input_size=(H, W))
                trk.confthre = float((sc_[199] + sc_[200]) / 2)      # synthetic scores ~1e-4: ~200 candidates reach the NMS
                trk.initialize(raw[0], {"init_bbox": [480.0, 270.0, 480.0, 540.0]})
                trk.t = StageTimer()
                configs["sot_track_raw_1080p"] = staged(lambda i: trk.track(raw[1 + i % 3]), trk.t,
                                                        stream=lambda k: sum(1 for _ in trk.track_stream(raw[1 + j % 3] for j in range(k))),
                                                        set_timer=lambda t_: setattr(trk, "t", t_))
                torch.cuda.synchronize()
                t1_ = time.perf_counter()
                n4 = sum(1 for _ in trk.track_stream((raw[1 + j % 3] for j in range(48)), batch=4))
                torch.cuda.synchronize()
                configs["sot_track_raw_1080p"]["ms_per_frame_stream_batch4"] = round(1e3 * (time.perf_counter() - t1_) / n4, 3)
                configs["sot_track_raw_1080p"]["note"] = ("UnicornSOTTrack.track / track_stream per frame: pinned uint8 1080p -> H2D -> uni_letterbox -> backbone+FPN -> interaction -> "
                                                          "2 x upsample -> correlation -> head -> uni_postprocess (conf thr set for ~200 candidates) -> box")
            # (b) evaluate_omni loop, one frame per call
            ms_.omni.t = StageTimer()
            if ms_._gen is not None:               # the timed loop's pipelined generator still has frames admitted: retire it first
                ms_._gen.close()
                ms_._gen = None
            ms_.omni.reset()                       # a new "video" (tracker/omni.py: refuses while a pipeline is in flight)
            configs["mot_omni_loop"] = staged(lambda i: ms_.omni.run(ms_.frames[1 + i % 4], (1080, 1920)), ms_.omni.t,
                                              stream=lambda k: sum(1 for _ in ms_.omni.run_stream((ms_.frames[1 + j % 4] for j in range(k)), (1080, 1920))),
                                              set_timer=lambda t_: setattr(ms_.omni, "t", t_))
            configs["mot_omni_loop"]["note"] = "mot_evaluator.py:991-1045 per frame on unicorn_track_large_mot_challenge, ~200 NMS candidates, native association"
            ms_.omni.t = NoTimer_()
            configs["mot_omni_loop"]["roofline"] = ctx_roofline(ms_.model, lambda i: ms_.omni.run(ms_.frames[1 + i % 4], (1080, 1920)))
            ms_.omni.reset()
            configs["large_mot_challenge_step"]["roofline"] = ctx_roofline(ms_.model, lambda i: ms_.omni.run_batch(ms_.batches[i % 4], (H, W)))
            # (b') tools/track.py's OWN loop: MOTEvaluator.evaluate (mot_evaluator.py:198-222) = mode="whole" -> postprocess -> native BYTETracker.update ->
            # area / aspect filter (unicorn_amd.tracker.ByteMOTFrame).  BYTETracker's logic runs on absolute score thresholds (0.1 floor, det_thresh =
            # track_thresh + 0.1): the synthetic heads (scores ~1e-4) get detector-like scores here by zero obj / cls prediction biases and doubled
            # prediction weights (the same planting as tests/planted.py:confident_head; top-300 scores ~0.5 - 0.94)
            from types import SimpleNamespace as NS_
            from unicorn_amd.tracker import BYTETracker, ByteMOTFrame
            Pb_ = dict(ms_.P)
            for k_ in list(Pb_):
                if k_.startswith("head.") and (".obj_preds" in k_ or ".cls_preds" in k_):
                    Pb_[k_] = torch.zeros_like(Pb_[k_]) if k_.endswith(".bias") else Pb_[k_] * 2.0
            bs_ = Stream("unicorn_track_large_mot_challenge", args.precision, "sot", H, W, 1, dev, seed=1, corr_prec=args.corr_precision, P=Pb_)
            ob_, _ = bs_.model(bs_.frames[1])
            scb_ = (ob_[0, :, 4] * ob_[0, :, 5]).sort(descending=True)[0]
            # ~100 candidates per frame (a crowded MOT17 / MOT20 frame; the exact assignment is O(n^3): 300 candidates cost 8.4 ms of host time per frame)
            byte_ = ByteMOTFrame(bs_.model, BYTETracker(NS_(track_thresh=float((scb_[49] + scb_[50]) / 2), track_buffer=30, match_thresh=0.9, mot20=False)),
                                 (H, W), num_classes=1, confthre=float((scb_[99] + scb_[100]) / 2), nmsthre=0.7, min_box_area=100, timer=StageTimer())
            info_b = (1080, 1920, 1, 1, "synthetic/000001.jpg")
            ntr_ = [0]

            def run_byte(i):
                r_ = byte_.run(bs_.frames[1 + i % 4], info_b)
                ntr_[0] = max(ntr_[0], 0 if r_ is None else len(r_[1]))
            configs["byte_track_loop"] = staged(run_byte, byte_.t,
                                                stream=lambda k: sum(1 for _ in byte_.run_stream((bs_.frames[1 + j % 4] for j in range(k)), info_b)),
                                                set_timer=lambda t_: setattr(byte_, "t", t_))
            configs["byte_track_loop"].update({"tracks_reported_max": ntr_[0], "candidates_after_conf_filter": 100,
                                               "note": "mot_evaluator.py:198-222 (tools/track.py's loop) per frame on unicorn_track_large_mot_challenge: whole -> "
                                                       "uni_postprocess -> native BYTETracker.update (Kalman filter, IoU + score fusion, exact assignment) -> filter; "
                                                       "detector-like scores planted (zero obj / cls biases, prediction weights x2)"})
            del bs_, byte_
        del ms_
        torch.cuda.empty_cache()
        with torch.no_grad():      # (c) MOTS loop (mot_evaluator.py:770-890): CondInst masks, overlap-free merge, device RLE
            mm_ = Stream("unicorn_track_large_mot_challenge_mask", args.precision, "mot", H, W, 1, dev, seed=1, corr_prec=args.corr_precision)
            o_, _ = mm_.model(mm_.frames[1])
            sc_ = (o_[0][0, :, 4] * o_[0][0, :, 5]).sort(descending=True)[0]
            thr_ = float((sc_[63] + sc_[64]) / 2)
            kw_ = dict(init_score_thr=float(sc_[16]), obj_score_thr=float(sc_[40]), match_score_thr=0.5, memo_tracklet_frames=10, memo_backdrop_frames=1,
                       memo_momentum=0.8, nms_conf_thr=float(sc_[40]), nms_backdrop_iou_thr=0.3, nms_class_iou_thr=0.7, with_cats=True, match_metric="bisoftmax")
            mots = OmniMOTSFrame(mm_.model, QuasiDenseEmbedTracker(**kw_), (H, W), num_classes=1, confthre=thr_, nmsthre=0.7, embed_score_thr=thr_,
                                 mask_thres=0.3, d_rate=mm_.cfg.d_rate, timer=StageTimer())
            nrle = [0]

            def run_mots(i):
                r_ = mots.run(mm_.frames[1 + i % 4], (1080, 1920))
                nrle[0] = len(r_[1])
            configs["mots_loop"] = staged(run_mots, mots.t, n=8,
                                          stream=lambda k: sum(1 for _ in mots.run_stream((mm_.frames[1 + j % 4] for j in range(k)), (1080, 1920))),
                                          set_timer=lambda t_: setattr(mots, "t", t_))
            configs["mots_loop"]["rle_strings_last_frame"] = nrle[0]
            mots.t = NoTimer_()
            configs["mots_loop"]["roofline"] = ctx_roofline(mm_.model, run_mots)
            configs["mots_loop"]["note"] = ("MOTS loop per frame on unicorn_track_large_mot_challenge_mask: postprocess_inst (64 candidates) + CondInst masks -> "
                                            "uni_mask_resize > thr at 1080p -> association -> uni_mots_overlap_free -> uni_rle_encode strings")
        del mm_, mots
        torch.cuda.empty_cache()
        vs, configs["large_vos_k3"] = quick("unicorn_track_large_mask", args.precision, "vos", 1, steps=6, warmup=2, keep=True)
        configs["large_vos_k3"]["note"] = "3 objects per frame: one backbone, per object correlation + head + CondInst masks + postprocess (UnicornVOSTrack.step)"
        with torch.no_grad():
            configs["large_vos_k3"]["roofline"] = ctx_roofline(vs.model, lambda i: vs.trk.step(vs.frames[1 + i % 4]))
            # stage table of the VOS step (host-synchronised per stage, tools/vos_profile.py's cut): where the frame goes
            def vt(fn_, n_=4):
                fn_()
                torch.cuda.synchronize()
                t1_ = time.perf_counter()
                for _ in range(n_):
                    r_ = fn_()
                torch.cuda.synchronize()
                return round(1e3 * (time.perf_counter() - t1_) / n_, 3), r_
            tr_ = vs.trk
            st_ = {}
            st_["backbone+fpn"], (fpn_, dcur_) = vt(lambda: vs.model(imgs=vs.frames[1], mode="backbone"))
            st_["group: interaction + 2 x upsample + correlation (K rows) + head (K objects) + postprocess_inst + CondInst"], _ = vt(
                lambda: tr_.get_mask_results(fpn_, dcur_, tr_.out_dict_pre, 1.0, tr_.init_object_ids))
            st_["whole step (UnicornVOSTrack.step)"], _ = vt(lambda: tr_.step(vs.frames[1]))
            configs["large_vos_k3"]["stages_ms_host_synchronised"] = st_
        if not args.no_cpu_baseline:      # mask parity of the VOS config on one frame (oracle loop over the 3 objects)
            with torch.no_grad():
                res, _ = vs.trk.step(vs.frames[1])
                torch.set_num_threads(min(os.cpu_count() or 1, 16))
                st = uo.vos_init(vs.P, vs.cfg, vs.frames[0].cpu(), vs.vos_boxes)
                exp = uo.vos_step(vs.P, vs.cfg, st, vs.frames[1].cpu())
                torch.set_num_threads(1)
            mi, bi = [], []
            for k in vs.vos_boxes:
                d_o, m_o = exp[k]
                d_h, m_h = res[k]
                if d_o is None or d_h is None:
                    continue
                a, b = m_h.cpu() > 0.5, m_o > 0.5
                mi.append(float((a & b).sum()) / max(float((a | b).sum()), 1.0))
                cx = lambda t: torch.stack([(t[0] + t[2]) / 2, (t[1] + t[3]) / 2, t[2] - t[0], t[3] - t[1]])[None]
                bi.append(float(box_iou_pairs(cx(d_h.cpu()), cx(d_o))[0]))
            if mi and parity is not None:
                parity["mask_iou_min"] = round(min(mi), 6)
                parity["vos_best_box_iou_min"] = round(min(bi), 6)
                parity["pass"] = bool(parity["pass"] and min(mi) >= 0.999)
            configs["large_vos_k3"]["parity"] = {"mask_iou_min": min(mi) if mi else None, "best_box_iou_min": min(bi) if bi else None}
        # (d) VOS with 16 objects in one reference group: ONE correlation pass (16 value rows) + ONE object-batched head call
        with torch.no_grad():
            trk16 = vs.trk
            bx16 = {str(k_ + 1): [W * (0.05 + 0.22 * (k_ % 4)), H * (0.05 + 0.22 * (k_ // 4)), W * 0.18, H * 0.18] for k_ in range(16)}
            trk16.initialize(vs.frames[0], {"init_object_ids": list(bx16), "init_bbox": bx16})
            for i in range(2):
                trk16.step(vs.frames[1 + i])
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for i in range(5):
                trk16.step(vs.frames[1 + i % 4])
            torch.cuda.synchronize()
            d16 = (time.perf_counter() - t1) / 5
        configs["large_vos_k16"] = {"fps": round(1.0 / d16, 2), "ms_per_frame": round(1e3 * d16, 3), "frames_per_step": 1, "precision": args.precision,
                                    "note": "16 objects per frame (UnicornVOSTrack.step): one backbone, one 16-row correlation pass, one object-batched head call, CondInst masks"}

    if rank == 0:
        nf = main_s.frames_per_step()
        dtype = {"f16x2": "f16x2 (fp32-equivalent: split-f16 MFMA operands, fp32 accumulate)", "bf16": "bf16", "fp32": "f32"}[args.precision]
        line = {
            "metric": "frames/sec @ %dx%d %s" % (H, W, args.model), "value": round(fps, 3), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(1e3 * dt / args.steps, 4),
            "frames_per_step": nf, "ms_per_frame": round(1e3 * dt / (args.steps * nf), 4),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": "%s %s per-frame step %dx%d (backbone+FPN, deform interaction, embedding, fp32-equivalent correlation, "
                                   "head); one independent stream per GPU, %d consecutive frames per step" % (args.model, args.task.upper(), H, W, nf),
                       "model": args.model, "task": args.task, "precision": args.precision, "frames_per_step": nf, "streams": world,
                       "distinct_frames_per_batch": main_s.distinct_frames_per_batch,
                       "weights": "synthetic (oracle/synth.py)",
                       "corr_dtype": ["f32", "f32-equivalent (bf16x3 split operands, fp32 accumulate)",
                                      "f32-equivalent (f16x2 split operands, fp32 accumulate)",
                                      "f16 (single pass, reference driver class)"][args.corr_precision], "accum": "f32",
                       "rank_tasks": per_rank, "gather": gstat if world > 1 else None},
            "single_frame": single,
            "parity": parity, "roofline": roof, "cpu_baseline": cpu, "modes": modes, "configs": configs, "kernels": extra,
            "rank_errors": rank_errors,
            # third-party arithmetic on the path that no reference-owned vector pins (absent offline: SURVEY.md 8c); also inside `parity`
            "parity_unpinned": ["cv2.resize", "torchvision.nms", "pycocotools.rle", "lap.lapjv", "cython_bbox.bbox_overlaps"],
        }
        print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
