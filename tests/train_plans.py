"""The launch plans of the ConvNeXt training operators (ops.layernorm_cf / csrc/lncf_train.hip, ops.dwconv7_ln / csrc/dwln_train.hip,
ops.block_tail / csrc/block_tail.hip, ops.pw_mlp / csrc/pw_mlp.hip), written down as explicit lists, and the maps their parity cases run on.

A launcher's variant tag (uni_variant_trace, include/unicorn_hip.h) reads `<operator> <fwd|bwd...><plan> <need flags>`, for instance
`lncf_train bwd_cl<f16,V=8,NV=3> G=4 gx=1 gwb=1`.  The PLAN CLASS of a tag is the part between the kernel name and the need flags:
`cl<f16,V=8,NV=3> G=4`.  It names the template instantiation and the lane mapping, and the forward and the backward of one call carry the
same one.  EXPECTED lists, per operator, every plan class the host code can pick for C = 4, 8, ..., 2048 (lncf_plan, dwln_plan in
csrc/train_plan.h).  tests/test_train_plans_gpu.py sweeps every C on the device and demands that the classes found are EXPECTED, in both
directions -- a retuned plan function shows up as a diff of these lists, an instantiation nobody can reach as well -- and then runs the
smallest and the largest C of every class against the operator's restatement.  block_tail's tag does not carry its plan (PP = 512 / (C / V)
is a kernel argument, not a template argument), so it has an explicit list of widths instead.

predicted() and bt_class() do not restate the plans: they answer from what the host code itself prints, `tools/build/train_plan_check --list`
(tools/train_plan_check.cpp over csrc/train_plan.h, the header the launchers read).

Data and small helpers only: no GPU work, importable without a device."""
import functools
import os
import re
import subprocess

C_STEP, C_MAX = 4, 2048                     # train_shape_ok (csrc/train_plan.h): C % 4 == 0, 4 <= C <= TRAIN_MAX_C
SWEEP_C = tuple(range(C_STEP, C_MAX + 1, C_STEP))

# (N, H, W) of the parity cases.  21 pixels per image and 42 in all: neither is a multiple of any pixels-per-block value of the channels-last
# kernels (4 .. 256) or of the 64-pixel tile of the NCHW kernels, and a tile ends with its image.  block_tail runs three samples of this map.
MAP = (2, 3, 7)
# dwln: W = 11 is two strips of 8 pixels per row in fp32, the last of 3; six strips of 2 in fp64, the last of 1
MAP_DW = (2, 5, 11)

# every stage width of the ConvNeXt variants (96 .. 1536, 128 .. 1024, 192 .. 1536, 256 .. 2048), the smallest V = 8 width and four ragged ones:
#   C = 384: PP = 5; 768: PP = 2 on 384 threads; 2048: CG = 512, PP = 1; 1000: PP = 2, 12 threads of the block idle; 500: PP = 4, 12 idle;
#   2044: PP = 1, one idle lane; in NCHW memory 1000 and 2044 end in a partial channel tile behind 15 and 31 whole ones
WIDTHS_BT = (8, 96, 100, 128, 192, 256, 384, 500, 512, 768, 1000, 1024, 1536, 2044, 2048)
SCALE_BT = (1 / 0.7, 0.0, 1 / 0.7)          # the middle sample dropped, as STRADDLE of tests/test_block_tail_gpu.py

_G = (1, 2, 4, 8, 16, 32, 64)
# channels-last lncf: (NV, G) with G NV >= C / V and the fewest idle vector slots.  NV = 1 and NV = 3 exist at every G; 2, 4, 6 and 8 only
# at G = 64 (below it a smaller NV with a larger G has as few idle slots and wins the tie)
_CL_V4 = [(1, g) for g in _G] + [(2, 64)] + [(3, g) for g in _G] + [(4, 64), (6, 64), (8, 64)]          # 18
_CL_V8 = [(1, g) for g in _G] + [(2, 64)] + [(3, g) for g in _G] + [(4, 64)]                            # 16: C / 8 <= 256 = 4 x 64
# half x with C % 8 == 4 stays at V = 4: C / 4 is odd there, so NV = 1 with G = 2 or 4 (C = 8, 16) cannot occur; the other sixteen can
_CL_V4_HALF = [p for p in _CL_V4 if p not in ((1, 2), (1, 4))]                                          # 16


def _cl(dt, V, pairs):
    return ["cl<%s,V=%d,NV=%d> G=%d" % (dt, V, nv, g) for nv, g in pairs]


EXPECTED = {
    "lncf": (_cl("f32", 4, _CL_V4) + _cl("f64", 4, _CL_V4)
             + _cl("f16", 8, _CL_V8) + _cl("bf16", 8, _CL_V8) + _cl("f16", 4, _CL_V4_HALF) + _cl("bf16", 4, _CL_V4_HALF)
             # NCHW: 16 channels per lane in registers (C <= 128), 32 (fp32 arithmetic only, C <= 256), else streamed in chunks of 8
             + ["nchw<%s,%s>" % (dt, plan) for dt in ("f32", "f16", "bf16") for plan in ("regs=16", "regs=32", "stream=8")]
             + ["nchw<f64,regs=16>", "nchw<f64,stream=8>"]),
    # wps = ceil(C / 4 / 64) waves per strip, NS = 512 / (64 wps) strips per block; 8 pixels per lane in fp32, 2 in fp64
    "dwln": ["<%s,PXT=%d> wps=%d NS=%d" % (dt, pxt, wps, 512 // (64 * wps)) for dt, pxt in (("f32", 8), ("f64", 2)) for wps in range(1, 9)],
}

# the classes no test had launched before this table existed, for the record and for the census file
FIRST_RUN = {
    "lncf": [c for c in EXPECTED["lncf"] if re.search(r"NV=[248]>|V=8,NV=[124]>|^cl<(f16|bf16),V=4,NV=[68]>|regs=32", c)],
    "dwln": [c for c in EXPECTED["dwln"] if re.search(r"wps=[4578] ", c)],
}


# ---------------------------------------------------------------------------------------------------------------- pw_mlp
# pw_plan (csrc/train_plan.h) over N = 4, 8, ..., 8192: a plan class is (dtype, V, L) -- `<f16,V=8> L=16` -- with V = N's columns per lane and
# L the lanes per row of a block.  tests/test_pw_mlp_plans_gpu.py sweeps every N and runs every class; train_plan_census.json and the two
# dicts above stay those of the three operators swept first, so pw_mlp has lists of its own.
N_STEP, N_MAX = 4, 8192                     # pw_width_ok: N % 4 == 0, 4 <= N <= PW_MAX_H
SWEEP_N = tuple(range(N_STEP, N_MAX + 1, N_STEP))
PW_DTYPES = ("f32", "f64", "f16", "bf16")
_PW_L = (1, 2, 4, 8, 16, 32, 64, 128, 256)
# half types at V = 4 are the widths with N % 8 == 4: N / 4 is odd, so L = 2 (N = 8 alone, which takes V = 8) cannot occur
_PW_L_HALF4 = tuple(L for L in _PW_L if L != 2)


def _pw(dt, V, ls):
    return ["<%s,V=%d> L=%d" % (dt, V, L) for L in ls]


EXPECTED_PW = (_pw("f32", 4, _PW_L) + _pw("f64", 4, _PW_L) + _pw("f16", 8, _PW_L) + _pw("bf16", 8, _PW_L)
               + _pw("f16", 4, _PW_L_HALF4) + _pw("bf16", 4, _PW_L_HALF4))                                # 2 x 9 + 2 x 9 + 2 x 8 = 52

# the widths (Hd and Co) at which a test compared pw_mlp with a reference before this list existed: the fixtures, the wide and long shapes
# and the mini-backbone of tests/test_pw_mlp_gpu.py.  pw_first_run() is every class none of them reaches.
PW_WIDTHS_BEFORE = {"f32": (4, 12, 16, 24, 32, 48, 64, 96, 100, 128, 192, 1536, 2048, 6144, 8192),
                    "f64": (4, 12, 16, 24, 32, 48, 64, 96, 100, 128, 192),
                    "f16": (12, 16, 24, 32, 48, 64, 96, 100, 128, 192),
                    "bf16": (12, 16, 24, 48, 96, 100, 192)}


PLAN_CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "build", "train_plan_check")


@functools.lru_cache(maxsize=None)
def plan_list():
    """`train_plan_check --list`, run once: ({(op, layout, dt, C): (plan class, {"PP" | "block" | "L" | "gx" | "idle": value})}, {limit: value}); op is lncf,
    block_tail, dwln or pw_mlp, layout is "" for the two operators that have one layout only"""
    if not os.path.exists(PLAN_CHECK):
        raise AssertionError("tools/build/train_plan_check is missing: run __graft_entry__.build() (csrc/build.sh builds it)")
    r = subprocess.run([PLAN_CHECK, "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    plans, limits = {}, {}
    for line in r.stdout.splitlines():
        head, *rest = line.split(" | ")
        if head == "limits":
            limits = {k: int(v) for k, v in (kv.split("=") for kv in rest[0].split())}
            continue
        op, layout, dt, C = head.split()
        extra = {k: int(v) for k, v in (kv.split("=") for kv in rest[1].split())} if len(rest) > 1 else {}
        key = (op, "" if layout == "-" else layout, dt, int(C))
        assert key not in plans, key
        plans[key] = (rest[0], extra)
    return plans, limits


def predicted(op, layout, dt, C):
    """The plan class the host code (csrc/train_plan.h) picks: it picks the widths of the CPU checks and says where a class begins and ends"""
    return plan_list()[0][(op, layout, dt, C)][0]


_FLAGS = re.compile(r"(?: (?:gx|gwb|du|gb|gy|gg)=\d+)+$")
_KERNEL = re.compile(r"^(lncf_train|dwln_train|block_tail) (fwd|bwd)(_a|_dx)?_?")


def strip_flags(tag):
    """a variant tag without its trailing need flags (gx= gwb=, du= gb=, gy= gg=)"""
    return _FLAGS.sub("", tag)


def plan_class(tag):
    """the plan class of a map kernel's tag: 'lncf_train bwd_cl<f32,V=4,NV=3> G=8 gx=1 gwb=0' -> 'cl<f32,V=4,NV=3> G=8',
    'dwln_train bwd_a<f32,PXT=8> wps=1 NS=8 du=1 gb=1' -> '<f32,PXT=8> wps=1 NS=8'.  None for a tag that is not one of a map kernel
    (the reduce launches, the weight pass of dwln)"""
    m = _KERNEL.match(tag)
    if not m or " reduce" in tag or "bwd_dw" in tag:
        return None
    return strip_flags(tag[m.end():])


def group(by_c):
    """{C: tag} -> {tag: [C, ...]}, every list ascending"""
    out = {}
    for C in sorted(by_c):
        out.setdefault(by_c[C], []).append(C)
    return out


def ends(cs):
    """the smallest and the largest C of a class (one value where they coincide): the smallest has the most idle vector slots or lanes, the
    largest is the full one"""
    return sorted({min(cs), max(cs)})


def bt_class(layout, dt, C):
    """the plan part of the block_tail tag at width C: V = 8 for half y where C allows it"""
    return plan_list()[0][("block_tail", layout, dt, C)][0]


def plan_extra(op, layout, dt, C):
    """what the list says next to the class: PP and block for block_tail; for pw_mlp L, and at M = 1 gx (column tiles of L vectors) and idle
    (vector slots of those tiles that no vector fills)"""
    return plan_list()[0][(op, layout, dt, C)][1]


def zero_one_vector(x, C):
    """x (N, C, H, W) with the last 4-channel vector of pixel (0, 0, 0) zeroed: what a lane whose `vok`, G or slot index is wrong reads"""
    x = x.clone()
    x[0, C - 4:C, 0, 0] = 0.0
    return x


# ---------------------------------------------------------------------------------------------------------------- pw_mlp: classes, widths, rows
_PW_TAG = re.compile(r"^pw_mlp (act_fwd|act_bwd|colsum)(<[^>]+> L=\d+)")


def pw_tag(tag):
    """('act_fwd' | 'act_bwd' | 'colsum', plan class) of a map kernel's tag: 'pw_mlp act_bwd<f16,V=8> L=16 a=1 gh=1 gb=1' -> ('act_bwd',
    '<f16,V=8> L=16'); None for the reduce launch"""
    m = _PW_TAG.match(tag)
    return (m.group(1), m.group(2)) if m else None


@functools.lru_cache(maxsize=None)
def pw_classes(dt):
    """{plan class: [N, ...]} of the element type dt over SWEEP_N, as the host code says (train_plan_check --list)"""
    return group({N: predicted("pw_mlp", "", dt, N) for N in SWEEP_N})


def pw_lanes(cls):
    """L of a plan class"""
    return int(cls.rsplit("L=", 1)[1])


def pw_first_run():
    """the classes no test had compared with a reference before tests/test_pw_mlp_plans_gpu.py, in the order of EXPECTED_PW"""
    before = {predicted("pw_mlp", "", dt, N) for dt, ws in PW_WIDTHS_BEFORE.items() for N in ws}
    return [c for c in EXPECTED_PW if c not in before]


def pw_widths(dt, cls):
    """(lo, hi, ragged) of a class: its smallest and its largest N, and the smallest N with more than one column tile (gx > 1) AND idle vector
    slots in the last one (idle > 0) -- `vok` false in a block with blockIdx.x > 0.  Classes with L < 8 have one tile only: ragged = lo"""
    ns = pw_classes(dt)[cls]
    ragged = [N for N in ns if plan_extra("pw_mlp", "", dt, N)["gx"] > 1 and plan_extra("pw_mlp", "", dt, N)["idle"] > 0]
    assert bool(ragged) == (pw_lanes(cls) >= 8), (cls, ragged[:1])
    return ns[0], ns[-1], ragged[0] if ragged else ns[0]


def pw_rows(L):
    """(M_short, M_loop) for a class of L lanes per row, rpb = 256 / L rows per group.  M_short = rpb + 5: two groups, the second with five
    live slots.  M_loop = 256 rpb + rpb + 5: 258 groups on PW_ROWS = 256 rows of partials, so blockIdx.y 0 and 1 take two groups each and the
    last group has five rows.  That is so for rpb > 5 (L <= 32); with 4, 2 and 1 rows per group the same counts make 3, 4, 6 and 259, 260, 262
    groups (tests/test_train_plans_cpu.py states it)"""
    rpb = 256 // L
    return rpb + 5, 256 * rpb + rpb + 5


def pw_shapes(dt):
    """[(class, M, N)]: per class of dt, lo and hi at M_short and ragged at M_loop"""
    out = []
    for cls in pw_classes(dt):
        lo, hi, ragged = pw_widths(dt, cls)
        short, loop = pw_rows(pw_lanes(cls))
        out += [(cls, short, lo), (cls, short, hi), (cls, loop, ragged)]
    return out
