"""The plan lists of the ConvNeXt training operators (tests/train_plans.py) without a GPU: the host check of the launch plans
(tools/train_plan_check.cpp over csrc/train_plan.h) holds over its whole domain; the lists are well formed and every class is a string the
header's own formatters print; the plans of the host code give exactly the lists; the fp32 yardstick of the restatements is positive at the
widths tests/test_train_plans_gpu.py runs, so its 4 x bound never collapses to "<= 0"; and a lane that reads the wrong vector would miss that
bound by more than 100 x."""
import functools
import os
import re
import subprocess

import pytest
import torch

import block_tail_ref as RB
import dwln_train_ref as RD
import lncf_ref as RL
import pw_mlp_ref as RP
import train_plans as P

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unicorn_amd", "csrc")
ENAMES = ("f32", "f16", "bf16", "f64")           # train_ename (csrc/train_plan.h)


def test_the_plans_hold_over_the_whole_admitted_domain():
    """block size, grid, counters, lane mappings, partials inside the workspace, LDS and the size functions, at every point of the domain;
    and each condition refuses a deliberately wrong plan"""
    P.plan_list()                               # fails by name where the program was not built
    r = subprocess.run([P.PLAN_CHECK], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "train_plan_check: OK" in r.stdout and "FAIL" not in r.stdout
    assert re.search(r"each condition bites: [1-9]\d* deliberately wrong plans refused", r.stdout)


def test_the_limits_of_ops_are_the_limits_of_the_header():
    from unicorn_amd import ops
    limits = P.plan_list()[1]
    assert ops.TRAIN_MAX_C == limits["TRAIN_MAX_C"] == P.C_MAX and ops.PW_MLP_MAX_H == limits["PW_MAX_H"]
    assert limits["TRAIN_ROWS"] == 1024 and limits["PW_ROWS"] == 256


def _printable(op):
    """every plan class the formatter of `op` in csrc/train_plan.h writes over the whole domain (train_plan_check --list)"""
    out = {cls for (o, _, _, _), (cls, _) in P.plan_list()[0].items() if o == op}
    assert out, op
    return out


def test_expected_is_well_formed():
    for op, classes in P.EXPECTED.items():
        assert len(classes) == len(set(classes)), (op, sorted(c for c in classes if classes.count(c) > 1))
    assert len(P.EXPECTED["lncf"]) == 2 * 18 + 2 * 16 + 2 * 16 + 11 and len(P.EXPECTED["dwln"]) == 16
    for op in P.EXPECTED:
        assert P.FIRST_RUN[op] and set(P.FIRST_RUN[op]) < set(P.EXPECTED[op])
    assert len(P.WIDTHS_BT) == len(set(P.WIDTHS_BT)) and all(C % 4 == 0 and 4 <= C <= P.C_MAX for C in P.WIDTHS_BT)
    n, h, w = P.MAP
    for per_block in (4, 8, 16, 32, 64, 128, 256):
        assert (h * w) % per_block and (n * h * w) % per_block
    assert P.MAP_DW[2] % 8 == 3 and P.MAP_DW[2] % 2 == 1 and -(-P.MAP_DW[2] // 8) == 2 and -(-P.MAP_DW[2] // 2) == 6


def test_every_class_is_a_tag_the_launchers_can_print():
    """a class is one the header's formatter prints (the launchers put it between the kernel name and the need flags), with a dtype of
    train_ename and a layout the launcher has; and plan_class finds it again in the whole tag"""
    lncf, dwln, bt = _printable("lncf"), _printable("dwln"), _printable("block_tail")
    for cls in P.EXPECTED["lncf"]:
        for kind, flags in (("fwd", "gx=0 gwb=0"), ("bwd", "gx=1 gwb=1")):
            tag = "lncf_train %s_%s %s" % (kind, cls, flags)
            assert cls in lncf, tag
            assert P.plan_class(tag) == cls and P.strip_flags(tag) == "lncf_train %s_%s" % (kind, cls)
        assert re.match(r"^(cl|nchw)<(%s)," % "|".join(ENAMES), cls), cls
    for cls in P.EXPECTED["dwln"]:
        for tag in ("dwln_train fwd%s" % cls, "dwln_train bwd_a%s du=1 gb=1" % cls, "dwln_train bwd_dx%s" % cls):
            assert cls in dwln, tag
            assert P.plan_class(tag) == cls
        assert re.match(r"^<(f32|f64),", cls), cls
    for layout in ("cl", "nchw"):
        for dt in ENAMES:
            for C in P.WIDTHS_BT:
                tag = "block_tail bwd_%s gy=1 gg=1" % P.bt_class(layout, dt, C)
                assert P.bt_class(layout, dt, C) in bt and re.match(r"^block_tail bwd_(cl<(%s),V=[48]>|nchw<(%s)>) " % (("|".join(ENAMES),) * 2), tag), tag
                assert P.plan_class(tag) == P.bt_class(layout, dt, C)
    for tag in ("lncf_train reduce<f32>", "block_tail reduce<f64>", "dwln_train reduce<f32> dw=1 gb=1", "dwln_train bwd_dw<f32> slen=65"):
        assert P.plan_class(tag) is None, tag
    assert P.group({8: "a", 4: "a", 12: "b"}) == {"a": [4, 8], "b": [12]} and P.ends([4, 8, 12]) == [4, 12] and P.ends([4]) == [4]
    # the launchers format no plan class of their own: the tag text is stated once, in the header
    for unit in ("lncf_train.hip", "dwln_train.hip", "block_tail.hip", "pw_mlp.hip"):
        text = open(os.path.join(CSRC, unit)).read()
        assert "_plan_class(" in text and not re.search(r'uni_variant_note\("[^"]*(V=|PXT=|NV=|regs=|stream=)', text), unit


def test_the_block_tail_widths_are_what_their_comment_says():
    """the PP and idle-thread facts next to train_plans.WIDTHS_BT, for fp32 y in channels-last memory (4 channels per lane)"""
    facts = {384: (5, 512, 32), 768: (2, 384, 0), 2048: (1, 512, 0), 1000: (2, 512, 12), 500: (4, 512, 12), 2044: (1, 512, 1)}      # PP, block, idle
    for C, (pp, block, idle) in facts.items():
        assert C in P.WIDTHS_BT
        got = P.plan_extra("block_tail", "cl", "f32", C)
        assert (got["PP"], got["block"], got["block"] - got["PP"] * (C // 4)) == (pp, block, idle), (C, got)
    assert 2048 // 4 == 512                                                                  # CG = 512 at the widest C
    assert -(-1000 // 64) == 15 + 1 and 1000 % 64 and -(-2044 // 64) == 31 + 1 and 2044 % 64      # NCHW: a partial channel tile behind 15 and 31 whole ones


def _predicted_classes(op, combos):
    return {(layout, dt): P.group({C: P.predicted(op, layout, dt, C) for C in P.SWEEP_C}) for layout, dt in combos}


def test_the_restated_plan_arithmetic_gives_exactly_the_lists():
    lncf = _predicted_classes("lncf", [(lay, dt) for lay in ("cl", "nchw") for dt in ENAMES])
    dwln = _predicted_classes("dwln", [("", "f32"), ("", "f64")])
    for op, per in (("lncf", lncf), ("dwln", dwln)):
        got = [cls for classes in per.values() for cls in classes]
        assert len(got) == len(set(got)) and sorted(got) == sorted(P.EXPECTED[op]), sorted(set(got) ^ set(P.EXPECTED[op]))
    f32 = lncf[("cl", "f32")]
    assert (f32["cl<f32,V=4,NV=2> G=64"][0], f32["cl<f32,V=4,NV=2> G=64"][-1]) == (388, 512)
    assert (f32["cl<f32,V=4,NV=8> G=64"][0], f32["cl<f32,V=4,NV=8> G=64"][-1]) == (1540, 2048)
    assert (lncf[("cl", "f16")]["cl<f16,V=4,NV=8> G=64"][0], lncf[("cl", "f16")]["cl<f16,V=4,NV=8> G=64"][-1]) == (1540, 2044)
    assert lncf[("nchw", "f32")]["nchw<f32,regs=32>"] == list(range(132, 257, 4))
    assert dwln[("", "f32")]["<f32,PXT=8> wps=4 NS=2"] == list(range(772, 1025, 4))


# ------------------------------------------------------------------------------------------------ the yardstick is never zero
@functools.lru_cache(maxsize=None)
def lncf_yardstick(C):
    ins = RL.draw("plain", C + sum(P.MAP), (P.MAP[0], C) + P.MAP[1:])
    ref, f32 = RL.value_and_grads(*ins, dtype=torch.float64), RL.value_and_grads(*ins, dtype=torch.float32)
    return ins, ref, {n: RL.rel_err(f32[n], ref[n]) for n in RL.RESULTS}


def test_lncf_fp32_yardstick_is_positive_at_both_ends_of_every_class():
    widths = sorted({C for cs in P.group({C: P.predicted("lncf", "cl", "f32", C) for C in P.SWEEP_C}).values() for C in P.ends(cs)})
    assert len(widths) == 32 and widths[0] == 4 and widths[-1] == 2048          # 18 classes, four of one width (C = 4, 8, 12, 16)
    for C in widths:
        dev = lncf_yardstick(C)[2]
        print("C=%4d " % C + "  ".join("%s %.2e" % kv for kv in dev.items()))
        assert all(0 < v < 1e-5 for v in dev.values()), (C, dev)


def test_dwln_and_block_tail_fp32_yardsticks_are_positive():
    """dwln at both ends of every class (its x and parameters are drawn on a grid; grad_y and the normalisation are not); block_tail at every
    listed width, where g_residual is grad_out itself: that yardstick is zero by construction and the result is held to the exact bits"""
    for C in sorted({C for cs in P.group({C: P.predicted("dwln", "", "f32", C) for C in P.SWEEP_C}).values() for C in P.ends(cs)}):
        ins = RD.draw("plain", C + sum(P.MAP_DW), (P.MAP_DW[0], C) + P.MAP_DW[1:])
        ref, f32 = RD.value_and_grads(*(t.double() for t in ins)), RD.value_and_grads(*ins)
        dev = {n: RD.rel_err(f32[n], ref[n]) for n in RD.RESULTS}
        assert all(0 < v < 1e-5 for v in dev.values()), (C, dev)
    for C in P.WIDTHS_BT:
        ins = RB.draw("plain", C + 3 + sum(P.MAP[1:]), (3, C) + P.MAP[1:], scale=P.SCALE_BT)
        ref, f32 = RB.value_and_grads(*ins, dtype=torch.float64), RB.value_and_grads(*ins, dtype=torch.float32)
        dev = {n: RB.rel_err(f32[n], ref[n]) for n in RB.RESULTS}
        assert dev.pop("g_residual") == 0.0 and torch.equal(f32["g_residual"], ins[4])
        assert all(0 < v < 1e-5 for v in dev.values()), (C, dev)


# ------------------------------------------------------------------------------------------------ a wrong lane must be visible
@pytest.mark.parametrize("C", [2044, 500])
def test_a_lane_that_reads_the_wrong_vector_would_show(C):
    """On the restatement, one 4-channel vector of one pixel of x zeroed -- what a wrong `vok`, G or slot index does to the one lane whose later
    vectors are idle at these widths (C = 2044: NV = 8, lane 63 has seven vectors; C = 500: NV = 2, lane 63 has one) -- moves y, g_x and
    g_weight by more than 100 x the fp32 bound of the GPU test: that test can tell such a defect from rounding."""
    ins, ref, dev = lncf_yardstick(C)
    wrong = RL.value_and_grads(P.zero_one_vector(ins[0], C), *ins[1:], dtype=torch.float64)
    for n in ("y", "g_x", "g_weight"):
        moved, bound = RL.rel_err(wrong[n], ref[n]), 4 * dev[n]
        print("C=%d %-8s moved %.3e  bound %.3e  ratio %.3g" % (C, n, moved, bound, moved / bound))
        assert moved > 100 * bound, (n, moved, bound)


# ================================================================================================================ pw_mlp (csrc/pw_mlp.hip)
def test_the_pw_mlp_list_is_exactly_what_the_host_code_prints():
    """train_plans.EXPECTED_PW against pw_plan over N = 4, 8, ..., 8192 and the four element types, in both directions; every class is a tag the
    launcher can print and pw_tag finds it again"""
    assert len(P.EXPECTED_PW) == len(set(P.EXPECTED_PW)) == 2 * 9 + 2 * 9 + 2 * 8
    assert P.SWEEP_N[0] == 4 and P.SWEEP_N[-1] == P.N_MAX == P.plan_list()[1]["PW_MAX_H"] and len(P.SWEEP_N) == 2048
    listed = {k: v for k, v in P.plan_list()[0].items() if k[0] == "pw_mlp"}
    assert sorted(listed) == sorted(("pw_mlp", "", dt, N) for dt in P.PW_DTYPES for N in P.SWEEP_N)
    printed = _printable("pw_mlp")
    assert printed == set(P.EXPECTED_PW), "printed but not listed: %s; listed but never printed: %s" % (
        sorted(printed - set(P.EXPECTED_PW)), sorted(set(P.EXPECTED_PW) - printed))
    per = {dt: P.pw_classes(dt) for dt in P.PW_DTYPES}
    assert {dt: len(c) for dt, c in per.items()} == {"f32": 9, "f64": 9, "f16": 17, "bf16": 17}
    for dt, classes in per.items():
        for cls, ns in classes.items():
            assert cls.startswith("<%s,V=" % dt) and re.match(r"^<(%s),V=[48]> L=(1|2|4|8|16|32|64|128|256)$" % "|".join(ENAMES), cls), cls
            assert {P.plan_extra("pw_mlp", "", dt, N)["L"] for N in ns} == {P.pw_lanes(cls)}, cls       # the L of the tag is the L of the plan
            for tag, kind in (("pw_mlp act_fwd%s" % cls, "act_fwd"), ("pw_mlp act_bwd%s a=1 gh=0 gb=1" % cls, "act_bwd"), ("pw_mlp colsum%s" % cls, "colsum")):
                assert P.pw_tag(tag) == (kind, cls), tag
    assert P.pw_tag("pw_mlp reduce<f32>") is None and P.pw_tag("lncf_train fwd_cl<f32,V=4,NV=1> G=1 gx=0 gwb=0") is None
    first = P.pw_first_run()
    assert first and set(first) < set(P.EXPECTED_PW) and len(first) == 28, first
    assert "<f32,V=4> L=64" in first and "<f64,V=4> L=256" in first and "<f16,V=8> L=256" in first and "<f32,V=4> L=256" not in first


def test_pw_mlp_spot_facts_of_the_plan():
    f32, f16 = P.pw_classes("f32"), P.pw_classes("f16")
    assert (f32["<f32,V=4> L=8"][0], f32["<f32,V=4> L=8"][-1]) == (20, 8160)
    assert (f32["<f32,V=4> L=256"][0], f32["<f32,V=4> L=256"][-1]) == (996, 8192)
    lanes = (8, 16, 32, 64, 128, 256)
    assert [P.pw_widths("f32", "<f32,V=4> L=%d" % L)[2] for L in lanes] == [68, 164, 356, 740, 1508, 2020]
    assert [P.pw_widths("f16", "<f16,V=8> L=%d" % L)[2] for L in lanes] == [136, 328, 712, 1480, 3016, 4040]
    assert "<f16,V=4> L=2" not in f16 and f16["<f16,V=8> L=1"] == [8] and f16["<f16,V=8> L=2"] == [16]
    for dt in P.PW_DTYPES:
        for N in P.SWEEP_N:
            e = P.plan_extra("pw_mlp", "", dt, N)
            V = 8 if dt in ("f16", "bf16") and N % 8 == 0 else 4
            assert 0 <= e["idle"] <= 7 and e["gx"] * e["L"] - e["idle"] == N // V and (e["gx"] - 1) * e["L"] < N // V, (dt, N, e)
        for cls in P.pw_classes(dt):
            lo, hi, ragged = P.pw_widths(dt, cls)
            assert lo <= ragged <= hi and (ragged == lo) == (P.pw_lanes(cls) < 8 or lo == hi), (cls, lo, hi, ragged)


def test_pw_mlp_rows_make_two_groups_and_a_block_that_loops():
    """Where a group has more than five rows (L <= 32) -- M_short: two groups, five rows in the second; M_loop: 258 groups on 256 rows of
    partials, so blockIdx.y 0 and 1 take two groups each, and the last group has five rows.  With 4, 2 and 1 rows per group the same row counts
    make 3, 4 and 6 groups and 259, 260 and 262: still more than one group, still more groups than rows of partials, and the last group partial
    wherever a group has more than one row.  The largest maps stay small: 1.1 M elements where a lane has four columns, twice that where it
    has eight"""
    rows = P.plan_list()[1]["PW_ROWS"]
    for L in (1, 2, 4, 8, 16, 32, 64, 128, 256):
        rpb = 256 // L
        short, loop = P.pw_rows(L)
        assert (short, loop) == (rpb + 5, 256 * rpb + rpb + 5)
        if rpb > 5:
            assert -(-short // rpb) == 2 and short - rpb == 5
            assert -(-loop // rpb) == rows + 2 and loop - (rows + 1) * rpb == 5
        else:
            assert (-(-short // rpb), -(-loop // rpb)) == {4: (3, 259), 2: (4, 260), 1: (6, 262)}[rpb]
            assert rpb == 1 or (short % rpb and loop % rpb)
        assert 1 < -(-short // rpb) <= rows < -(-loop // rpb) <= 2 * rows
    assert P.pw_rows(1) == (261, 65797) and P.pw_rows(256) == (6, 262)
    for dt in P.PW_DTYPES:
        shapes = P.pw_shapes(dt)
        assert len(shapes) == 3 * len(P.pw_classes(dt))
        for cls, M, N in shapes:
            assert P.predicted("pw_mlp", "", dt, N) == cls and M * N < (2.2e6 if "V=8" in cls else 1.1e6), (cls, M, N)
    assert max(M for _, M, N in P.pw_shapes("f32")) == 65797 and ("<f32,V=4> L=256", 262, 2020) in P.pw_shapes("f32")


@functools.lru_cache(maxsize=None)
def pw_yardstick(M, N):
    """h, grad_a, grad_y drawn for the shape; a, grad_h, g_b1 and the column sums of grad_y in fp64 and the fp32 restatement's deviation"""
    h, ga, gy = RP.draw_maps(M, N, N)
    ref, f32 = RP.act_maps(h.double(), ga.double()), RP.act_maps(h, ga)
    return (h, ga, gy), ref, {n: RP.rel_err(f32[n], ref[n]) for n in ("a", "grad_h", "g_b1")}


def test_pw_mlp_fp32_yardstick_is_positive_at_every_shape_the_gpu_file_runs():
    shapes = sorted({(M, N) for _, M, N in P.pw_shapes("f32")})
    # 27 less the two classes of one width (N = 4, N = 8), whose lo and hi coincide
    assert len(shapes) == 27 - 2 and (8229, 68) in shapes and (65797, 4) in shapes and (262, 2020) in shapes and (37, 8160) in shapes
    for M, N in shapes:
        dev = pw_yardstick(M, N)[2]
        print("M=%5d N=%4d " % (M, N) + "  ".join("%s %.2e" % kv for kv in dev.items()))
        assert all(0 < v < 1e-5 for v in dev.values()), (M, N, dev)


@pytest.mark.parametrize("L,which", [(1, "ragged"), (8, "ragged"), (256, "ragged"), (8, "hi")])
def test_a_pw_mlp_lane_that_skips_a_vector_or_a_group_would_show(L, which):
    """On the restatement: the last V columns of the last row of h zeroed -- what the last lane of the last column tile reads when its `vok`, its
    column or its group stride is wrong -- moves a, grad_h and g_b1, and the last five rows left out of the column sum -- a last group that
    is dropped -- moves g_b1, each by more than 100 x the fp32 bound of the GPU test (4 x the yardstick)."""
    cls = "<f32,V=4> L=%d" % L
    lo, hi, ragged = P.pw_widths("f32", cls)
    M, N = (P.pw_rows(L)[1], ragged) if which == "ragged" else (P.pw_rows(L)[0], hi)
    (h, ga, _), ref, dev = pw_yardstick(M, N)
    wrong_h = h.double().clone()
    wrong_h[-1, -4:] = 0.0
    wrong = RP.act_maps(wrong_h, ga.double())
    short = RP.act_maps(h.double()[:-5], ga.double()[:-5])
    for n, moved in [(n, RP.rel_err(wrong[n], ref[n])) for n in ("a", "grad_h", "g_b1")] + [("g_b1", RP.rel_err(short["g_b1"], ref["g_b1"]))]:
        bound = 4 * dev[n]
        print("%s M=%d N=%d %-7s moved %.3e  bound %.3e  ratio %.3g" % (cls, M, N, n, moved, bound, moved / bound))
        assert moved > 100 * bound, (n, moved, bound)
