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
