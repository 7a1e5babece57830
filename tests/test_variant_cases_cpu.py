"""Consistency of the variant -> parity-case table (tests/variant_cases.py) without a GPU: unique tags, entry points that exist, bounds that
refer to an existing test, a CTX_ONLY list limited to the launchers that have no context-free entry point, and -- for the stacked-sample and
row-remapped GEMM cases -- that a leak across samples or rows would be visible at the case's shape."""
import glob
import os
import re

import pytest
import torch
import torch.nn.functional as F

import variant_cases as vc

TESTS = os.path.dirname(os.path.abspath(__file__))


def test_tags_are_unique():
    tags = [c["tag"] for c in vc.CASE_LIST]
    dup = sorted({t for t in tags if tags.count(t) > 1})
    assert not dup, dup
    assert len(vc.CASES) == len(vc.CASE_LIST)


def test_every_case_names_a_declared_entry_point_and_a_reference():
    from unicorn_amd._lib import PROTOS
    for c in vc.CASE_LIST:
        assert c["entry"] in PROTOS, (c["tag"], c["entry"])
        assert c["ref"] and "fp64" in c["ref"], c["tag"]


def test_every_bound_is_restated_from_an_existing_test():
    defined = set()
    for path in glob.glob(os.path.join(TESTS, "test_*.py")):
        defined |= set(re.findall(r"^def (test_\w+)\(", open(path).read(), re.M))
    for c in vc.CASE_LIST:
        assert c["bound_from"] in defined, (c["tag"], c["bound_from"])
        assert 0 < c["bound"] < 0.1, c["tag"]


def test_ctx_only_is_limited_to_launchers_without_a_context_free_entry_point():
    defined = set()
    for path in glob.glob(os.path.join(TESTS, "test_*.py")):
        defined |= set(re.findall(r"^def (test_\w+)\(", open(path).read(), re.M))
    for pat, reason, test in vc.CTX_ONLY:
        assert pat.startswith("^") and pat[1:].startswith(vc.CTX_ONLY_ALLOWED), pat
        assert reason and test in defined, (pat, test)
        assert "gemm:" not in pat, "GEMM tags have a context-free entry for every switch (uni_gemm_stacked): %s" % pat
        if pat.startswith("^msda_fused"):   # fp32 has uni_msda_tokens
            assert "f32" not in pat, pat
    for c in vc.CASE_LIST:
        assert not vc.ctx_only_match(c["tag"]), "a tag with a parity case is also parked in CTX_ONLY: %s" % c["tag"]


def test_trace_text_round_trip():
    assert vc.parse_trace("a b=1\t3\nc\t1\n") == {"a b=1": 3, "c": 1}
    assert vc.parse_trace("") == {}


# ------------------------------------------------------------------------------------------------ a leak must be visible at the case's shape
def _leaks(a, P):
    """{name: (leaky value, correct value, tolerance)}: what a kernel that ignores the sample boundaries or the remap would produce"""
    Hin, Win, Cin, N, k, stride, pad = a["geo"]
    B, G, M = a["B"], a["G"], P["M"]
    out = {}
    raw_tall = None
    if k > 1 and B > 1:      # halos across samples: the samples stacked into one tall (B * Hin, Win) image (stride 1, "same" padding: M rows again)
        tall = P["x"].double().permute(1, 0, 2, 3).reshape(1, Cin, B * Hin, Win)
        raw_tall = P["rows"](F.conv2d(tall, P["w"].double(), P["bias"].double() if a["bias"] else None, stride=stride, padding=pad))
        assert raw_tall.shape == P["raw"].shape
        if a["outF"] or a["outB"]:
            out["outputs of the tall-image conv"] = (P["finish"](raw_tall), P["exp"], P["tol"])
    if G and B > 1:
        if raw_tall is not None:
            out["sums of the tall-image conv"] = (P["stats"](raw_tall), P["stats_ref"], P["stats_tol"])
        out["sums over the whole batch in every slot"] = (P["stats_ref"].sum(0, keepdim=True).expand(B, G, 2), P["stats_ref"], P["stats_tol"])
        out["sums over samples shifted by one row"] = (P["stats"](P["raw"], 1), P["stats_ref"], P["stats_tol"])
    if B > 1 and a["splitk"]:      # the reduce kernel's grid is (cdiv(Mper, 8), B): sample b addressed at b * 8 cdiv(Mper, 8) instead of b * Mper
        m = torch.arange(M)
        src = (m + (m // P["Mper"]) * (-P["Mper"] % 8)).clamp(max=M - 1)
        out["reduce rows addressed by the block grid"] = (P["finish"](P["raw"][src]), P["exp"], P["tol"])
    if a["out_hw"]:          # the output rows without the remap, seen through the remap (rows the unmapped launch never writes hold the fill)
        buf = torch.full((max(a["outF_rows"], M), N), -777.0, dtype=torch.float64)
        buf[:M] = P["exp"]
        out["outF without the remap"] = (buf[P["orow"]], P["exp"], P["tol"])
    return out


@pytest.mark.parametrize("tag", [c["tag"] for c in vc.STACKED])
def test_stacked_gemm_case_would_show_a_leak(tag):
    """Every stacked-sample / row-remapped GEMM case, in fp64 on the CPU: the correct reference against the references of a kernel that leaks
    -- 3x3 halos taken from the neighbouring sample, statistics summed over the whole batch or over samples shifted by one row, outF rows
    written without the remap, and for the K-range cases the reduce kernel addressing sample b by its block grid (8-row blocks, ragged per
    sample) instead of b * Mper.  Each leak must move at least one element or statistics value by more than 100x the tolerance the GPU test
    applies there, or the case could not tell the defect from rounding.  Plain 1x1 cases have no halo, so the tall-image variant does not exist
    for them; every case must still have at least one leak that applies to it."""
    case = vc.CASES[tag]
    a = case["args"]
    assert a["B"] > 1 or a["out_hw"], "neither stacked nor remapped"
    P = vc.gemm_stacked_problem(a, case["bound"])
    assert P["M"] == a["B"] * P["Mper"]
    if a["out_hw"]:          # the case's own remap arguments satisfy the entry's rule, and the remapped rows are distinct
        assert P["M"] % a["out_hw"] == 0 and int(P["orow"].max()) < a["outF_rows"] and len(set(P["orow"].tolist())) == P["M"]
        assert (P["M"] // a["out_hw"] - 1) * a["out_stride"] + a["out_off"] + a["out_hw"] <= a["outF_rows"]
    leaks = _leaks(a, P)
    assert leaks, "no leak applies to this case: it checks nothing the one-sample case does not"
    for name, (bad, good, tol) in leaks.items():
        ratio = ((bad - good).abs() / tol).max().item()
        print("%s: %s: max |leaky - correct| / tolerance %.3g" % (tag, name, ratio))
        assert ratio > 100.0, (name, ratio)
