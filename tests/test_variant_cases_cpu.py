"""Consistency of the variant -> parity-case table (tests/variant_cases.py) without a GPU: unique tags, entry points that exist, bounds that
refer to an existing test, and a CTX_ONLY list limited to the launchers that have no context-free entry point."""
import glob
import os
import re

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
        if pat.startswith("^gemm:"):        # GEMM tags only with the row-remap or the stacked-sample switch set
            assert "remap=1" in pat or "stacked=1" in pat, pat
        if pat.startswith("^msda_fused"):   # fp32 has uni_msda_tokens
            assert "f32" not in pat, pat
    for c in vc.CASE_LIST:
        assert not vc.ctx_only_match(c["tag"]), "a tag with a parity case is also parked in CTX_ONLY: %s" % c["tag"]


def test_trace_text_round_trip():
    assert vc.parse_trace("a b=1\t3\nc\t1\n") == {"a b=1": 3, "c": 1}
    assert vc.parse_trace("") == {}
