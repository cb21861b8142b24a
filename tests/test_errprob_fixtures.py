"""The committed fixtures of the error report (tests/golden/errprob_*.json.gz, errprob_arms.json) are what the GPU tests take them
for, and maple_amd.ops.format_error_report writes the reference's text from them.  No GPU."""
import hashlib

import pytest

import em_util
import errprob_util as eu

NAMES = eu.fixture_names()


def test_the_expected_fixtures_are_there():
    assert NAMES == sorted(["cat_a_gerr", "cat_a_full", "cat_a_gerr_gtr", "cat_b_gerr", "cat_b_full", "cat_zero_gerr", "cat_zero_full",
                            "synth_siteerr", "example_siteerr", "synth_gtr_err"])


@pytest.mark.parametrize("name", NAMES)
def test_fixture_is_consistent(name):
    fx = eu.load(name)
    assert fx["em"] in em_util.fixture_names()                           # the tree it belongs to is committed
    em = eu.em_of(fx)
    assert em["model"]["usingErrorRate"]
    tree = em["tree"]
    order = eu.dfs_leaves(tree)
    assert [r["minErrorProb"] for r in fx["thresholds"]] == list(eu.THRESHOLDS)
    assert [len(m) for m in fx["minorIds"]] == tree["nMinor"] and len(fx["nodeName"]) == tree["n"]
    for rec in fx["thresholds"]:
        thr = rec["minErrorProb"]
        assert rec["leaves"] == order                                    # the reference's depth-first order
        assert len(rec["records"]) == len(order)
        for v, rl in zip(rec["leaves"], rec["records"]):
            if tree["nMinor"][v] > 0:
                assert rl == []                                          # M:9805-9807
            pos = [p for p, _, _ in rl]
            assert pos == sorted(set(pos)) and all(1 <= p <= em["context"]["lRef"] for p in pos)
            assert all(0 <= a <= 4 for _, a, _ in rl)
            for _, _, x in rl:
                assert x >= thr
                assert thr == 0.0 or abs(x - thr) > eu.MARGIN * thr      # a last-bit difference cannot move a record across it
    at0, at_half = fx["thresholds"][0]["records"], fx["thresholds"][2]["records"]
    assert at_half == [[r for r in rl if r[2] >= 0.5] for rl in at0]
    assert fx["thresholds"][1]["records"] == [[r for r in rl if r[2] >= 0.01] for rl in at0]
    assert sum(len(rl) for rl in at0) > 0


def test_every_arm_is_reached():
    a = eu.arms()
    assert len(a["arms"]) == 74 and a["unreached"] == [] and a["reached"] == a["arms"]
    assert all(a["range"][0] <= x <= a["range"][1] for x in a["arms"])
    seen = set()
    for name in NAMES:
        seen.update(eu.load(name)["lines"])
    assert set(a["arms"]) <= seen
    cats = set()
    for name in NAMES:
        if name.startswith("cat_"):
            cats.update(eu.load(name)["lines"])
    assert set(a["arms"]) <= cats                                        # the caterpillar fixtures alone reach them all


def test_zero_div_fixture():
    fx = eu.load("zero_div")
    assert "ZeroDivisionError" in fx["raised"]
    t, m = fx["tree"], fx["model"]
    assert m["usingErrorRate"] and m["errorRateGlobal"] == 0.0 and not m["errorRateSiteSpecific"]
    assert sum(1 for c in t["children"] if not c) == 3
    v = fx["node"]
    assert not t["children"][v] and t["dist"][v] == 0.0
    p = t["up"][v]
    upper = t["probVectUpRight"][p] if t["children"][p][0] == v else t["probVectUpLeft"][p]
    assert [len(e) for e in upper] == [2]                                # the reference everywhere, no lengths


@pytest.mark.parametrize("name", NAMES)
def test_format_error_report_is_the_references_text(name):
    """The text format: the recorded records through format_error_report hash to what the reference wrote."""
    from maple_amd.ops import format_error_report
    fx = eu.load(name)
    for rec in fx["thresholds"]:
        text = format_error_report(*eu.arrays(rec), fx["minorIds"], fx["nodeName"], fx["namesInTree"])
        assert hashlib.sha256(text.encode()).hexdigest() == rec["sha256"], (name, rec["minErrorProb"])
