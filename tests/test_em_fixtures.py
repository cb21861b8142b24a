"""The EM fixtures (tests/golden/em_*.json.gz) reach every arm of the reference's walk and maximisation: the union of the
reference lines their recorded calls executed covers every arm-opening line of M:10168-10790 and M:10855-10946
(tests/golden/em_arms.json, written by make_golden_em.py from the reference's syntax tree: the first line of every if / elif /
else / loop body, without bodies that only raise -- a call that raises returns nothing to record; em_cat_a_ratevar_negq records
one such call -- and without bodies under trackMutations, which is out of scope), but for at most three arms named there as
unreachable, each with its reason."""
import em_util


def test_every_arm_is_reached():
    a = em_util.arms()
    assert len(a["arms"]) > 200 and all(any(lo <= x <= hi for lo, hi in a["ranges"]) for x in a["arms"])
    seen = set()
    for name in em_util.fixture_names():
        seen.update(em_util.load(name)["lines"])
    unreachable = {u["line"]: u["reason"] for u in a["unreachable"]}
    assert len(unreachable) <= 3 and all(isinstance(r, str) and len(r) > 20 and "\n" not in r for r in unreachable.values())
    missed = [x for x in a["arms"] if x not in seen and x not in unreachable]
    assert not missed, f"arms no fixture reaches: {missed}"
    assert not [x for x in unreachable if x in seen], "an arm listed as unreachable is reached"


def test_cases_the_issue_names_are_present():
    names = set(em_util.fixture_names())
    for ref_tree in ("synth_unrest", "synth_siteerr", "example_siteerr", "synth_gtr_err", "synth_ratevar"):
        assert ref_tree in names
    for tree in ("cat_a", "cat_b", "cat_zero"):
        for mode in ("plain", "ratevar", "gerr", "full"):
            assert f"{tree}_{mode}" in names
    for name in names:
        fx = em_util.load(name)
        assert (fx["raised"] is None) == ("ret" in fx)
        if "ret" in fx:
            m = fx["model"]
            assert (fx["ret"]["siteRates"] is None) == (not m["useRateVariation"])
            assert (fx["ret"]["errorRate"] is None) == (not m["usingErrorRate"])
            assert (fx["ret"]["siteErrRates"] is None) == (not m["errorRateSiteSpecific"])
    assert "lkAfterOneRound" in em_util.load("synth_unrest") and "lkAfterOneRound" in em_util.load("synth_ratevar")
