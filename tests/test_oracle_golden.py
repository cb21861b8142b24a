"""Pin the C oracle to the golden call records harvested from the unmodified reference.

Every record in tests/golden/calls_*.json.gz is (arguments, resolved model, value returned by
MAPLEv0.7.5.4.py).  Integer structure (types, positions, tuple lengths, flags) must match
bit-for-bit; floats within 1e-12 relative (the oracle keeps the reference's operand order, so in
practice they are identical to the last bit apart from libm's log()).
"""
import math

import pytest

from golden_util import close, fixture_names, lists_match, load, model_args, ref_indices, tup
from oracle.oracle_py import Oracle

REL = 1e-12
FIXTURES = fixture_names()


def make_oracle(fx):
    ctx = fx["context"]
    return Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                  minBLenSensitivity=ctx["minBLenSensitivity"],
                  thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                  thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"])


def by_model(fx, fn):
    groups = {}
    for rec in fx["calls"][fn]:
        groups.setdefault(rec["model"], []).append(rec)
    return groups


@pytest.fixture(scope="module", params=FIXTURES)
def fx(request):
    f = load(request.param)
    return f, make_oracle(f)


def test_fixtures_present():
    assert len(FIXTURES) >= 5


def test_appendProbNode(fx):
    f, o = fx
    n = 0
    for mid, recs in by_model(f, "appendProbNode").items():
        o.set_model(**model_args(f["models"][mid]))
        for r in recs:
            got = o.appendProbNode(tup(r["P"]), tup(r["C"]), r["isTipC"], r["bLen"])
            want = r["ret"]
            assert close(got, want, REL), (got, want)
            n += 1
    assert n > 100


def test_mergeVectors(fx):
    f, o = fx
    n = 0
    for mid, recs in by_model(f, "mergeVectors").items():
        o.set_model(**model_args(f["models"][mid]))
        for r in recs:
            if r.get("raised"):
                continue
            got = o.mergeVectors(tup(r["pv1"]), r["b1"], r["tip1"], tup(r["pv2"]), r["b2"], r["tip2"],
                                 returnLK=r["returnLK"], isUpDown=r["isUpDown"], numMinor1=r["numMinor1"],
                                 numMinor2=r["numMinor2"])
            want = r["ret"]
            if r["returnLK"]:
                assert lists_match(got[0], tup(want[0]), REL)
                assert close(got[1], want[1], REL), (got[1], want[1])
            else:
                assert lists_match(got, tup(want), REL), (got, want)
            n += 1
    assert n > 100


def test_estimateBranchLength(fx):
    f, o = fx
    for mid, recs in by_model(f, "estimateBranchLengthWithDerivative").items():
        o.set_model(**model_args(f["models"][mid]))
        for r in recs:
            got = o.estimateBranchLengthWithDerivative(tup(r["P"]), tup(r["C"]), r["fromTipC"])
            want = r["ret"]
            if want is False:
                assert got is False
            else:
                assert got is not False and close(got, want, REL), (got, want)


def test_evaluatePlacement(fx):
    f, o = fx
    for mid, recs in by_model(f, "evaluatePlacement").items():
        o.set_model(**model_args(f["models"][mid]))
        for r in recs:
            got = o.evaluatePlacement(tup(r["midTot"]), tup(r["downVect"]), tup(r["upVect"]), r["distance"],
                                      tup(r["removedPartials"]), r["isRemovedTip"], r["fromTip1"])
            want = [0.0 if w is False else w for w in r["ret"]]
            for g, w in zip(got, want):
                assert close(g, w, 1e-10), (got, want)


def test_rootVector(fx):
    f, o = fx
    for mid, recs in by_model(f, "rootVector").items():
        o.set_model(**model_args(f["models"][mid]))
        for r in recs:
            got = o.rootVector(tup(r["pv"]), r["bLen"], r["isFromTip"], r["pathMutations"])
            assert lists_match(got, tup(r["ret"]), REL), (got, r["ret"])


def test_findProbRoot(fx):
    f, o = fx
    n = 0
    for mid, recs in by_model(f, "findProbRoot").items():
        o.set_model(**model_args(f["models"][mid]))
        for r in recs:
            assert close(o.findProbRoot(tup(r["pv"]), r["pathMutations"]), r["ret"], REL), r["ret"]
            n += 1
    assert n > 30


def _u_groups(f, fn):
    g = {}
    for rec in f["calls"][fn]:
        g.setdefault(bool(rec["usingErrorRate"]), []).append(rec)
    return g


def test_structural_functions(fx):
    f, o = fx
    Q = f["models"][0]["Q"]
    for u, recs in _u_groups(f, "passGenomeListThroughBranch").items():
        o.set_model(Q, usingErrorRate=u, errorRateGlobal=1e-4)
        for r in recs:
            got = o.passGenomeListThroughBranch(tup(r["pv"]), r["mutations"], r["dirIsUp"])
            assert lists_match(got, tup(r["ret"]), 0.0)
    for u, recs in _u_groups(f, "shorten").items():
        o.set_model(Q, usingErrorRate=u, errorRateGlobal=1e-4)
        for r in recs:
            assert lists_match(o.shorten(tup(r["vec"])), tup(r["ret"]), 0.0)
    for u, recs in _u_groups(f, "areVectorsDifferent").items():
        o.set_model(Q, usingErrorRate=u, errorRateGlobal=1e-4)
        for r in recs:
            assert o.areVectorsDifferent(tup(r["pv1"]), tup(r["pv2"])) == r["ret"]


def test_getPartialVec_and_simplify(fx):
    f, o = fx
    Q = f["models"][0]["Q"]
    for u, recs in _u_groups(f, "getPartialVec").items():
        o.set_model(Q, usingErrorRate=u, errorRateGlobal=1e-4)
        for r in recs:
            got = o.getPartialVec(r["i12"], r["totLen"], r["mutMatrix"], r["errorRate"], r["vect"], r["upNode"],
                                  r["flag"])
            assert all(close(g, w, REL, 0.0) for g, w in zip(got, r["ret"])), (got, r["ret"])
    o.set_model(Q)
    for r in f["calls"]["simplify"]:
        assert o.simplify(r["vec"], r["refA"]) == r["ret"]
