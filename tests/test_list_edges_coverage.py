"""Coverage gate on the oracle (CPU): the adversarial corpus of tests/list_edges.py must reach every rarely taken operator
branch that oracle/maple_oracle.c counts when built with -DOMO_BRANCH_COUNTS.  The GPU tests of test_hip_list_edges.py
compare the kernels with the oracle on the same corpus, so a branch the corpus stops reaching would silently drop out of
them.

Not counted, because valid inputs cannot reach it: mergeVectors(isUpDown) with an O vector against N on the FIRST side and a
total length of 0 (oracle `else memcpy(newVec, e1->vec ...)` after `if (isUpDown && ((e1->len == 4 && e1->d0 > 0) || bLen1
!= 0.0))`, M:4647-4656): the condition asks for d0 > 0 or bLen1 != 0, and the sum of two non-negative branch lengths of
which one is not 0 is not 0.  Nor the length-3 error-model entry of M:4515-4516, marked unreachable in the reference.
"""
import ctypes as C
import os
import subprocess

import pytest

import list_edges as le
from golden_util import fixture_names, load, model_args, ref_indices, tup
from oracle.oracle_py import HERE, Oracle

# the counters the recorded golden calls (tests/golden/calls_*.json.gz) leave at 0
GOLDEN_ZERO = {"append_R_d1_O", "append_nuc_d1_O", "append_carry3", "merge_carry", "merge_underflow", "merge_updown_N_err_d0",
               "blen_none_R_d1", "blen_none_R_flag", "blen_none_nuc_d1", "blen_early_tenth", "evalplace_top_fallback"}


@pytest.fixture(scope="module")
def counting_lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("omo_bc") / "libmaple_oracle_bc.so")
    subprocess.check_call(["gcc", "-O2", "-std=c11", "-ffp-contract=off", "-fPIC", "-fopenmp", "-DOMO_BRANCH_COUNTS", "-shared",
                           os.path.join(HERE, "maple_oracle.c"), os.path.join(HERE, "maple_oracle_search.c"), "-o", out, "-lm"])
    return out


def read_counts(lib, reset=True):
    n = lib.omo_branch_counts(None, None, 0, 0)
    vals = (C.c_longlong * n)()
    names = (C.c_char_p * n)()
    lib.omo_branch_counts(vals, names, n, int(reset))
    return {names[k].decode(): int(vals[k]) for k in range(n)}


def run_case(o, fam, c):
    """One corpus case through the oracle; the merge underflow is fatal (the reference raises)."""
    if fam.startswith("append") or fam in ("skip_edges", "long"):
        return o.appendProbNode(c["P"], c["C"], c["isTipC"], c["bLen"])
    if fam.startswith("merge"):
        try:
            return o.mergeVectors(c["pv1"], c["b1"], c["tip1"], c["pv2"], c["b2"], c["tip2"], returnLK=c["returnLK"],
                                  isUpDown=c["isUpDown"])
        except RuntimeError:
            assert fam == "merge_underflow"
            return "fatal"
    if fam.startswith("blen"):
        return o.estimateBranchLengthWithDerivative(c["P"], c["C"], c["fromTipC"])
    return o.evaluatePlacement(c["midTot"], c["down"], c["up"], c["distance"], c["rem"], c["isRemovedTip"], c["fromTip1"])


def test_corpus_follows_the_grammar():
    for mode in le.MODES:
        u = bool(le.model(mode).get("usingErrorRate"))
        for fam, cases in le.corpus(mode).items():
            for c in cases:
                for k, v in c.items():
                    if isinstance(v, list) and v and isinstance(v[0], tuple):
                        le.check_grammar(v, le.L_REF, u)
        qs, cs = le.dense_lists(mode) if not mode.startswith("zeroq") else ([], [])
        for gl in qs + cs:
            le.check_grammar(gl, le.L_REF, u)


def test_corpus_reaches_every_counted_branch(counting_lib):
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    read_counts(o.lib)
    per_family = {}
    for mode in le.MODES:
        o.set_model(**le.model(mode))
        for fam, cases in le.corpus(mode).items():
            for c in cases:
                run_case(o, fam, c)
            got = read_counts(o.lib)
            for k, v in got.items():
                per_family.setdefault(k, {}).setdefault(f"{fam}/{mode}", 0)
                per_family[k][f"{fam}/{mode}"] += v
    total = {k: sum(v.values()) for k, v in per_family.items()}
    print("\ncorpus branch counts:", total)
    missing = sorted(k for k, v in total.items() if v == 0)
    assert not missing, f"the corpus no longer reaches {missing}"
    # each family reaches its own branch in every mode that can reach it
    aims = {"append_R_d1_O": "append_d1_O", "append_nuc_d1_O": "append_d1_O", "append_carry3": "append_carry",
            "merge_carry": "merge_carry", "merge_underflow": "merge_underflow", "merge_updown_N_O_zero": "merge_updown",
            "blen_early_tenth": "blen_tenth", "evalplace_top_fallback": "evalplace_fallback"}
    for counter, fam in aims.items():
        for mode in le.MODES[:5]:
            assert per_family[counter].get(f"{fam}/{mode}", 0) > 0, (counter, fam, mode)
    for mode in ("gerr", "siteerr"):
        assert per_family["merge_updown_N_err_d0"].get(f"merge_updown/{mode}", 0) > 0, mode
    assert per_family["blen_none_R_d1"].get("blen_none/zeroq", 0) > 0 and per_family["blen_none_nuc_d1"].get("blen_none/zeroq", 0) > 0
    assert all(per_family[k].get("blen_none/zeroq_err", 0) > 0 for k in ("blen_none_R_d1", "blen_none_R_flag", "blen_none_nuc_d1"))


def test_golden_calls_leave_these_branches_at_zero(counting_lib):
    """What the recorded calls of the reference reach of the same counters: the gap the corpus closes."""
    total = None
    for name in fixture_names():
        f = load(name)
        ctx = f["context"]
        o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                   minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                   thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"],
                   lib_path=counting_lib)
        read_counts(o.lib)
        for fn in ("appendProbNode", "mergeVectors", "estimateBranchLengthWithDerivative", "evaluatePlacement"):
            for r in f["calls"][fn]:
                if r.get("raised"):
                    continue
                o.set_model(**model_args(f["models"][r["model"]]))
                if fn == "appendProbNode":
                    o.appendProbNode(tup(r["P"]), tup(r["C"]), r["isTipC"], r["bLen"])
                elif fn == "mergeVectors":
                    o.mergeVectors(tup(r["pv1"]), r["b1"], r["tip1"], tup(r["pv2"]), r["b2"], r["tip2"], returnLK=r["returnLK"],
                                   isUpDown=r["isUpDown"], numMinor1=r["numMinor1"], numMinor2=r["numMinor2"])
                elif fn == "estimateBranchLengthWithDerivative":
                    o.estimateBranchLengthWithDerivative(tup(r["P"]), tup(r["C"]), r["fromTipC"])
                else:
                    o.evaluatePlacement(tup(r["midTot"]), tup(r["downVect"]), tup(r["upVect"]), r["distance"],
                                        tup(r["removedPartials"]), r["isRemovedTip"], r["fromTip1"])
        got = read_counts(o.lib)
        total = got if total is None else {k: total[k] + got[k] for k in got}
    zero = {k for k, v in total.items() if v == 0}
    print("\ngolden calls leave at 0:", sorted(zero))
    assert zero == GOLDEN_ZERO, (sorted(zero), total)
