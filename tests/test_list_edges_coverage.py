"""Coverage gate on the oracle (CPU): the adversarial corpus of tests/list_edges.py must reach every rarely taken operator
branch that oracle/maple_oracle.c and oracle/maple_oracle_search.c count when built with -DOMO_BRANCH_COUNTS (the counters are
listed in oracle/maple_oracle_bc.h).  The GPU tests of test_hip_list_edges.py and test_hip_struct_edges.py compare the kernels
with the oracle on the same corpus, so a branch the corpus stops reaching would silently drop out of them.

Not counted, because valid inputs cannot reach it: mergeVectors(isUpDown) with an O vector against N on the FIRST side and a
total length of 0 (oracle `else memcpy(newVec, e1->vec ...)` after `if (isUpDown && ((e1->len == 4 && e1->d0 > 0) || bLen1
!= 0.0))`, M:4647-4656): the condition asks for d0 > 0 or bLen1 != 0, and the sum of two non-negative branch lengths of
which one is not 0 is not 0.  Nor the length-3 error-model entry of M:4515-4516, marked unreachable in the reference.

Counted, and asserted to stay at 0 (UNREACHABLE), because valid inputs cannot reach them:
  rootprob_minus_inf  findProbRoot's exit through -inf (M:4905-4907).  The running product is reset to 1 whenever it is at most
                      minimumCarryOver = DBL_MIN * 1e50, and one step multiplies it by sum(rootFreqs[i] * vec[i]) of a
                      normalised O vector or by rootFreqs[i] * (1 - 1.33333 e) + 0.33333 e of a flagged nucleotide: at least
                      min(rootFreqs) (1 - 1.33333 e), far above 1e-50.  No step takes it from above minimumCarryOver to below
                      DBL_MIN.
  minor_end_both      isMinorSequence's `return 0` after the loop (M:5996-5998).  found1bigger and found2bigger are tested
                      together at the end of every step, the last one included, before the loop is left (M:5977-5978).
"""
import numpy as np
import pytest

import list_edges as le
import sink_trees as st
from golden_util import build_counting_oracle, fixture_names, load, model_args, read_counts, ref_indices, tup
from oracle.oracle_py import Oracle

# the counters the recorded golden calls (tests/golden/calls_*.json.gz) leave at 0
GOLDEN_ZERO = {"append_R_d1_O", "append_nuc_d1_O", "append_carry3", "merge_carry", "merge_underflow", "merge_updown_N_err_d0",
               "blen_none_R_d1", "blen_none_R_flag", "blen_none_nuc_d1", "blen_early_tenth", "evalplace_top_fallback"}
# ... and of the structural operators (the fixtures record no isMinorSequence call at all)
GOLDEN_ZERO |= {
    "differ_O_d0", "differ_O_zero", "differ_d1", "differ_flag4", "differ_flag5",
    "minor_N_R", "minor_N_site", "minor_O1_big", "minor_O1_small", "minor_O2_big", "minor_O2_small",
    "minor_OO_found1", "minor_OO_found2", "minor_OO_identical_diff", "minor_OO_identical_same",
    "minor_R_N", "minor_early_both", "minor_end_1_bigger", "minor_end_2_bigger", "minor_end_both",
    "minor_end_equal", "minor_identical_type", "minor_nuc_mismatch", "minor_site_N",
    "pass_down_O_mut_d0", "pass_down_R_mut_adjacent", "pass_down_mut_at_1", "pass_down_mut_at_lRef",
    "pass_up_N_skip_many", "pass_up_R_mut_adjacent", "pass_up_R_tail_len5", "pass_up_mut_at_1",
    "pass_up_mut_at_lRef",
    "rootprob_carry", "rootprob_flag_R", "rootprob_flag_nuc_global", "rootprob_flag_nuc_site",
    "rootprob_minus_inf",
    "rootvec_O_len_d0", "rootvec_O_zero_d0",
    "shorten_head_near_neighbour_far", "shorten_refuse_head_far"}
UNREACHABLE = {"rootprob_minus_inf", "minor_end_both"}
PLAIN_ONLY = {"shorten_absorb_len3", "pass_down_R_tail_len3", "pass_up_R_tail_len3", "rootvec_plain_tail", "rootvec_plain_blen",
              "rootvec_plain_bare"}                                # tuple forms and arms that exist only without an error model
ERR_ONLY = {"shorten_absorb_len5", "shorten_refuse_flag", "pass_down_R_tail_len5", "pass_up_R_tail_len5", "differ_flag4",
            "differ_flag5", "rootvec_err_tail", "rootvec_err_blen", "rootvec_err_bare", "rootprob_flag_R"}
STRUCT_PREFIX = {"shorten_runs": ("shorten_",), "pass_edges": ("pass_",), "differ_edges": ("differ_",), "rootvec": ("rootvec_",),
                 "rootprob": ("rootprob_",), "minor": ("minor_",)}


@pytest.fixture(scope="module")
def counting_lib(tmp_path_factory):
    return build_counting_oracle(tmp_path_factory.mktemp("omo_bc"))


def run_case(o, fam, c):
    """One corpus case through the oracle; the merge underflow is fatal (the reference raises)."""
    if fam.startswith("sink"):                                         # a five-node tree through the root search (test_sink_trees.py)
        return st.oracle_root_scores(o, st.root_gadget(o, c))
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


def run_struct_case(o, fam, c):
    """One case of the structural families through the oracle (both modes of isMinorSequence)."""
    if fam == "shorten_runs":
        return o.shorten(c["vec"])
    if fam.startswith("pass"):
        return o.passGenomeListThroughBranch(c["pv"], c["mutations"], c["dirIsUp"])
    if fam == "differ_edges":
        return o.areVectorsDifferent(c["pv1"], c["pv2"])
    if fam == "rootvec":
        return o.rootVector(c["pv"], c["bLen"], c["isFromTip"], c["path"])
    if fam == "rootprob":
        return o.findProbRoot(c["pv"], [])
    return [o.isMinorSequence(c["pv1"], c["pv2"], f) for f in (False, True)]


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
    for mode in le.WITNESS_MODES:
        qs, cs = le.witness_corpus(mode)
        for gl in qs + [c for c in cs if c is not None]:
            le.check_grammar(gl, le.L_REF, False)
    for mode in le.MODES[:5]:
        u = bool(le.model(mode).get("usingErrorRate"))
        for fam, cases in le.struct_corpus(mode).items():
            assert len(cases) <= 240, (fam, len(cases))
            for c in cases:
                for k, v in c.items():
                    if k in ("mutations", "path"):                 # mutation lists: sorted, positions unique and inside the genome
                        for ml in ([v] if k == "mutations" else v):
                            ps = [m[0] for m in ml]
                            assert ps == sorted(set(ps)) and all(1 <= p <= le.L_REF for p in ps), (fam, c["name"])
                            assert all(0 <= m[1] < 4 and 0 <= m[2] < 4 and m[1] != m[2] for m in ml)
                    elif isinstance(v, list) and v and isinstance(v[0], tuple):
                        le.check_grammar(v, le.L_REF, u)


def test_struct_corpus_reaches_every_counted_branch(counting_lib):
    """Every counter of the six structural operators is reached by its own family in every standard mode that can reach it;
    the two that valid inputs cannot reach stay at 0.  The families also give both answers of areVectorsDifferent (the window
    cases with the answer they are built to have), all three of isMinorSequence, and lists that shorten changes and leaves."""
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    read_counts(o.lib)
    for mode in le.MODES[:5]:
        m = le.model(mode)
        u, ss = bool(m.get("usingErrorRate")), m.get("errorRates") is not None
        o.set_model(**m)
        corp = le.struct_corpus(mode)
        assert set(corp) == set(le.STRUCT_FAMILIES)
        counts = {}
        for fam, cases in corp.items():
            res = [run_struct_case(o, fam, c) for c in cases]
            counts[fam] = read_counts(o.lib)
            if fam == "differ_edges":
                assert all(c["expect"] is None or c["expect"] == r for c, r in zip(cases, res))
                assert sum(c["expect"] is not None for c in cases) > 50 and {True, False} == set(res)
            elif fam == "minor":
                assert {r[0] for r in res} == {0, 1, 2} and {r[1] for r in res} == {0, 1}
            elif fam == "shorten_runs":
                changed = [r != c["vec"] for c, r in zip(cases, res)]
                assert any(changed) and not all(changed)
        for fam, prefixes in STRUCT_PREFIX.items():
            got = dict(counts[fam])
            for k, v in got.items():
                if not k.startswith(prefixes):
                    continue
                cannot = (k in UNREACHABLE or (u and k in PLAIN_ONLY) or (not u and k in ERR_ONLY)
                          or k == ("rootprob_flag_nuc_global" if (ss or not u) else "rootprob_flag_nuc_site")
                          or (not u and k == "rootprob_flag_nuc_site"))
                assert (v == 0) if cannot else (v > 0), (mode, fam, k, v)


def test_run_head_rule_and_fold_change_window():
    """The two inputs that tell a subtly wrong implementation from a right one, with the answers written out."""
    o = Oracle(le.reference(), le.ROOT_FREQS)
    L = le.L_REF
    a, thr = 1e-4, le.THR
    for mode in ("unrest", "gerr"):
        o.set_model(**le.model(mode))
        tail = (lambda d: (d, False)) if o.u else (lambda d: (d,))
        run = lambda ds: [(4, 10)] + [(4, 11 + k) + tail(d) for k, d in enumerate(ds)] + [(4, L)]     # noqa: E731
        far = o.shorten(run([a, a + 0.8 * thr, a + 1.6 * thr]))
        assert far == [(4, 10), (4, 12) + tail(a + 0.8 * thr), (4, 13) + tail(a + 1.6 * thr), (4, L)]   # two kept, not one
        assert o.shorten(run([a, a + 0.8 * thr, a])) == [(4, 10), (4, 13) + tail(a), (4, L)]
        for x, y, want in le.WINDOW:
            v1, v2 = le.o_pair(np.random.default_rng(0), x, y, 2)
            assert o.areVectorsDifferent([(4, 5), (6, 1, v1), (4, L)], [(4, 5), (6, 1, v2), (4, L)]) == want, (x, y)


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
    structural = tuple(x for pre in STRUCT_PREFIX.values() for x in pre)      # (test_struct_corpus_reaches_every_counted_branch)
    assert len([k for k in total if not k.startswith(structural)]) == 12
    missing = sorted(k for k, v in total.items() if v == 0 and not k.startswith(structural))
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
        Q = f["models"][0]["Q"]
        for fn in ("passGenomeListThroughBranch", "shorten", "areVectorsDifferent"):
            for r in f["calls"][fn]:
                o.set_model(Q, usingErrorRate=bool(r["usingErrorRate"]), errorRateGlobal=1e-4)
                if fn == "passGenomeListThroughBranch":
                    o.passGenomeListThroughBranch(tup(r["pv"]), r["mutations"], r["dirIsUp"])
                elif fn == "shorten":
                    o.shorten(tup(r["vec"]))
                else:
                    o.areVectorsDifferent(tup(r["pv1"]), tup(r["pv2"]))
        for fn in ("rootVector", "findProbRoot"):
            for r in f["calls"][fn]:
                o.set_model(**model_args(f["models"][r["model"]]))
                if fn == "rootVector":
                    o.rootVector(tup(r["pv"]), r["bLen"] or 0.0, r["isFromTip"], r["pathMutations"])
                else:
                    o.findProbRoot(tup(r["pv"]), r["pathMutations"])
        got = read_counts(o.lib)
        total = got if total is None else {k: total[k] + got[k] for k in got}
    zero = {k for k, v in total.items() if v == 0}
    print("\ngolden calls leave at 0:", sorted(zero))
    assert zero == GOLDEN_ZERO, (sorted(zero), total)


# ---- the corpus of the whole-tree searches' score rows (witness filter, maple_amd/csrc/witness.hip) ------------------------------
@pytest.fixture(scope="module")
def witness_ref():
    """mode -> (queries, candidates, the rule's answer per pair, its arm counts, the oracle's scores per isTipC), made once."""
    o = Oracle(le.reference(), le.ROOT_FREQS)
    cache = {}

    def get(mode):
        if mode not in cache:
            o.set_model(**le.model(mode))
            qs, cs = le.witness_corpus(mode)
            counts = {}
            excl = le.witness_matrix(qs, cs, counts)
            cache[mode] = (qs, cs, excl, counts, {tip: le.oracle_rows(o, qs, cs, tip, 0.0) for tip in (False, True)})
        return cache[mode]
    return get


@pytest.mark.parametrize("mode", le.WITNESS_MODES)
def test_witness_rule_is_sound_against_the_oracle(witness_ref, mode):
    """The proof in witness.hip's header, tested: a pair the rule may leave out scores -inf by the oracle, over a removed branch
    of length 0, for both values of isTipC -- and the rule that takes an entry WITH a stored length for one without is caught."""
    qs, cs, excl, counts, want = witness_ref(mode)
    for tip in (False, True):
        bad = excl & np.isfinite(want[tip])
        assert not bad.any(), (mode, tip, np.argwhere(bad)[:5])
    rq, rc = le.witness_family_ranges(mode)["wit_sites"]
    wrong = 0
    for q in rq:
        arm = le.witness_arms(qs[q], lengthless=lambda e: True)    # (the mutant: d0 ignored)
        for k in rc:
            if any(arm[p] != x for p, x in le.witness_eligible(cs[k])) and np.isfinite(want[False][q, k]):
                wrong += 1
    assert wrong > 0


@pytest.mark.parametrize("mode", le.WITNESS_MODES)
def test_witness_corpus_reaches_every_arm(witness_ref, mode):
    qs, cs, excl, counts, want = witness_ref(mode)
    assert set(le.witness_families(mode)) == set(le.WITNESS_FAMILIES)
    assert 180 <= len(cs) <= 220 and len(cs) % 64 != 0 and 130 <= len(qs) <= 170, (len(qs), len(cs))
    for arm in le.ARMS + ("no_eligible",):                         # every arm of wit_ranges, and bucket 0
        assert counts.get(arm, 0) > 0, (mode, arm, counts)
    elig = [le.witness_eligible(c) if c is not None else [] for c in cs]
    assert sum(c is None for c in cs) >= 2 and sum(c is not None and not e for c, e in zip(cs, elig)) >= 8
    sites = {p for e in elig for p, _ in e}
    assert {1, 2, le.L_REF - 1, le.L_REF} <= sites                 # the first and the last bucket of a nucleotide
    only = [e[0] for e in elig if len(e) == 1]                     # candidates whose bucket is known without the histogram
    assert len(only) > len(set(only))                              # ... two of them in one bucket
    assert any(len(e) > 1 for e in elig)
    ne = [len(q) for q in qs]
    assert max(ne) > 512 and [(5, le.L_REF)] in qs and [(4, le.L_REF)] in qs
    arms = [le.witness_arms(q) for q in qs]
    assert max(int((a[1:] == 5).sum()) for a in arms if not (a[1:] == 5).all()) > 400     # an N run over hundreds of buckets


@pytest.mark.parametrize("mode", le.WITNESS_MODES)
def test_witness_corpus_is_balanced(witness_ref, mode):
    """Conditions on the inputs, by the oracle alone: every family has pairs of both outcomes, a quarter of all pairs are finite,
    a quarter may be left out by the rule, and at least 20 are -inf without any witness saying so (they must be walked, and
    their bit must stay clear)."""
    qs, cs, excl, counts, want = witness_ref(mode)
    for tip in (False, True):
        fin = np.isfinite(want[tip])
        for fam, (rq, rc) in le.witness_family_ranges(mode).items():
            if fam == "wit_query_extremes":
                continue
            sub = fin[np.ix_(list(rq), list(rc))]
            assert sub.any() and not sub.all(), (mode, fam)
        assert fin.mean() >= 0.25, (mode, fin.mean())
        assert excl.mean() >= 0.25, (mode, excl.mean())
        assert int((~fin & ~excl).sum()) >= 20
        assert not np.isnan(want[tip]).any() and not np.isposinf(want[tip]).any()
