"""The oracle twin of maple_tree_log_lk and maple_tree_find_best_root (tests/sink_trees.py) and the trees it is given, on the CPU.

The twin is pinned to the unmodified reference's records on every search_* fixture, with the tolerances the GPU tests give the
library against those same records (test_hip_tree_lk.py, test_hip_root_search.py): 1e-12 on the root term, 1e-11 on the tree's
log-likelihood, 1e-7 on the kept scores of findBestRoot (the reference shortens upVect in place at M:7819, which moves what is
computed below; the twin does not).

Coverage gate, with the counting build of the oracle (-DOMO_BRANCH_COUNTS), on the six counters of the arms that
tests/test_hip_sink_edges.py is about:
  merge_carry, merge_underflow                       mergeVectors' carry-over into the logarithm and its underflow (M:4830-4839)
  rootprob_carry                                      findProbRoot's carry-over
  rootprob_flag_R, rootprob_flag_nuc_global / _site   findProbRoot on flagged R runs and nucleotides (M:4876-4883)
The recurrences of both calls leave all six at 0 on every fixture; the gadget trees reach every one that the mode can reach.  None
of the six is out of reach of a valid tree.  What a mode cannot reach: the three flag counters without an error model (the flag
element only exists under one), rootprob_flag_nuc_global with site-specific error rates and rootprob_flag_nuc_site without (the
two are the arms of one `if`).

Conditions on the inputs, by the oracle alone, so that no GPU test can pass by scoring nothing: the carry families' trees score
both of their sides (16 of 16, 12 of 12, 16 of 16 per mode), merge_underflow's none (0 of 12), sink_abandon's exactly the
intended ones, each abandoned where it is meant to be.
"""
import gzip
import json
import os

import numpy as np
import pytest

import list_edges as le
import sink_trees as st
from golden_util import GOLDEN, build_counting_oracle, close, model_args, read_counts, ref_indices
from oracle.oracle_py import Oracle
from sink_trees import MODELS

NAMES = sorted(f[len("search_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("search_") and f.endswith(".json.gz"))
SIX = ("merge_carry", "merge_underflow", "rootprob_carry", "rootprob_flag_R", "rootprob_flag_nuc_global", "rootprob_flag_nuc_site")


def load(kind, name):
    with gzip.open(os.path.join(GOLDEN, f"{kind}_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


def fixture_oracle(f, lib_path=None):
    ctx = f["context"]
    o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
               thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
               defaultBLen=ctx["defaultBLen"], lib_path=lib_path)
    o.set_model(**model_args(f["model"]))
    return o


@pytest.fixture(scope="module")
def counting_lib(tmp_path_factory):
    return build_counting_oracle(tmp_path_factory.mktemp("omo_bc_sink"))


@pytest.fixture(scope="module")
def on_fixtures(counting_lib):
    """name -> (fixture, its tree, the twin's tree log-likelihood, the twin's scores, the counters after both), made once"""
    cache = {}

    def get(name):
        if name not in cache:
            f = load("search", name)
            o = fixture_oracle(f, counting_lib)
            t = st.fixture_columns(f)
            read_counts(o.lib)
            lk = st.oracle_tree_lk(o, t)
            why = {}
            scores = st.oracle_root_scores(o, t, why=why)
            cache[name] = (f, t, lk, scores, why, read_counts(o.lib))
        return cache[name]
    return get


@pytest.mark.parametrize("name", NAMES)
def test_twin_tree_lk_matches_the_reference(on_fixtures, name):
    f, t, (order, contrib, root_term), _, _, _ = on_fixtures(name)
    assert len(order) >= 50
    total = 0.0
    for x in contrib:
        total += x
    total += root_term
    print(f"{name}: twin {total!r} root {root_term!r}; reference {f['treeLK']!r} root {f['rootLK']!r}")
    assert close(root_term, f["rootLK"], 1e-12), (root_term, f["rootLK"])
    assert close(total, f["treeLK"], 1e-11), (total, f["treeLK"])


@pytest.mark.parametrize("name", NAMES)
def test_twin_root_scores_match_the_reference(on_fixtures, name):
    f, t, _, scores, why, _ = on_fixtures(name)
    recs = load("update", name)["find_best_root"]
    assert len(recs) == 2 and not why                                       # (nothing is abandoned on the fixtures)
    below = []                                                               # every branch below the root's children is scored
    stack = [(c, 1) for c in t.children[t.root]]
    while stack:
        v, d = stack.pop()
        if d >= 2:
            below.append(v)
        stack += [(c, d + 1) for c in t.children[v]]
    assert sorted(scores) == sorted(below) and len(below) > 100
    for rec in recs:
        ref = {int(k): v for k, v in rec["bestNodes"].items()}
        assert ref.pop(t.root) == 0.0 and len(ref) > 50
        assert set(ref) <= set(scores)
        worst = max(abs(scores[k][0] - x) / max(1e-7, 1e-7 * max(abs(x), abs(scores[k][0]))) for k, x in ref.items())
        print(f"{name}: {len(ref)} kept scores, largest deviation over the bound {worst:.3g}")
        assert all(close(scores[k][0], x, 1e-7, 1e-7) for k, x in ref.items())


def test_the_fixtures_pass_lists_through_mutation_lists():
    """what the two tests above rely on for the twin's pass-up and pass-down paths"""
    root_mat = child_mat = False
    for name in NAMES:
        t = load("search", name)["tree"]
        root_mat |= bool(t["mutations"][t["root"]])
        child_mat |= any(m for v, m in enumerate(t["mutations"]) if v != t["root"] and t["children"][v])
    assert root_mat and child_mat


def test_the_fixtures_leave_the_six_counters_at_zero(on_fixtures):
    """A recorded fact, and the reason for tests/test_hip_sink_edges.py: if a future fixture reaches one of them, this says so and
    the counter can leave the list."""
    for name in NAMES:
        counts = on_fixtures(name)[5]
        assert {k: counts[k] for k in SIX} == {k: 0 for k in SIX}, name


@pytest.fixture(scope="module")
def on_gadgets(counting_lib):
    """model name -> {family: (cases, trees, [(scores, why)], counters)} over the five-node trees, made once"""
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    cache = {}

    def get(name):
        if name not in cache:
            mode, kw = MODELS[name]
            o.set_model(**kw)
            corp = le.corpus(mode)
            out = {}
            for fam in st.GADGET_FAMS:
                if fam not in corp:
                    continue
                trees = st.family_gadgets(o, corp, fam)
                read_counts(o.lib)
                res = []
                for t in trees:
                    why = {}
                    res.append((st.oracle_root_scores(o, t, why=why), why))
                out[fam] = (corp[fam], trees, res, read_counts(o.lib))
            cache[name] = out
        return cache[name]
    return get


@pytest.mark.parametrize("name", list(MODELS))
def test_gadgets_reach_every_counter_the_mode_can_reach(on_gadgets, name):
    fams = on_gadgets(name)
    kw = MODELS[name][1]
    u, ss = bool(kw.get("usingErrorRate")), kw.get("errorRates") is not None
    assert set(fams) == set(st.GADGET_FAMS) - (set() if u else {"sink_flag"})
    print(name, {fam: {k: v[3][k] for k in SIX} for fam, v in fams.items()})
    for fam in st.CARRY_FAMS:
        counts = fams[fam][3]
        assert counts["merge_carry"] > 50 and counts["rootprob_carry"] >= 4 and counts["merge_underflow"] == 0, (fam, counts)
    for fam in ("merge_underflow", "sink_abandon"):
        counts = fams[fam][3]
        assert counts["merge_underflow"] >= 6 and counts["merge_carry"] == 0, (fam, counts)
    for fam, v in fams.items():
        reach = u and fam == "sink_flag"
        want = {"rootprob_flag_R": reach, "rootprob_flag_nuc_global": reach and not ss, "rootprob_flag_nuc_site": reach and ss}
        for k, yes in want.items():
            assert (v[3][k] > 500) if yes else (v[3][k] == 0), (fam, k, v[3][k])
    if u:
        # (on flagged factors: over the stretch where upVect is N nothing else multiplies logFactor, and its 550 to 700 flagged
        # nucleotides at about 0.25 each take it below minimumCarryOver = 2.2e-258 at least once per rooting)
        assert fams["sink_flag"][3]["rootprob_carry"] >= 8


@pytest.mark.parametrize("name", list(MODELS))
def test_gadgets_score_what_they_are_meant_to(on_gadgets, name):
    fams = on_gadgets(name)
    u = bool(MODELS[name][1].get("usingErrorRate"))
    expected = {"merge_carry": (16, 16), "long": (12, 12), "append_carry": (16, 16), "merge_underflow": (0, 12), "sink_flag": (8, 8),
                "sink_abandon": (2, 12)}
    worst = 0.0
    for fam, (cases, trees, res, _) in fams.items():
        scored = total = 0
        for c, t, (scores, why) in zip(cases, trees, res):
            sides = st.gadget_sides(t)
            scored += sum(v in scores for v in sides)
            total += 2
            assert not (set(scores) & set(why)) and all(np.isfinite(s[0]) for s in scores.values())
            for v, (sc, terms) in scores.items():
                if v in sides and sc != 0.0:
                    worst = max(worst, sum(abs(x) for x in terms) / abs(sc))
            for key, gl in c.items():
                if isinstance(gl, list) and gl and isinstance(gl[0], tuple):
                    le.check_grammar(gl, le.L_REF, u)
            for gl in t.probVect:
                le.check_grammar(gl, le.L_REF, u)
            if fam == "sink_abandon":
                for key, v in zip(("k0", "k1"), sides):
                    assert why.get(v, "scored") == c["expect"][key], (c["name"], key, why.get(v))
                    assert (v in scores) == (c["expect"][key] == "scored")
                    assert t.children[v] and all((w in scores) == (v in scores) for w in t.children[v])      # what is below
        assert (scored, total) == expected[fam], (fam, scored, total)
    reasons = {w for _, _, res, _ in [fams["sink_abandon"]] for _, why in res for w in why.values()}
    assert reasons == {"up_underflow", "up_none", "new_underflow", "new_none"}
    print(f"{name}: on k0 and k1 the four terms' magnitudes sum to up to {worst:.3g} times the score")
    assert worst > 100.0                                                     # (why the GPU test's bound is on the terms)


def test_root_gadget_branch_lengths_add_up_exactly():
    o = Oracle(le.reference(), le.ROOT_FREQS)
    o.set_model(**le.model("unrest"))
    corp = le.corpus("unrest")
    for fam in st.GADGET_FAMS:
        if fam not in corp:
            continue
        for c, t in zip(corp[fam], st.family_gadgets(o, corp, fam)):
            p = c if "k0" in c else st.as_pair(c)
            m = t.mark
            assert t.dist[m["c1"]] + t.dist[m["c2"]] == p["b2"] and t.dist[m["k1"]] == p["b1"]
            assert t.probVect[m["k1"]] == p["pv1"] and t.probVect[m["c2"]] == p["pv2"]
            assert t.children[t.root] == [m["c1"], m["c2"]] and t.children[m["c1"]] == [m["k0"], m["k1"]]
            assert (not t.children[m["k1"]]) == p["tip1"] and (not t.children[m["c2"]]) == p["tip2"]


@pytest.mark.parametrize("name", ["unrest", "siteerr"])
def test_the_larger_trees_are_what_the_gpu_tests_take_them_for(counting_lib, name):
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    mode, kw = MODELS[name]
    o.set_model(**kw)
    corp = le.corpus(mode)
    comb = st.standard_comb(o, corp)
    read_counts(o.lib)
    order, contrib, _ = st.oracle_tree_lk(o, comb)
    counts = read_counts(o.lib)
    assert counts["merge_carry"] > 300 and counts["merge_underflow"] == 0
    assert st.oracle_tree_lk(o, comb, known=comb.mark["contrib"])[1] == contrib          # the builder's values are the twin's
    assert len(comb.mark["cherry"]) == st.N_COMB and len(order) > 3 * 256 and len(order) % 64 != 0
    assert [v for v in order if v in {c[0] for c in comb.mark["cherry"]}] == [c[0] for c in comb.mark["cherry"]]
    assert any(comb.n_minor) and all(np.isfinite(contrib))
    bad = st.underflow_comb(o, corp)
    first, second = (bad.mark["cherry"][k][0] for k in st.UNDERFLOW_AT)
    order = st.lk_order(bad)
    assert order.index(first) < order.index(second) and first > second
    with pytest.raises(RuntimeError):
        st.oracle_tree_lk(o, bad)
    read_counts(o.lib)
    deep = st.deep_gadget(o, corp)
    scores = st.oracle_root_scores(o, deep)
    assert len(st.level_sizes(deep)) >= 4 and min(len(deep.probVect[v]) for v in deep.mark["inner"]) > 300
    assert all(v in scores for v in deep.mark["inner"][1:]) and read_counts(o.lib)["merge_carry"] > 20
    wide = st.gadget_grove(o, corp)
    assert len(wide.mark["roots"]) >= 40 and max(st.level_sizes(wide)) > 32 and len(st.oracle_root_scores(o, wide)) >= 300
