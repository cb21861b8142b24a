"""Coverage gate of the SPR search's own arms, on the oracle (CPU): the counters of OMO_BC_SEARCH_LIST (oracle/maple_oracle_bc.h,
counting build only) inside omo_findBestParentTopology and omo_sprWorker, read through omo_search_branch_counts.

What the reference's recorded trees reach: every node slot of the eight tests/golden/search_*.json.gz trees searched under every
recorded parameter set leaves FIXTURE_ZERO at 0 (test_the_recorded_trees_leave_these_arms_at_zero prints the whole table).  The
None merges they do reach (up_bottom, up_vup, up_bottom_late: 8, 30 and 2 hits) are all real ones, mergeVectors returning None on
two lists; no merge of theirs lacks an input list.

What the gadgets of tests/search_trees.py reach: every counter but the UNREACHABLE ones and the *_absent ones, in each of the five
standard modes, without and with a mutation list on the root; each gadget the counters it is named for.  The gadgets' None merges
are real ones as well (every *_absent counter stays at 0): a search that lacks a list is handed to the one-lane kernel by the
frontier tier, which the GPU test must not see.  More than half of their searches end with status 0 and a finite score.

UNREACHABLE, counted and asserted to stay at 0:
  veto_parent       `bestNode == parent` (M:9686).  bestNode is the sibling or the node of a scored item.  Items are seeded at the
                    parent's parent (upwards) and at the sibling (downwards); an upward item pushes its own parent and the child it
                    did not come from, a downward item its children.  An upward item is therefore always a proper ancestor of the
                    parent, and a downward item lies below the sibling or below a child that is not on the path from the parent
                    to the root: no item is ever at the parent itself.
  refine_top_none   midTop None again after the retry with bestTopLength = defaultBLen * 0.1 (M:6798-6802).  mergeVectors returns
                    None where two entries of different nucleotides meet over total lengths that are both 0 (M:4753-4758), or where
                    the product of the two sides' vectors sums to 0.  After the retry the first side's total length is at least
                    defaultBLen * 0.1 > 0; over a positive length every component of its vector is positive (all off-diagonal
                    rates of the five modes' Q are positive), and the other side's vector has a positive component.
"""
import gzip
import json
import os

import numpy as np
import pytest

import list_edges as le
import search_trees as sts
from golden_util import GOLDEN, build_counting_oracle, model_args, read_search_counts, ref_indices
from oracle.oracle_py import Oracle, OracleTree

NAMES = sorted(f[len("search_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("search_") and f.endswith(".json.gz"))
MERGES = ("down_mid", "down_vup", "up_bottom", "up_mid", "up_vup", "up_bottom_late", "refine_lower")
ABSENT = {m + "_absent" for m in MERGES}
UNREACHABLE = {"veto_parent", "refine_top_none"}
# the counters the recorded trees leave at 0 (without the search_ prefix)
FIXTURE_ZERO = ABSENT | UNREACHABLE | {
    "down_mid_none", "down_vup_none", "up_mid_none", "shorten_own", "refine_no_list", "refine_lower_none", "refine_top_retry",
    "refine_newmid_none", "status_minus_1", "veto_chain_top", "veto_sibling", "veto_below_sibling"}
# ... and what the gadgets must leave with at least one hit each, in every mode
MUST = {"veto_chain_top", "veto_sibling", "veto_below_sibling", "refine_no_list", "refine_lower_none", "refine_top_retry",
        "refine_newmid_none", "status_minus_1", "status_2", "down_stop", "up_stop"}


def counts_of(lib):
    return {k[len("search_"):]: v for k, v in read_search_counts(lib).items()}


@pytest.fixture(scope="module")
def counting_lib(tmp_path_factory):
    return build_counting_oracle(tmp_path_factory.mktemp("omo_bc_search"))


def test_the_counters_are_the_listed_ones(counting_lib):
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    names = set(counts_of(o.lib))
    assert len(names) == 35 and FIXTURE_ZERO | MUST <= names
    assert {m + "_none" for m in MERGES} | ABSENT <= names


def test_the_recorded_trees_leave_these_arms_at_zero(counting_lib):
    """A recorded fact, and the reason for tests/test_hip_search_edges.py: a later fixture that reaches one of them shows up here."""
    total, trees = {}, {}
    for name in NAMES:
        with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
            f = json.load(fh)
        ctx, t = f["context"], f["tree"]
        o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
                   thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
                   defaultBLen=ctx["defaultBLen"], lib_path=counting_lib)
        o.set_model(**model_args(f["model"]))
        tree = OracleTree(o, t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"],
                          [t["probVect"], t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"]])
        counts_of(o.lib)
        for rnd in f["spr"]:
            ps = rnd["params"]
            o.spr_worker(tree, np.arange(len(t["up"])), strict=ps["strict"], allowedFails=ps["fails"], thresholdLogLKtopology=ps["thr"],
                         thresholdTopologyPlacement=ps["place"],
                         thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
                         thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
                         effectivelyNon0BLen=ctx["effectivelyNon0BLen"])
        for k, v in counts_of(o.lib).items():
            total[k] = total.get(k, 0) + v
            trees[k] = trees.get(k, 0) + (v > 0)
    print("\narm: hits over the eight recorded trees (trees that reach it)")
    for k, v in total.items():
        print(f"  {k:28s} {v:8d} ({trees[k]})")
    assert len(NAMES) == 8
    assert {k for k, v in total.items() if v == 0} == FIXTURE_ZERO, sorted(k for k, v in total.items() if v == 0)


@pytest.fixture(scope="module")
def on_gadgets(counting_lib):
    """(mode, mat) -> [(gadget, the oracle's result, the counters of its searches)], made once"""
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    cache = {}

    def get(mode, mat):
        if (mode, mat) not in cache:
            o.set_model(**le.model(mode))
            res = []
            for g in sts.gadgets(o, mode, mat):
                counts_of(o.lib)
                out = o.spr_worker(g.tree.oracle_tree(o), g.nodes, **g.params)
                res.append((g, out, counts_of(o.lib)))
            cache[(mode, mat)] = res
        return cache[(mode, mat)]
    return get


@pytest.mark.parametrize("mat", [False, True], ids=["plain", "root_mutations"])
@pytest.mark.parametrize("mode", le.MODES[:5])
def test_gadgets_reach_the_arms_they_are_named_for(on_gadgets, mode, mat):
    res = on_gadgets(mode, mat)
    u = bool(le.model(mode).get("usingErrorRate"))
    total = {}
    print(f"\n{mode}, {'with' if mat else 'without'} a mutation list on the root: hits per gadget")
    for g, out, counts in res:
        print(f"  {g.name:24s}", {k: v for k, v in counts.items() if v})
        assert 5 <= g.tree.n <= 15 and (not mat or g.tree.mutations[g.tree.root])
        for gl in g.tree.lists():
            le.check_grammar(gl, le.L_REF, u)
        for k in g.reach:
            assert counts[k] > 0, (g.name, k, counts)
        if g.handback == (None, None):                                       # (no list of its searches is shortened to another one)
            assert counts["shorten_own"] == 0 and counts["shorten_passed"] == 0, (g.name, counts)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    zero = {k for k, v in total.items() if v == 0}
    assert zero == ABSENT | UNREACHABLE, sorted(zero ^ (ABSENT | UNREACHABLE))
    assert all(total[k] > 0 for k in MUST)
    assert len({g.name for g, _, _ in res}) == len(res)


@pytest.mark.parametrize("mode", le.MODES[:5])
def test_most_gadget_searches_still_find_a_placement(on_gadgets, mode):
    """so that the corpus does not degenerate into failures: status 0 with a finite bestScore for at least half the searches"""
    status, score = [], []
    for mat in (False, True):
        for g, out, _ in on_gadgets(mode, mat):
            status += out["status"].tolist()
            score += out["bestScore"].tolist()
    good = sum(s == 0 and np.isfinite(x) for s, x in zip(status, score))
    print(f"{mode}: {good} of {len(status)} searches end with status 0 and a finite score; statuses {sorted(set(status))}")
    assert 2 * good >= len(status) and {0, -1, 2} <= set(status)


def test_stop_here_is_what_the_search_computes(counting_lib):
    """handed(), which the "stop here" lists are made of, against the search itself: with probVectTotUp of a node set to the list
    handed() gives, the search stops updating exactly there; with one of its lengths moved it does not."""
    o = Oracle(le.reference(), le.ROOT_FREQS, lib_path=counting_lib)
    o.set_model(**le.model("unrest"))
    t = sts.frame(o, sts.leaf_lists(False, 5))
    for v in range(t.n):
        t.totUp[v] = None if t.totUp[v] is None else sts.ALL_N             # (no stop by the tree's own lists)
    counts_of(o.lib)
    o.spr_worker(t.oracle_tree(o), [t.mark["v"]], **sts.PARAMS)
    base = counts_of(o.lib)
    assert base["down_stop"] == 0 and base["up_stop"] == 0
    sts.stop_at(o, t, "v", "up", "G")
    o.spr_worker(t.oracle_tree(o), [t.mark["v"]], **sts.PARAMS)
    got = counts_of(o.lib)
    assert got["up_stop"] == 1 and got["down_stop"] == 0 and got["root_cross_cached"] == 1 and got["root_cross_updating"] == 0
