"""Pin the oracle's SPR search (oracle/maple_oracle_search.c) to the reference's own records of
startTopologyUpdatesParallel / findBestParentTopology on a frozen tree (tests/golden/search_*.json.gz)."""
import gzip
import json
import os

import pytest

from golden_util import GOLDEN, close, lists_match, model_args, ref_indices, tup
from oracle.oracle_py import Oracle, OracleTree

NAMES = sorted(f[len("search_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("search_") and f.endswith(".json.gz"))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_spr_search_matches_reference(name):
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        f = json.load(fh)
    ctx, t = f["context"], f["tree"]
    o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
               minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
               thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"])
    o.set_model(**model_args(f["model"]))
    tree = OracleTree(o, t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"],
                      [t["probVect"], t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"]])
    for rnd in f["spr"]:
        ps, calls = rnd["params"], rnd["calls"]
        nodes = [t["children"][c["node"]][c["child"]] for c in calls]
        out = o.spr_worker(tree, nodes, strict=ps["strict"], allowedFails=ps["fails"], thresholdLogLKtopology=ps["thr"],
                           thresholdTopologyPlacement=ps["place"],
                           thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
                           thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
                           effectivelyNon0BLen=ctx["effectivelyNon0BLen"], want_removed_partials=True)
        for k, c in enumerate(calls):
            want = c["ret"]
            assert out["status"][k] == 0
            assert close(float(out["currentLK"][k]), c["bestLKdiff"], 1e-12)
            assert int(out["bestNode"][k]) == want["bestNode"], (k, out["bestNode"][k], want["bestNode"])
            assert close(float(out["bestScore"][k]), want["bestScore"], 1e-9)
            wb = [0.0 if b is False else b for b in want["bestBranchLengths"]]
            assert all(close(float(g), w, 1e-8, 1e-15) for g, w in zip(out["blen"][k], wb))
            assert int(out["nAppend"][k]) == c["n_append"], (k, out["nAppend"][k], c["n_append"])
            assert lists_match(out["removedPartials"][k], tup(want["bestRemovedPartials"]), 1e-9)
        got = sorted((nodes[k], int(out["placement"][k])) for k in range(len(nodes)) if out["placement"][k] >= 0)
        assert got == sorted((m[0], m[1]) for m in rnd["proposedMoves"])


@pytest.mark.parametrize("name", NAMES[:3])
def test_packed_lists_to_oracle_entries_c_equals_numpy(name):
    """The oracle library's converter of packed lists (omo_entries_from_packed, used for whole trees of 10^8 entries) against
    the numpy conversion and against to_entries() of the tuple form, on every list of a reference tree."""
    import numpy as np
    from maple_amd.genome_list import pack_lists
    from oracle.oracle_py import packed_to_entries, packed_to_entries_numpy, to_entries
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        f = json.load(fh)
    t, u = f["tree"], bool(f["model"]["usingErrorRate"])
    lists = [tup(gl) for kind in ("probVect", "probVectUpRight", "probVectUpLeft", "probVectTotUp") for gl in t[kind] if gl]
    pk = pack_lists(lists, u)
    a, off = packed_to_entries(pk, u, threads=3)
    b, off2 = packed_to_entries_numpy(pk, u)
    assert np.array_equal(off, off2) and a.tobytes() == b.tobytes()
    want = np.concatenate([to_entries(gl, u) for gl in lists[:400]])
    assert a[: len(want)].tobytes() == want.tobytes()


def check_placements(name):
    """findBestParentForNewSample (M:7912-8292): the oracle against the reference's own records of every placement query
    on the frozen tree (node, nAppend and bestDiffs exact; score 1e-9; branch lengths 1e-8; None exactly where the
    reference returns it).  Both exits occur: minor sequences (M:7971-8008) and real placements with the refinement."""
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        f = json.load(fh)
    ctx, t = f["context"], f["tree"]
    o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
               minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
               thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"])
    o.set_model(**model_args(f["model"]))
    tree = OracleTree(o, t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"],
                      [t["probVect"], t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"]])
    only_identical = any(x in f["flags"] for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    pkw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
               thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
               thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
               allowedFails=ctx["allowedFails"], strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical)
    n_real = n_minor = 0
    for k, rec in enumerate(f["placements"]):
        status, node, score, blens, best_diffs, n_append = o.find_best_parent_for_new_sample(tree, tup(rec["query"]), **pkw)
        want = rec["ret"]
        assert node == want["bestNode"], (k, node, want["bestNode"])
        assert n_append == rec["n_append"], (k, n_append, rec["n_append"])
        assert close(score, want["bestScore"], 1e-9), (k, score, want["bestScore"])
        if want["bestBranchLengths"] is None:
            assert status == 1 and blens is None, (k, status, blens)
            n_minor += 1
        else:
            assert status == 0 and blens is not None, (k, status)
            wb = [0.0 if b is False else b for b in want["bestBranchLengths"]]
            assert all(close(g, w, 1e-8, 1e-15) for g, w in zip(blens, wb)), (k, blens, wb)
            n_real += 1
        assert lists_match(best_diffs, tup(want["bestDiffs"]), 0.0), (k, best_diffs, want["bestDiffs"])
    assert n_real + n_minor == len(f["placements"]) >= 40
    assert n_real > 20
    return n_real, n_minor


@pytest.mark.parametrize("name", NAMES)
def test_oracle_placement_search_matches_reference(name):
    check_placements(name)


def test_oracle_placement_search_sees_both_exits():
    """Across the fixtures the records hold minor sequences as well as real placements, and the oracle meets both."""
    got = [check_placements(name) for name in NAMES]
    n_real, n_minor = sum(g[0] for g in got), sum(g[1] for g in got)
    assert n_real + n_minor == 440 and n_minor >= 5 and n_real >= 300, (n_real, n_minor)


def test_oracle_tree_updated_in_place():
    """OracleTree.update: a tree whose mid-branch lists were wrong for a third of the branches, and whose last two nodes were not
    there yet, brought up to date in place (the new lists appended behind the others, only those nodes' start/len rewritten):
    the placement records of the reference again, every other list where it was."""
    import numpy as np
    name = NAMES[0]
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        f = json.load(fh)
    ctx, t = f["context"], f["tree"]
    o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
               minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
               thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"])
    o.set_model(**model_args(f["model"]))
    n = len(t["up"])
    have = [v for v in range(n) if t["probVectTotUp"][v]]
    wrong = have[::3]
    tot = list(t["probVectTotUp"])
    for i, v in enumerate(wrong):                                # (another branch's mid-branch list)
        tot[v] = t["probVectTotUp"][wrong[(i + len(wrong) // 2) % len(wrong)]]
    # the tree without its last two nodes' lists, and with the wrong mid-branch lists
    kinds = [list(t["probVect"]), list(t["probVectUpRight"]), list(t["probVectUpLeft"]), tot]
    late = [n - 2, n - 1]
    for k in range(4):
        for v in late:
            kinds[k][v] = None
    tree = OracleTree(o, t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], kinds, headroom=64)
    start_before = [s.copy() for s in tree.start]
    n_ent = tree.n_ent
    only_identical = any(x in f["flags"] for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    pkw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
               thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
               thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
               allowedFails=ctx["allowedFails"], strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical)
    n_stale = 0
    for rec in f["placements"]:
        try:
            r = o.find_best_parent_for_new_sample(tree, tup(rec["query"]), **pkw)
            n_stale += r[1] != rec["ret"]["bestNode"] or not close(r[2], rec["ret"]["bestScore"], 1e-9)
        except RuntimeError:                                      # (the reference would raise on such a tree too)
            n_stale += 1
    assert n_stale > 5, n_stale
    fix = {v: t["probVectTotUp"][v] for v in wrong + late}
    others = [{v: t[kind][v] for v in late} for kind in ("probVect", "probVectUpRight", "probVectUpLeft")]
    children = np.asarray([c if c else [-1, -1] for c in t["children"]])
    up = [-1 if x is None else x for x in t["up"]]
    tree.update(o, t["root"], up, children, t["dist"], t["nMinor"], others + [fix])
    assert tree.n_ent > n_ent
    keep = np.setdiff1d(np.arange(n), wrong + late)
    for k in range(4):
        kk = keep if k == 3 else np.setdiff1d(np.arange(n), late)
        assert np.array_equal(tree.start[k][kk], start_before[k][kk]), k
    for k, rec in enumerate(f["placements"]):
        status, node, score, blens, _, n_append = o.find_best_parent_for_new_sample(tree, tup(rec["query"]), **pkw)
        assert node == rec["ret"]["bestNode"] and n_append == rec["n_append"], k
        assert close(score, rec["ret"]["bestScore"], 1e-9), k
