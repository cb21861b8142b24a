"""GPU parity of the device-resident SPR search against records of the
reference's own startTopologyUpdatesParallel / findBestParentTopology run on a frozen tree
(tests/golden/search_*.json.gz, made by tests/golden/make_golden_search.py).

Bar: node ids, proposed moves and the number of candidate placements scored (appendProbNode calls)
bit-exact; scores / branch lengths within 1e-8 relative (the reference shortens shared lists in place
while it searches, which moves later results at the 1e-12 level).
"""
import gzip
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, close, lists_match, model_args, ref_indices, tup

pytestmark = pytest.mark.gpu
NAMES = sorted(f[len("search_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("search_") and f.endswith(".json.gz"))


def load(name):
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


@pytest.fixture(scope="module", params=NAMES)
def env(request):
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree
    f = load(request.param)
    ctx, t = f["context"], f["tree"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                 minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                 thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"],
                 arena_bytes=256 << 20)
    dev.set_model(**model_args(f["model"]))
    tree = HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"],
                    t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
    yield f, dev, tree
    dev.close()


def load_update(name):
    path = os.path.join(GOLDEN, f"update_{name}.json.gz")
    if not os.path.exists(path):
        pytest.skip(f"no update records for {name}")
    with gzip.open(path, "rt") as fh:
        return json.load(fh)


UPDATE_NAMES = sorted(f[len("update_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("update_"))


def test_fixture_present():
    assert NAMES and UPDATE_NAMES


def test_spr_search_matches_reference(env):
    f, dev, tree = env
    ctx = f["context"]
    for rnd in f["spr"]:
        ps = rnd["params"]
        calls = rnd["calls"]
        # the pruned node of each recorded findBestParentTopology(tree, node, child, ...) call
        nodes = [tree.children[c["node"]][c["child"]] for c in calls]
        out = dev.spr_search_batch(nodes, strict=ps["strict"], allowedFails=ps["fails"],
                                   thresholdLogLKtopology=ps["thr"], thresholdTopologyPlacement=ps["place"],
                                   thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
                                   thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
                                   effectivelyNon0BLen=ctx["effectivelyNon0BLen"], want_removed_partials=True)
        rpr = dev.download(out["removedPartials"])
        n_total = 0
        for k, c in enumerate(calls):
            assert out["status"][k] == 0, (k, out["status"][k])
            assert close(float(out["currentLK"][k]), c["bestLKdiff"], 1e-9)
            want = c["ret"]
            assert want is not None
            assert int(out["bestNode"][k]) == want["bestNode"], (k, out["bestNode"][k], want["bestNode"])
            assert close(float(out["bestScore"][k]), want["bestScore"], 1e-8), (out["bestScore"][k], want["bestScore"])
            wb = [0.0 if b is False else b for b in want["bestBranchLengths"]]
            assert all(close(float(g), w, 1e-7, 1e-15) for g, w in zip(out["blen"][k], wb)), (out["blen"][k], wb)
            assert int(out["nAppend"][k]) == c["n_append"], (k, out["nAppend"][k], c["n_append"])
            assert lists_match(rpr[k], tup(want["bestRemovedPartials"]), 1e-7), (rpr[k], want["bestRemovedPartials"])
            n_total += c["n_append"]
        assert n_total > 1000
        # a13: the proposed moves (node, placement, improvement)
        got_moves = sorted((nodes[k], int(out["placement"][k]), float(out["improvement"][k]))
                           for k in range(len(nodes)) if out["placement"][k] >= 0)
        want_moves = sorted(tuple(m) for m in rnd["proposedMoves"])
        assert [(m[0], m[1]) for m in got_moves] == [(m[0], m[1]) for m in want_moves]
        assert all(close(g[2], w[2], 1e-7) for g, w in zip(got_moves, want_moves))


def test_nodes_not_searched(env):
    """Nodes the reference's worker skips (root; zero-length branch with a good current cost) report why."""
    f, dev, tree = env
    ctx = f["context"]
    ps = f["spr"][0]["params"]
    searched = {tree.children[c["node"]][c["child"]] for c in f["spr"][0]["calls"]}
    others = [v for v in tree.preorder() if v not in searched]
    out = dev.spr_search_batch(others, strict=ps["strict"], allowedFails=ps["fails"], thresholdLogLKtopology=ps["thr"],
                               thresholdTopologyPlacement=ps["place"],
                               thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
                               thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
                               effectivelyNon0BLen=ctx["effectivelyNon0BLen"])
    for v, st in zip(others, out["status"]):
        assert st == (1 if tree.up[v] is None else 2), (v, st)
    assert (out["placement"] == -1).all()


@pytest.mark.parametrize("path", ["native", "host_replay"])
def test_placement_search_matches_reference(env, path):
    """a12: findBestParentForNewSample on the frozen tree for 60 new samples, one query per call: the native call
    (GPU scoring + the traversal function on the host) and the Python replay over the same all-branch scores."""
    from maple_amd.search import PlacementParams, PlacementSearcher
    f, dev, tree = env
    ctx = f["context"]
    any_err = f["model"]["usingErrorRate"]
    flags = f["flags"]
    only_identical = any(x in flags for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    ps = PlacementSearcher(dev, tree, PlacementParams(
        oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
        thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
        thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
        allowedFails=ctx["allowedFails"], strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical))
    n_real = 0
    search = ps.find_best_parent_for_new_sample if path == "native" else ps.find_best_parent_host_replay
    for rec in f["placements"]:
        node, score, blens, best_diffs, info = search(tup(rec["query"]))
        want = rec["ret"]
        assert node == want["bestNode"], (node, want["bestNode"])
        assert close(score, want["bestScore"], 1e-9), (score, want["bestScore"])
        if want["bestBranchLengths"] is None:
            assert blens is None
        else:
            wb = [0.0 if b is False else b for b in want["bestBranchLengths"]]
            gb = [0.0 if b is False else b for b in blens]
            assert all(close(g, w, 1e-8, 1e-15) for g, w in zip(gb, wb)), (gb, wb)
            assert info["n_append"] == rec["n_append"], (info["n_append"], rec["n_append"])
            n_real += 1
        assert lists_match(best_diffs, tup(want["bestDiffs"]), 0.0), (best_diffs, want["bestDiffs"])
    assert n_real > 20


def test_batched_placement_matches_reference(env):
    """The same 60 queries in ONE maple_placement_search_batch call (device-side traversal, one lane per query)."""
    from maple_amd.search import PlacementParams, PlacementSearcher
    f, dev, tree = env
    ctx = f["context"]
    flags = f["flags"]
    only_identical = any(x in flags for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    ps = PlacementSearcher(dev, tree, PlacementParams(
        oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
        thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
        thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
        allowedFails=ctx["allowedFails"], strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical))
    recs = f["placements"]
    res = ps.find_best_parent_batch([tup(r["query"]) for r in recs])
    n_real = 0
    for rec, (node, score, blens, best_diffs, info) in zip(recs, res):
        want = rec["ret"]
        assert node == want["bestNode"], (node, want["bestNode"])
        assert close(score, want["bestScore"], 1e-9), (score, want["bestScore"])
        if want["bestBranchLengths"] is None:
            assert blens is None
        else:
            wb = [0.0 if b is False else b for b in want["bestBranchLengths"]]
            assert all(close(g, w, 1e-8, 1e-15) for g, w in zip(blens, wb)), (blens, wb)
            assert info["n_append"] == rec["n_append"], (info["n_append"], rec["n_append"])
            n_real += 1
        assert lists_match(best_diffs, tup(want["bestDiffs"]), 0.0), (best_diffs, want["bestDiffs"])
    assert n_real > 20


def test_placement_supports_match_reference(env):
    """f3: the computePlacementSupportOnly=True return of findBestParentForNewSample (M:8101-8290), the form the
    reference's batch-placement call site consumes (process_chunk, M:11200): possiblePlacements (node, support, branch
    lengths) in the reference's order and bestPlacementTotalLh, for the recorded queries, in ONE batch call."""
    from maple_amd.search import PlacementParams, PlacementSearcher
    f, dev, tree = env
    if "supports" not in f["placements"][0]:
        pytest.skip("fixture without supports records")
    ctx = f["context"]
    flags = f["flags"]
    only_identical = any(x in flags for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    ps = PlacementSearcher(dev, tree, PlacementParams(
        oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
        thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
        thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
        allowedFails=ctx["allowedFails"], strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical))
    recs = f["placements"]
    got = ps.find_placement_supports([tup(r["query"]) for r in recs], ctx["thresholdLogLKoptimizationTopology"],
                                     ctx["minBranchSupport"])
    n_multi = 0
    for rec, (placements, total_lh) in zip(recs, got):
        want = rec["supports"]
        assert [p[0] for p in placements] == [p[0] for p in want["possiblePlacements"]], (placements, want["possiblePlacements"])
        for g, w in zip(placements, want["possiblePlacements"]):
            assert close(g[1], w[1], 1e-7), (g, w)
            assert all(close(a, b, 1e-7, 1e-15) for a, b in zip(g[2], w[2])), (g, w)
        assert lists_match(total_lh, tup(want["bestPlacementTotalLh"]), 1e-7), (total_lh[:3], want["bestPlacementTotalLh"][:3])
        n_multi += len(placements) > 1
    assert n_multi > 0 or f["name"].startswith("b1429")      # (no query of that fixture has two supported placements)


def test_batched_placement_in_chunks_is_the_same(env, monkeypatch):
    """A batch too large for the arena is processed in chunks whose temporaries are released; the lists handed back
    (bestDiffs) are compacted to the bottom of the arena and must still be the reference's."""
    f, dev, tree = env
    ctx = f["context"]
    flags = f["flags"]
    only_identical = any(x in flags for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    kw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"], thresholdLogLK=ctx["thresholdLogLK"],
              thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
              thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], allowedFails=ctx["allowedFails"],
              strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical)
    recs = f["placements"]
    dev.placement_prepare(**kw)
    mark = dev.mark()
    q_ids = dev.upload([tup(r["query"]) for r in recs])
    whole = dev.placement_search_batch(q_ids, **kw)
    whole_lists = dev.download(whole["bestDiffs"])
    used_whole = dev.stats()["n_entries"]
    dev.release(mark)
    dev.set_tuning(placement_chunk_max=7)
    mark = dev.mark()
    q_ids = dev.upload([tup(r["query"]) for r in recs])
    parts = dev.placement_search_batch(q_ids, **kw)
    dev.set_tuning()
    part_lists = dev.download(parts["bestDiffs"])
    used_parts = dev.stats()["n_entries"]
    dev.release(mark)
    for k in ("bestNode", "bestScore", "blen", "nAppend", "status"):
        assert np.array_equal(whole[k], parts[k]), k
    assert whole_lists == part_lists
    for rec, lst in zip(recs, part_lists):
        assert lists_match(lst, tup(rec["ret"]["bestDiffs"]), 0.0)
    assert used_parts <= used_whole


def test_tree_log_likelihood_matches_reference(env):
    """The parity metric of BASELINE.json: tree log-LK (calculateTreeLikelihood, M:9721) within 1e-6 relative
    (observed ~1e-14) on the reference's own final tree."""
    from maple_amd.tree_host import tree_log_likelihood
    f, dev, tree = env
    if "treeLK" not in f:
        pytest.skip("fixture predates the tree-LK record")
    got, got_root = tree_log_likelihood(dev, tree)
    assert close(got_root, f["rootLK"], 1e-12), (got_root, f["rootLK"])
    assert close(got, f["treeLK"], 1e-11), (got, f["treeLK"])
    assert abs(got - f["treeLK"]) / abs(f["treeLK"]) < 1e-6


def test_wide_searches_batch_scored_identically():
    """Deep-round searches that walk most of the tree are batch-scored (k_append_queries) and replayed over the cached
    scores; every output must be bit-identical to the plain lane-sequential search (a size-independent property,
    checked on a synthetic 1500-tip tree built on the GPU)."""
    import math
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_mirror import TreeMirror
    data = make_dataset(n_samples=1500, l_ref=29903, seed=3, mean_diffs=30.0)
    ref_idx, rf = reference_tables(data.ref)
    dev = Device(ref_idx, rf, arena_bytes=1 << 30)
    dev.set_model([[-0.55, 0.06, 0.37, 0.12], [0.17, -2.6, 0.04, 2.39], [0.84, 0.13, -2.4, 1.43], [0.07, 0.48, 0.05, -0.6]])
    tips = {int(v): tip_genome_list(dl, ref_idx) for v, dl in zip(data.tip_node, data.diffs)}
    m = TreeMirror(dev, data.parent, data.blen, tips).build()
    dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left,
                    m.tot_up, -np.ones(m.n_nodes, dtype=np.int32))
    ll = math.log(dev.lRef)
    kw = dict(strict=False, allowedFails=4, thresholdLogLKtopology=14.0 * ll, thresholdTopologyPlacement=-0.1,
              thresholdLogLKoptimizationTopology=ll, thresholdLogLKconsecutivePlacement=1.0,
              effectivelyNon0BLen=1.0 / (10 * dev.lRef))
    nodes = np.arange(m.n_nodes)
    plain = dev.spr_search_batch(nodes, wide_search_budget=-1, **kw)
    hybrid = dev.spr_search_batch(nodes, wide_search_budget=64, **kw)
    assert (plain["status"] >= 0).all() and (plain["nAppend"] > 64).sum() > 50
    for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "blen", "improvement", "currentLK"):
        assert np.array_equal(plain[k], hybrid[k]), k
    # and a sanity property of every proposed move: it improves on the current placement by the accept margin
    mv = plain["placement"] >= 0
    assert (plain["bestScore"][mv] - 0.1 > plain["currentLK"][mv]).all()
    dev.close()


def test_hybrid_search_with_local_references_matches_reference(env):
    """The wide-search regime on the reference's own trees, which carry MAT local references: with a budget of 8
    placements nearly every search is handed to the batch kernel (removed list re-expressed in every reference frame,
    scores cached, traversal replayed) -- results must still be the reference's."""
    f, dev, tree = env
    ctx = f["context"]
    assert any(len(m) for m in tree.mutations)
    rnd = f["spr"][1]                                                  # the deep-round parameter set
    ps, calls = rnd["params"], rnd["calls"]
    nodes = [tree.children[c["node"]][c["child"]] for c in calls]
    kw = dict(strict=ps["strict"], allowedFails=ps["fails"], thresholdLogLKtopology=ps["thr"],
              thresholdTopologyPlacement=ps["place"],
              thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
              thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
              effectivelyNon0BLen=ctx["effectivelyNon0BLen"])
    out = dev.spr_search_batch(nodes, wide_search_budget=8, want_removed_partials=True, **kw)
    plain = dev.spr_search_batch(nodes, wide_search_budget=-1, **kw)
    assert (np.asarray([c["n_append"] for c in calls]) > 8).sum() > min(100, len(calls) // 2)
    rpr = dev.download(out["removedPartials"])
    for k, c in enumerate(calls):
        want = c["ret"]
        assert out["status"][k] == 0
        assert int(out["bestNode"][k]) == want["bestNode"], (k, out["bestNode"][k], want["bestNode"])
        assert int(out["nAppend"][k]) == c["n_append"], (k, out["nAppend"][k], c["n_append"])
        assert close(float(out["bestScore"][k]), want["bestScore"], 1e-8)
        # bestRemovedPartials: the removed list in the best branch's reference frame, shortened where the reference did
        assert lists_match(rpr[k], tup(want["bestRemovedPartials"]), 1e-7), (k, rpr[k][:3], want["bestRemovedPartials"][:3])
    for key in ("status", "bestNode", "placement", "nAppend"):
        assert np.array_equal(plain[key], out[key]), key
    for key in ("bestScore", "blen", "improvement"):
        assert np.allclose(plain[key], out[key], rtol=1e-11, atol=1e-15), key


def _model_for(mode, l_ref, seed=31):
    """Model tables of BASELINE's configs[1..3]: UNREST; + per-site rates; + per-site error rates."""
    import math
    Qm = [[-0.55, 0.06, 0.37, 0.12], [0.17, -2.6, 0.04, 2.39], [0.84, 0.13, -2.4, 1.43], [0.07, 0.48, 0.05, -0.6]]
    kw = dict(Q=Qm)
    rng = np.random.default_rng(seed)
    if mode != "unrest":
        kw["siteRates"] = np.clip(rng.gamma(0.5, 2.0, size=l_ref), 0.001, 0.005 * l_ref)
    if mode == "siteerr":
        er = np.exp(rng.uniform(math.log(1e-10), math.log(1e-3), size=l_ref))
        kw.update(usingErrorRate=True, errorRates=er, errorRateGlobal=float(er.mean()))
    return kw


@pytest.mark.parametrize("mode", ["unrest", "ratevar", "siteerr"])
def test_hybrid_search_on_big_tree_with_local_references(mode):
    """A 1500-tip tree given MAT local references the way setUpMAT does (maple_amd.mat, 30 descendants per clade):
    lane-only search, hybrid search and the C oracle's search agree on every node id, move and candidate count."""
    import math
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.mat import add_local_references
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_host import HostTree
    from maple_amd.tree_mirror import TreeMirror
    from oracle.oracle_py import Oracle, OracleTree
    data = make_dataset(n_samples=1500, l_ref=29903, seed=6, mean_diffs=30.0, frac_with_n=0.05, frac_ambig=0.05,
                        rate_variation=(mode != "unrest"))
    ref_idx, rf = reference_tables(data.ref)
    mkw = _model_for(mode, len(ref_idx))
    dev = Device(ref_idx, rf, arena_bytes=2 << 30)
    dev.set_model(**mkw)
    orc = Oracle(ref_idx, rf)
    orc.set_model(**mkw)
    tip_kw = dict(error_rates=mkw["errorRates"]) if mode == "siteerr" else {}
    tips = {int(v): tip_genome_list(dl, ref_idx, **tip_kw) for v, dl in zip(data.tip_node, data.diffs)}
    m = TreeMirror(dev, data.parent, data.blen, tips).build()
    ht = HostTree.from_mirror(m)
    n_ref = add_local_references(dev, ht, 30)
    assert n_ref > 20
    n = ht.n
    up = np.asarray([-1 if u is None else u for u in ht.up], dtype=np.int32)
    c0 = np.asarray([c[0] if c else -1 for c in ht.children], dtype=np.int32)
    c1 = np.asarray([c[1] if c else -1 for c in ht.children], dtype=np.int32)
    dist = np.asarray([float(x or 0.0) for x in ht.dist])
    dev.upload_tree(ht.root, up, c0, c1, dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft, ht.id_totUp, ht.id_mut)
    lists4 = [dev.download(ids) for ids in (ht.id_lower, ht.id_upRight, ht.id_upLeft, ht.id_totUp)]
    otree = OracleTree(orc, ht.root, ht.up, ht.children, dist, ht.mutations, [0] * n, lists4)
    ll = math.log(dev.lRef)
    kw = dict(strict=False, allowedFails=4, thresholdLogLKtopology=14.0 * ll, thresholdTopologyPlacement=-0.1,
              thresholdLogLKoptimizationTopology=ll, thresholdLogLKconsecutivePlacement=1.0,
              effectivelyNon0BLen=1.0 / (10 * dev.lRef))
    nodes = np.arange(n)
    plain = dev.spr_search_batch(nodes, wide_search_budget=-1, **kw)
    hybrid = dev.spr_search_batch(nodes, wide_search_budget=64, **kw)
    assert (plain["status"] >= 0).all() and (plain["nAppend"] > 64).sum() > 50
    for k in ("status", "bestNode", "placement", "nAppend"):
        assert np.array_equal(plain[k], hybrid[k]), k
    for k in ("bestScore", "blen", "improvement", "currentLK"):
        assert np.allclose(plain[k], hybrid[k], rtol=1e-11, atol=1e-15), k
    sel = nodes[::5]
    o = orc.spr_worker(otree, sel, **kw)
    for k in ("status", "bestNode", "placement", "nAppend"):
        assert np.array_equal(hybrid[k][sel], o[k]), k
    assert np.allclose(hybrid["bestScore"][sel], o["bestScore"], rtol=1e-11, atol=1e-15)
    dev.close()


@pytest.mark.parametrize("mode", ["unrest", "ratevar", "siteerr"])
def test_device_search_vs_oracle_search_on_gpu_built_tree(mode):
    """Beyond the reference's small recorded trees: every node of a 1500-tip synthetic tree (mirror built on the GPU)
    searched by the device state machine and by the C oracle (itself pinned to the reference's records): node ids,
    proposed moves and candidate counts bit-exact, scores to 1e-12."""
    import math
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_mirror import TreeMirror
    from oracle.oracle_py import Oracle, OracleTree
    data = make_dataset(n_samples=1500, l_ref=29903, seed=4, mean_diffs=30.0, frac_with_n=0.05, frac_ambig=0.05,
                        rate_variation=(mode != "unrest"))
    ref_idx, rf = reference_tables(data.ref)
    mkw = _model_for(mode, len(ref_idx))
    dev = Device(ref_idx, rf, arena_bytes=1 << 30)
    dev.set_model(**mkw)
    orc = Oracle(ref_idx, rf)
    orc.set_model(**mkw)
    tip_kw = dict(error_rates=mkw["errorRates"]) if mode == "siteerr" else {}
    tips = {int(v): tip_genome_list(dl, ref_idx, **tip_kw) for v, dl in zip(data.tip_node, data.diffs)}
    m = TreeMirror(dev, data.parent, data.blen, tips).build()
    n = m.n_nodes
    dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left,
                    m.tot_up, -np.ones(n, dtype=np.int32))
    lists4 = []
    for ids in (m.lower, m.up_right, m.up_left, m.tot_up):
        got = dev.download(ids)
        lists4.append(got)
    up = [None if p < 0 else int(p) for p in m.parent]
    children = [[] if m.children[v, 0] < 0 else [int(m.children[v, 0]), int(m.children[v, 1])] for v in range(n)]
    otree = OracleTree(orc, m.root, up, children, m.dist, [[] for _ in range(n)], [0] * n, lists4)
    ll = math.log(dev.lRef)
    nodes = np.arange(n)
    for kw in (dict(strict=True, allowedFails=2, thresholdLogLKtopology=6.0 * ll),
               dict(strict=False, allowedFails=4, thresholdLogLKtopology=14.0 * ll)):
        kw.update(thresholdTopologyPlacement=-0.1, thresholdLogLKoptimizationTopology=ll,
                  thresholdLogLKconsecutivePlacement=1.0, effectivelyNon0BLen=1.0 / (10 * dev.lRef))
        sel = nodes if kw["strict"] else nodes[::7]                   # the deep round is ~100x the work on the CPU
        g = dev.spr_search_batch(sel, **kw)
        o = orc.spr_worker(otree, sel, **kw)
        lane = dev.spr_search_batch(sel, search_tier=1, **kw)            # one lane per search instead of the frontier tier
        for k in ("status", "bestNode", "placement", "nAppend"):
            assert np.array_equal(g[k], o[k]), k
            assert np.array_equal(g[k], lane[k]), k
        assert np.array_equal(g["bestScore"], lane["bestScore"]) and np.array_equal(g["blen"], lane["blen"])
        for k in ("bestScore", "currentLK", "improvement", "blen"):
            assert np.allclose(g[k], o[k], rtol=1e-11, atol=1e-15), k
        assert g["nAppend"].sum() > 10000
        if not kw["strict"]:
            # the whole-tree searches of the full round, replayed inside the frontier tier (k_fr_replay_wide) and one wavefront
            # per search from their first step (k_spr_search): the same results, bit for bit
            dev.timing_reset()
            a = dev.spr_search_batch(nodes, **kw)
            inside = dev.timing_read_kind(Device.KIND_FR_WIDE)[0]
            dev.set_tuning(wide_outside_frontier=True)
            b = dev.spr_search_batch(nodes, **kw)
            dev.set_tuning(dense_wide_scoring=True)                      # every branch scored instead of the witness filter's survivors
            d = dev.spr_search_batch(nodes, **kw)
            dev.set_tuning()
            for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
                assert np.array_equal(a[k], b[k]), k
                assert np.array_equal(a[k], d[k]), k
            assert np.array_equal(a["nAppend"][::7], g["nAppend"])
            if mode != "siteerr":                                        # (without an error model such searches are known beforehand)
                assert inside > 0
    dev.close()


def test_rebuild_all_genome_lists_matches_reference(env):
    """reCalculateAllGenomeLists (M:6013-6347) as level-synchronous GPU batches, on the reference's own final tree
    (with MAT local references): from the tips' lists alone, every other list of the tree must come out as the
    reference computed it.

    With an error model the reference's tips share their ambiguity vectors between samples (one object per
    ambiguity code, rewritten in place by updateProbVectTerminalNode M:3966 for whichever tip is visited last with
    that site's error rate), so its internal lists were merged from tip values that no longer exist in the final
    tree; there only the lists that no such tip feeds can agree (more than half of them do)."""
    from maple_amd.tree_host import rebuild_genome_lists
    f, dev, tree = env
    mark = dev.mark()
    lower, up_right, up_left, tot_up = rebuild_genome_lists(dev, tree)
    t = f["tree"]
    # (with an error model too: the fixtures' tips are de-aliased before the reference recomputes its lists, see
    # make_golden_search.frozen_reference_tree, so every list is a function of the tips' lists)
    exact = True
    checked = n_same = 0
    for ids, key in ((lower, "probVect"), (up_right, "probVectUpRight"), (up_left, "probVectUpLeft"), (tot_up, "probVectTotUp")):
        nodes = [v for v in tree.preorder() if t[key][v]]
        assert all(ids[v] >= 0 for v in nodes), key
        got = dev.download(ids[nodes])
        for v, g in zip(nodes, got):
            want = tup(t[key][v])
            same = lists_match(g, want, 1e-9)
            assert same or not exact, (key, v)
            n_same += bool(same)
            checked += 1
    assert checked > min(700, 3 * len(nodes) // 2)
    assert n_same == checked, (n_same, checked)
    dev.release(mark)


@pytest.mark.parametrize("uname", UPDATE_NAMES)
def test_update_partials_matches_reference(uname):
    """updatePartials (M:5479-5815) as level-synchronous GPU batches vs the reference's own repair of the same local
    change (tests/golden/update_synth_unrest.json.gz: 7 branch-length changes, 7 tip replacements on the frozen tree).
    Both stop propagating where areVectorsDifferent says "same", in a different visiting order, so lists are compared
    with that function's own thresholds rather than bit for bit; the tree log-likelihood must agree to 1e-9."""
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree, tree_log_likelihood, update_genome_lists
    f = load(uname)
    upd = load_update(uname)
    ctx, t = f["context"], f["tree"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                 minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                 thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"],
                 arena_bytes=256 << 20)
    dev.set_model(**model_args(f["model"]))
    keys = (("probVect", "id_lower"), ("probVectUpRight", "id_upRight"), ("probVectUpLeft", "id_upLeft"),
            ("probVectTotUp", "id_totUp"))
    n_lists = 0
    for case in upd["cases"]:
        tree = HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"],
                        t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
        ch = case["change"]
        v = ch["node"]
        if ch["kind"] == "dist":
            tree.dist[v] = ch["dist"]
        else:
            tree.id_lower[v] = dev.upload([tup(ch["probVect"])])[0]
        # the same repair by the Python level loop on a second copy of the tree: the library's loop (maple_update_partials) is
        # the same algorithm call for call, so the lists it leaves are identical entry for entry
        twin = HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], None, None, None, None)
        twin.id_mut = tree.id_mut
        for _, attr in keys:
            setattr(twin, attr, getattr(tree, attr).copy())
        twin.dist[v] = tree.dist[v]
        pre = {attr: getattr(tree, attr).copy() for _, attr in keys}
        replaced = update_genome_lists(dev, tree, [v])
        assert replaced >= 1
        moved_nodes = set()
        for _, attr in keys:
            moved_nodes.update(np.nonzero(getattr(tree, attr) != pre[attr])[0].tolist())
        assert moved_nodes <= set(dev.update_partials_touched().tolist())      # what maple_tree_patch has to be told
        try:
            twin_replaced = update_genome_lists(dev, twin, [v], native=False)
        except RuntimeError as e:
            # the Python cross-check stops where the upper pass meets an inconsistent zero-length branch (the reference's
            # updateBLen inside the from-parent direction, M:5522-5600); the library's loop handles it (update_plan.h: that arm is
            # pinned on the CPU by test_update_plan.py::test_none_in_the_upper_pass) and is still compared with the reference's
            # own repair below
            if "updateBLen" not in str(e):
                raise
            twin = None
        if twin is not None:
            assert twin_replaced == replaced
            assert np.array_equal(twin.dist, tree.dist)
            for _, attr in keys:
                a, b = getattr(tree, attr), getattr(twin, attr)
                assert np.array_equal(a >= 0, b >= 0), attr
                moved = np.nonzero((a >= 0) & (a != b))[0]
                if len(moved):
                    la, lb = dev.download(a[moved]), dev.download(b[moved])
                    assert la == lb, (attr, moved[:5])
        # every list of every node against the reference's tree after ITS updatePartials
        for key, attr in keys:
            ids = getattr(tree, attr)
            nodes, want = [], []
            for w in tree.preorder():
                ref = case["lists"].get(str(w), {}).get(key, t[key][w])
                if w == v and key == "probVect" and ch["kind"] == "tip":
                    ref = ch["probVect"]
                if ref:
                    nodes.append(w)
                    want.append(tup(ref))
                else:
                    assert ids[w] < 0 or key != "probVectTotUp" or not tree.dist[w], (key, w)
            assert all(ids[w] >= 0 for w in nodes), key
            want_ids = dev.upload(want)
            differ = dev.differ_batch(ids[nodes], want_ids) | dev.differ_batch(want_ids, ids[nodes])
            assert not differ.any(), (ch, key, [nodes[i] for i in np.nonzero(differ)[0]][:5])
            n_lists += len(nodes)
        for w, d in case["dist"].items():
            assert close(float(tree.dist[int(w)] or 0.0), float(d or 0.0), 1e-6, 1e-12), (w, tree.dist[int(w)], d)
        got, _ = tree_log_likelihood(dev, tree)
        assert close(got, case["treeLK"], 1e-9), (ch, got, case["treeLK"])
    assert n_lists > 3000
    dev.close()


def test_branch_length_fast_pass_matches_reference(env):
    """traverseTreeToOptimizeBranchLengths(fastPass=True) (M:8727-8893) as one estimateBranchLength launch + one root
    grid launch: branch lengths and the number of updates of the reference, on the converged tree and on a tree whose
    branch lengths were all perturbed."""
    from maple_amd.tree_host import optimize_branch_lengths_fast_pass
    f, dev, tree = env
    upd = load_update(f["name"])
    saved = list(tree.dist)
    try:
        for rec in upd["blen_sweeps"]:
            tree.dist = list(rec["dist_in"])
            updates, dirty = optimize_branch_lengths_fast_pass(dev, tree, upd["effectivelyNon0BLen"])
            assert updates == rec["updates"], (updates, rec["updates"])
            reach = tree.preorder()
            assert all(close(tree.dist[v], rec["dist_out"][v], 1e-7, 1e-15) for v in reach), \
                [(v, tree.dist[v], rec["dist_out"][v]) for v in reach if not close(tree.dist[v], rec["dist_out"][v], 1e-7, 1e-15)][:5]
            assert [dirty[v] for v in reach if v != tree.root and tree.up[v] != tree.root] == \
                   [rec["dirty_out"][v] for v in reach if v != tree.root and tree.up[v] != tree.root]
    finally:
        tree.dist = saved


@pytest.mark.parametrize("uname", UPDATE_NAMES)
def test_branch_length_sweep_matches_reference(uname):
    """f4: traverseTreeToOptimizeBranchLengths(tree, root) with the reference's default arguments (fastPass=False: the
    form every call site uses, M:8727-8893) -- a Gauss-Seidel sweep in the reference's order, one repair of the genome
    lists after every changed branch -- on the converged tree and on the tree with every length perturbed: the
    reference's number of updates, the nodes it updated in its order, every branch length, and the tree log-likelihood
    before and after."""
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree, optimize_branch_lengths, rebuild_genome_lists, tree_log_likelihood
    f = load(uname)
    upd = load_update(uname)
    if "blen_full_sweeps" not in upd:
        pytest.skip("fixture without full-sweep records")
    ctx, t = f["context"], f["tree"]
    for rec in upd["blen_full_sweeps"]:
        dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                     minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                     thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"],
                     arena_bytes=512 << 20)
        dev.set_model(**model_args(f["model"]))
        tree = HostTree(t["root"], t["up"], t["children"], rec["dist_in"], t["mutations"], t["nMinor"], t["probVect"],
                        t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
        # the lists of the tree with the recorded input lengths (the reference recomputed them the same way)
        tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp = rebuild_genome_lists(dev, tree)
        lk_in, _ = tree_log_likelihood(dev, tree)
        assert close(lk_in, rec["treeLK_in"], 1e-9), (lk_in, rec["treeLK_in"])
        updates, dirty, updated = optimize_branch_lengths(dev, tree, upd["effectivelyNon0BLen"])
        lk_out, _ = tree_log_likelihood(dev, tree)
        reach = tree.preorder()
        worst = max(abs(tree.dist[v] - rec["dist_out"][v]) / max(abs(rec["dist_out"][v]), 1e-9) for v in reach)
        print(f"{uname}: {updates} updates (reference {rec['updates']}), LK {lk_in:.6f} -> {lk_out:.6f} "
              f"(reference {rec['treeLK_out']:.6f}), worst branch-length difference {worst:.2e}")
        assert updates == rec["updates"], (updates, rec["updates"])
        root_kids = set(tree.children[tree.root])
        assert [v for v in updated] == [v for v in rec["update_order"] if v not in root_kids], "updated branches / their order"
        assert all(close(tree.dist[v], rec["dist_out"][v], 1e-6, 1e-12) for v in reach), \
            [(v, tree.dist[v], rec["dist_out"][v]) for v in reach if not close(tree.dist[v], rec["dist_out"][v], 1e-6, 1e-12)][:5]
        assert close(lk_out, rec["treeLK_out"], 1e-9), (lk_out, rec["treeLK_out"])
        assert lk_out >= lk_in - 1e-6
        dev.close()


def test_candidate_sharding_level2(env):
    """SURVEY 8e level 2: three ranks' candidate / leaf shards of one query, re-interleaved, are exactly the
    single-GPU score and minor-test vectors (the collective itself is covered by the gloo test)."""
    from maple_amd.search import PlacementParams, PlacementSearcher
    f, dev, tree = env
    ctx = f["context"]
    pp = PlacementParams(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
                         thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
                         thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"])
    one = PlacementSearcher(dev, tree, pp)
    world = 3
    shards = [PlacementSearcher(dev, tree, pp, rank=r, world=world) for r in range(world)]
    mark = dev.mark()
    q_id = dev.upload([tup(f["placements"][3]["query"])])[0]
    U, _ = one._frame_lists(q_id)
    frame_lists = [U[fr] for fr in one.frame_order]
    full = dev.append_candset(one.cset_cand, frame_lists, True, pp.oneMutBLen)
    full_minor = dev.minor_candset(one.cset_leaf, frame_lists, False)
    got = np.zeros(len(one.cand))
    got_minor = np.zeros(len(one.leaves), dtype=np.uint8)
    for r, s in enumerate(shards):
        sc = dev.append_candset(s.cset_cand, frame_lists, True, pp.oneMutBLen)
        assert sc[-1] == full[-1]                                   # every rank scores the root vector itself
        got[r::world] = sc[:-1]
        got_minor[r::world] = dev.minor_candset(s.cset_leaf, frame_lists, False)
    assert np.array_equal(got, full[:-1]) and np.array_equal(got_minor, full_minor)
    dev.release(mark)


def test_find_best_root_matches_reference(env):
    """findBestRoot's search (M:7730-7840) as level-synchronous GPU batches + host replay: best node, number of nodes
    visited and the relative log-likelihood of every branch the reference keeps in bestNodes (224 of them)."""
    from maple_amd.tree_host import find_best_root
    f, dev, tree = env
    upd = load_update(f["name"])
    ctx = f["context"]
    for rec in upd["find_best_root"]:
        node, best, best_nodes, visited = find_best_root(
            dev, tree, strictTopologyStopRules=rec["strict"], allowedFailsTopology=rec["fails"],
            thresholdLogLKtopology=rec["thr"], thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
            thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"])
        assert node == rec["bestNode"] and visited == rec["visited"], (node, rec["bestNode"], visited, rec["visited"])
        assert close(best, rec["bestLKdiff"], 1e-9, 1e-9)
        want = {int(k): v for k, v in rec["bestNodes"].items()}
        assert set(best_nodes) == set(want)
        assert all(close(best_nodes[k], want[k], 1e-7, 1e-7) for k in want), \
            [(k, best_nodes[k], want[k]) for k in want if not close(best_nodes[k], want[k], 1e-7, 1e-7)][:5]
        assert len(want) > 50


def test_tree_ops_under_reference_names(env):
    """maple_amd.ops.TreeOps: the tree-level functions under the reference's names give the recorded answers."""
    from maple_amd.ops import TreeOps
    f, dev, tree = env
    ctx = f["context"]
    ops = TreeOps(dev, tree)
    if "treeLK" in f:
        assert close(ops.calculateTreeLikelihood(), f["treeLK"], 1e-9)
    rnd = f["spr"][0]
    ps = rnd["params"]
    nodes = [tree.children[c["node"]][c["child"]] for c in rnd["calls"]]
    moves = ops.startTopologyUpdatesParallel(
        nodes, strictTopologyStopRules=ps["strict"], allowedFailsTopology=ps["fails"], thresholdLogLKtopology=ps["thr"],
        thresholdTopologyPlacement=ps["place"], thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
        thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
        effectivelyNon0BLen=ctx["effectivelyNon0BLen"])
    assert sorted((m[0], m[1]) for m in moves) == sorted((m[0], m[1]) for m in rnd["proposedMoves"])
    rec = f["placements"][0]
    only_identical = any(x in f["flags"] for x in ("--estimateErrorRate", "--estimateSiteSpecificErrorRate"))
    node, score, blens, diffs = ops.findBestParentForNewSample(
        tup(rec["query"]), oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
        thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
        thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], allowedFails=ctx["allowedFails"],
        strictStopRules=ctx["strictStopRules"], onlyFindIdentical=only_identical)
    assert node == rec["ret"]["bestNode"] and close(score, rec["ret"]["bestScore"], 1e-9)


# ---- end-to-end: the metric's second half (final tree log-LK) on sequences of tree states the reference produced ----
E2E_NAMES = sorted(f[len("e2e_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("e2e_"))


def _e2e_env(name):
    from maple_amd.runtime import Device
    with gzip.open(os.path.join(GOLDEN, f"e2e_{name}.json.gz"), "rt") as fh:
        f = json.load(fh)
    ctx = f["context"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                 minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                 thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"],
                 arena_bytes=1 << 30)
    return f, dev


def _tree_from_topology(dev, topo, tips):
    """HostTree of a recorded tree state: topology + the tips' lists; every other list rebuilt on the GPU."""
    from maple_amd.tree_host import HostTree, rebuild_genome_lists
    n = len(topo["up"])
    pv = [None] * n
    for v, lst in tips.items():
        if int(v) < n and not topo["children"][int(v)]:
            pv[int(v)] = lst
    tree = HostTree(topo["root"], topo["up"], topo["children"], topo["dist"], topo.get("mutations") or [[] for _ in range(n)],
                    topo["nMinor"], pv, [None] * n, [None] * n, [None] * n).upload(dev)
    tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp = rebuild_genome_lists(dev, tree)
    return tree


def _has_moves(name):
    with gzip.open(os.path.join(GOLDEN, f"e2e_{name}.json.gz"), "rt") as fh:
        return bool(json.load(fh)["spr_moves"])


# (e2e_b1429_unrest: the reference applied no move on that tree; e2e_synth_fullmodel_mat records online additions only)
@pytest.mark.parametrize("name", [n for n in E2E_NAMES if _has_moves(n)])
def test_applied_spr_moves_tree_likelihood(name):
    """Metric part 2 on the reference's own SPR rounds: for every move the reference APPLIED (40 in a row, starting from a
    tree with 30 tips misplaced), the tree it produced is rebuilt on the GPU from the tips alone and its log-likelihood
    (calculateTreeLikelihood, M:9721-9779) must be the reference's to 1e-9; the reference's predicted improvement and the
    realised change of log-likelihood agree within its own --debugging bound of 0.5 (M:9508-9565)."""
    from maple_amd.tree_host import tree_log_likelihood
    f, dev = _e2e_env(name)
    if not f["spr_moves"]:
        pytest.skip("no applied SPR moves recorded")
    worst = 0.0
    for k, mv in enumerate(f["spr_moves"]):
        dev.set_model(mv["Q"])
        mark = dev.mark()
        tree = _tree_from_topology(dev, mv["after"], f["tips"])
        lk, _ = tree_log_likelihood(dev, tree)
        dev.release(mark)
        assert close(lk, mv["lk_after_fresh"], 1e-9), (k, lk, mv["lk_after_fresh"])
        worst = max(worst, abs(lk - mv["lk_after_fresh"]) / abs(lk))
        # predicted vs realised: the reference's own pair of numbers first (its --debugging bound is 0.5; a few of its large
        # moves miss that by themselves, e.g. 58.2 predicted / 56.2 realised), then ours against its prediction
        realised = mv["lk_after_incremental"] - mv["lk_before"]
        bound = max(0.5, 0.05 * abs(mv["improvement"]))
        assert abs(realised - mv["improvement"]) <= bound, (k, realised, mv["improvement"])
        assert abs(lk - mv["lk_before"] - mv["improvement"]) <= bound, (k, lk - mv["lk_before"], mv["improvement"])
        assert abs((lk - mv["lk_before"]) - realised) <= 1e-3, (k, lk - mv["lk_before"], realised)
    assert len(f["spr_moves"]) >= 20
    print(f"{name}: {len(f['spr_moves'])} applied moves, worst relative log-LK difference {worst:.2e}")
    dev.close()


@pytest.mark.parametrize("name", E2E_NAMES)
def test_online_sample_additions_through_tree_patch(name):
    """The same sequence as test_online_sample_additions with the library's copy of the tree kept up to date by
    maple_tree_patch (HostTree.sync: only the nodes a placement touched) instead of a full maple_tree_upload per sample:
    every single-query placement search on the patched tree must still return the reference's node, score and branch
    lengths, and the tables the batched search needs are rebuilt from the patched copy when it is asked for one."""
    from maple_amd.tree_host import update_genome_lists
    f, dev = _e2e_env(name)
    ctx = f["context"]
    dev.set_model(**model_args(f["model"]))
    tree = _tree_from_topology(dev, f["online_start"], f["tips"])
    pkw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"], thresholdLogLK=ctx["thresholdLogLK"],
               thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
               thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], allowedFails=ctx["allowedFails"],
               strictStopRules=ctx["strictStopRules"])
    tree.upload_topology(dev)
    patched = []
    last = None
    for k, rec in enumerate(f["online"]):
        patched.append(tree.sync(dev))
        dev.placement_prepare(**pkw)                                  # (root vector, outside the mark)
        mark = dev.mark()
        qid = dev.upload([tup(rec["query"])])
        out = dev.placement_search_batch(qid, **pkw)
        want = rec["ret"]
        assert out["status"][0] >= 0
        assert int(out["bestNode"][0]) == want["bestNode"], (k, out["bestNode"][0], want["bestNode"])
        assert close(float(out["bestScore"][0]), want["bestScore"], 1e-8), (k, out["bestScore"][0], want["bestScore"])
        if want["bestBranchLengths"] is None:
            assert out["status"][0] == 1
        else:
            # (branch lengths come out of a bisection that stops at minBLenSensitivity, on lists the two sides repaired in a
            # different order after 27 additions: 1e-6, the tolerance north_star states for floating point)
            assert all(close(float(g), w, 1e-6, 1e-15) for g, w in zip(out["blen"][0], want["bestBranchLengths"])), (k, out["blen"][0], want)
        last = (qid.copy(), {kk: v.copy() for kk, v in out.items()})
        dev.release(mark)
        after = rec["after"]
        changed = tree.apply_topology(after["root"], after["up"], after["children"], after["dist"], after["nMinor"],
                                      after.get("mutations"), dev)
        for v, lst in rec["new_tips"].items():
            tree.id_lower[int(v)] = dev.upload([tup(lst)])[0]
            if int(v) not in changed:
                changed.append(int(v))
        if changed:
            update_genome_lists(dev, tree, changed)
    print(f"{name}: nodes patched per added sample {patched}")
    assert patched[0] == 0 and all(-1 <= p < tree.n // 4 for p in patched), patched   # a few nodes each, never the whole tree
    assert sum(p > 0 for p in patched) >= len(patched) // 2, patched
    # a batch on the patched tree: the linearised tables are rebuilt from the library's copy; the last query again, five times
    tree.sync(dev)
    dev.placement_prepare(**pkw)
    mark = dev.mark()
    rec = f["online"][-1]
    qids = dev.upload([tup(rec["query"])] * 5)
    out = dev.placement_search_batch(qids, **pkw)
    assert (out["status"] >= 0).all() and len(set(out["bestNode"].tolist())) == 1
    dev.release(mark)
    dev.close()


def _has_mat(f):
    """Does the recorded online sequence ever have MAT local references (mutations on a branch)?"""
    topos = [f["online_start"]] + [r["after"] for r in f["online"]]
    return any(any(m for m in (t.get("mutations") or [])) for t in topos)


def test_an_e2e_fixture_without_mat_references():
    """The announced loop below makes rows only on trees without MAT references: at least one fixture must be one."""
    assert any(not _has_mat(json.load(gzip.open(os.path.join(GOLDEN, f"e2e_{n}.json.gz"), "rt"))) for n in E2E_NAMES)


@pytest.mark.parametrize("chunk", [30, 7])
@pytest.mark.parametrize("name", E2E_NAMES)
def test_announced_online_sample_additions_match_reference(name, chunk):
    """The sequence of test_online_sample_additions_through_tree_patch with its samples announced (maple_placement_ahead:
    `chunk` at a time, so that with 7 the batch boundaries fall inside the sequence): every search must still return the
    reference's own recorded node, score and branch lengths.  The queries are uploaded before any per-step mark, so the
    per-search release leaves them.  On a fixture without MAT references every search takes its row; where the tree has MAT
    references nothing is taken (nTaken 0) and the results are the same."""
    from maple_amd.tree_host import update_genome_lists
    f, dev = _e2e_env(name)
    ctx = f["context"]
    dev.set_model(**model_args(f["model"]))
    tree = _tree_from_topology(dev, f["online_start"], f["tips"])
    pkw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"], thresholdLogLK=ctx["thresholdLogLK"],
               thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
               thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], allowedFails=ctx["allowedFails"],
               strictStopRules=ctx["strictStopRules"])
    tree.upload_topology(dev)
    recs = f["online"]
    qids = [int(x) for x in dev.upload([tup(r["query"]) for r in recs])]
    s0 = dev.placement_ahead_stats()
    waiting, n_taken, n_announced_on_mat = [], 0, 0
    for k, rec in enumerate(recs):
        tree.sync(dev)
        dev.placement_prepare(**pkw)
        if not waiting:
            batch = qids[k: k + chunk]
            got = dev.placement_ahead(np.asarray(batch, dtype=np.int32), **pkw)
            if any(tree.mutations):
                assert got == 0, (k, got)                             # (a tree with MAT references: the call changes nothing)
                n_announced_on_mat += 1
            n_taken += got
            waiting = batch[:got] if got > 0 else batch
        qid = waiting.pop(0)
        assert qid == qids[k]
        mark = dev.mark()
        out = dev.placement_search_batch(np.asarray([qid], dtype=np.int32), **pkw)
        dev.release(mark)
        want = rec["ret"]
        assert out["status"][0] >= 0
        assert int(out["bestNode"][0]) == want["bestNode"], (k, out["bestNode"][0], want["bestNode"])
        assert close(float(out["bestScore"][0]), want["bestScore"], 1e-8), (k, out["bestScore"][0], want["bestScore"])
        if want["bestBranchLengths"] is None:
            assert out["status"][0] == 1
        else:
            assert all(close(float(g), w, 1e-6, 1e-15) for g, w in zip(out["blen"][0], want["bestBranchLengths"])), (k, out["blen"][0], want)
        after = rec["after"]
        changed = tree.apply_topology(after["root"], after["up"], after["children"], after["dist"], after["nMinor"],
                                      after.get("mutations"), dev)
        for v, lst in rec["new_tips"].items():
            tree.id_lower[int(v)] = dev.upload([tup(lst)])[0]
            if int(v) not in changed:
                changed.append(int(v))
        if changed:
            update_genome_lists(dev, tree, changed)
    s1 = dev.placement_ahead_stats()
    used = s1["searches"] - s0["searches"]
    print(f"{name} (announced {chunk} at a time): {n_taken} taken, {used} searches on rows, "
          f"{s1['fallbacks'] - s0['fallbacks']} scored in full, {s1['traversals_ahead_used'] - s0['traversals_ahead_used']} traversals "
          f"made ahead used")
    if not _has_mat(f):
        assert n_taken == len(recs) and used == len(recs), (n_taken, used)
    else:
        assert used <= n_taken
        assert chunk >= len(recs) or n_announced_on_mat > 0       # (announced at least once on a tree with MAT references)
    dev.close()


@pytest.mark.parametrize("name", E2E_NAMES)
def test_online_sample_additions(name):
    """BASELINE configs[4] in small (online update of a frozen tree): new samples are added one after the other -- placement
    search on the GPU (must be the reference's node, score and branch lengths), the reference's tree edit applied from
    the record, incremental repair of the genome lists on the GPU (update_genome_lists) -- and after every addition the
    tree log-likelihood must be the reference's."""
    from maple_amd.search import PlacementParams, PlacementSearcher
    from maple_amd.tree_host import tree_log_likelihood, update_genome_lists
    f, dev = _e2e_env(name)
    ctx = f["context"]
    dev.set_model(**model_args(f["model"]))
    tree = _tree_from_topology(dev, f["online_start"], f["tips"])
    lk, _ = tree_log_likelihood(dev, tree)
    assert close(lk, f["online_start_LK"], 1e-9), (lk, f["online_start_LK"])
    params = PlacementParams(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"],
                             thresholdLogLK=ctx["thresholdLogLK"], thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
                             thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"],
                             allowedFails=ctx["allowedFails"], strictStopRules=ctx["strictStopRules"])
    worst = 0.0
    for k, rec in enumerate(f["online"]):
        tree.upload_topology(dev)
        ps = PlacementSearcher(dev, tree, params)
        node, score, blens, best_diffs, info = ps.find_best_parent_for_new_sample(tup(rec["query"]))
        want = rec["ret"]
        assert node == want["bestNode"], (k, node, want["bestNode"])
        assert close(score, want["bestScore"], 1e-8), (k, score, want["bestScore"])
        if want["bestBranchLengths"] is None:
            assert blens is None
        else:
            assert all(close(float(g or 0.0), w, 1e-6, 1e-15) for g, w in zip(blens, want["bestBranchLengths"])), (k, blens, want)
        after = rec["after"]
        changed = tree.apply_topology(after["root"], after["up"], after["children"], after["dist"], after["nMinor"],
                                      after.get("mutations"), dev)
        for v, lst in rec["new_tips"].items():
            tree.id_lower[int(v)] = dev.upload([tup(lst)])[0]
            if int(v) not in changed:
                changed.append(int(v))                   # (an existing tip the placement rewrote: a minor sequence, M:3966)
        if changed:
            update_genome_lists(dev, tree, changed)
        lk, _ = tree_log_likelihood(dev, tree)
        assert close(lk, rec["treeLK"], 1e-8), (k, lk, rec["treeLK"])
        worst = max(worst, abs(lk - rec["treeLK"]) / abs(lk))
    print(f"{name}: {len(f['online'])} samples added, worst relative log-LK difference {worst:.2e}")
    dev.close()
