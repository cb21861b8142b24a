"""maple_spr_search_batch leaves the arena as it found it: the removed lists it re-expresses in other reference frames (in the
root's frame for the rows made ahead and for the rows of a chunk, in every frame for the frame-by-frame rows) live under an
arena mark each and are gone when the call returns.  Which of the three a call went through is read from its trace
(tuning.verbose); its results are the lane tier's (searchTier = 1)."""
import gzip
import json
import math
import os

import numpy as np
import pytest

from golden_util import GOLDEN, model_args, ref_indices

pytestmark = pytest.mark.gpu
NAMES = sorted(f[len("search_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("search_") and f.endswith(".json.gz"))
SITES = {"ahead": "their removed lists in the root's frame",          # the rows made ahead, on the side stream
         "chunk": "replayed inside the frontier tier",                # a chunk's rows in the root's frame (on a tree with references)
         "frames": "removed lists in all"}                            # frame by frame
EXACT = ("status", "bestNode", "placement", "nAppend")


def searched_twice(dev, capfd, nodes, **kw):
    """the call once to settle what a context keeps (pools; the candidates' copies in the root's frame, made once per tree), then
    again between two looks at the arena: (sites its trace names, results)"""
    dev.spr_search_batch(nodes, **kw)
    before = dev.stats()
    dev.set_tuning(verbose=1)
    capfd.readouterr()
    out = dev.spr_search_batch(nodes, **kw)
    trace = capfd.readouterr().err
    dev.set_tuning()
    assert dev.stats() == before
    sites = {s for s, line in SITES.items() if line in trace}
    print("arena-mark sites reached:", sorted(sites))
    return sites, out


@pytest.mark.parametrize("name", NAMES)
def test_wide_searches_on_recorded_trees_leave_the_arena_as_it_was(name, capfd):
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        f = json.load(fh)
    ctx, t = f["context"], f["tree"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
                 thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
                 defaultBLen=ctx["defaultBLen"], arena_bytes=256 << 20)
    dev.set_model(**model_args(f["model"]))
    tree = HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"], t["probVectUpRight"],
                    t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
    assert any(len(m) for m in tree.mutations)
    ps, calls = f["spr"][1]["params"], f["spr"][1]["calls"]             # the deep-round parameter set
    nodes = [tree.children[c["node"]][c["child"]] for c in calls]
    kw = dict(strict=ps["strict"], allowedFails=ps["fails"], thresholdLogLKtopology=ps["thr"], thresholdTopologyPlacement=ps["place"],
              thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
              thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"])
    lane = dev.spr_search_batch(nodes, search_tier=1, wide_search_budget=-1, **kw)
    # with a budget of 8 placements nearly every search leaves the budgeted pass: in chunks of rows in the root's frame through the
    # frontier tier, what it hands back (on the scrambled trees; nothing on the others) frame by frame; kept in the lane tier, all of
    # them frame by frame
    for tier, want in ((0, {"chunk"}), (1, {"frames"})):
        sites, out = searched_twice(dev, capfd, nodes, wide_search_budget=8, search_tier=tier, **kw)
        assert want <= sites <= want | {"frames"}, (tier, sites)
        for k in EXACT:
            assert np.array_equal(out[k], lane[k]), (tier, k)
        for k in ("bestScore", "blen", "improvement"):
            assert np.allclose(out[k], lane[k], rtol=1e-11, atol=1e-15), (tier, k)
    dev.close()


def test_rows_made_ahead_on_a_tree_with_references_leave_the_arena_as_it_was(capfd):
    """The searches from zero-length branches, known beforehand without an error model: 64 of them or more get their rows ahead of
    the pass, on a tree with local references from copies of their removed lists in the root's frame (the 1500-tip tree of
    test_hip_search.py, references the way setUpMAT places them)."""
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.mat import add_local_references
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_host import HostTree
    from maple_amd.tree_mirror import TreeMirror
    data = make_dataset(n_samples=1500, l_ref=29903, seed=6, mean_diffs=30.0, frac_with_n=0.05, frac_ambig=0.05, rate_variation=False)
    ref_idx, rf = reference_tables(data.ref)
    dev = Device(ref_idx, rf, arena_bytes=2 << 30)
    dev.set_model([[-0.55, 0.06, 0.37, 0.12], [0.17, -2.6, 0.04, 2.39], [0.84, 0.13, -2.4, 1.43], [0.07, 0.48, 0.05, -0.6]])
    tips = {int(v): tip_genome_list(dl, ref_idx) for v, dl in zip(data.tip_node, data.diffs)}
    m = TreeMirror(dev, data.parent, data.blen, tips).build()
    ht = HostTree.from_mirror(m)
    assert add_local_references(dev, ht, 30) > 20
    up = np.asarray([-1 if u is None else u for u in ht.up], dtype=np.int32)
    c0 = np.asarray([c[0] if c else -1 for c in ht.children], dtype=np.int32)
    c1 = np.asarray([c[1] if c else -1 for c in ht.children], dtype=np.int32)
    dist = np.asarray([float(x or 0.0) for x in ht.dist])
    dev.upload_tree(ht.root, up, c0, c1, dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft, ht.id_totUp, ht.id_mut)
    ll = math.log(dev.lRef)
    kw = dict(strict=False, allowedFails=4, thresholdLogLKtopology=14.0 * ll, thresholdTopologyPlacement=-0.1, thresholdLogLKoptimizationTopology=ll,
              thresholdLogLKconsecutivePlacement=1.0, effectivelyNon0BLen=1.0 / (10 * dev.lRef))
    nodes = np.arange(ht.n)
    assert (dist[nodes] == 0.0).sum() >= 64
    lane = dev.spr_search_batch(nodes, search_tier=1, wide_search_budget=-1, **kw)
    sites, out = searched_twice(dev, capfd, nodes, wide_search_budget=64, **kw)
    assert "ahead" in sites, sites
    for k in EXACT:
        assert np.array_equal(out[k], lane[k]), k
    for k in ("bestScore", "blen", "improvement", "currentLK"):
        assert np.allclose(out[k], lane[k], rtol=1e-11, atol=1e-15), k
    dev.close()
