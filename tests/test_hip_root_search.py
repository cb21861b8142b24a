"""maple_tree_find_best_root (maple_amd/csrc/root_search.hip): the search of findBestRoot (M:7730-7848) inside the library, on the
tree the library holds.  The contract is bit identity with the path it stands next to -- tree_host.find_best_root, i.e. per level
five maple_merge_batch(returnLK) launches, the passes through reference branches and maple_root_prob_batch, then the replay of the
reference's traversal -- so every comparison with that path below is `==`; against the unmodified reference's records the
tolerances are those of test_find_best_root_matches_reference."""
import math

import numpy as np
import pytest

import test_hip_search as S
from golden_util import close, model_args, ref_indices, tup

pytestmark = pytest.mark.gpu
Q_SMOKE = [[-0.9, 0.2, 0.5, 0.2], [0.3, -1.4, 0.1, 1.0], [0.8, 0.1, -1.3, 0.4], [0.1, 0.6, 0.1, -0.8]]
EVERY = dict(strictTopologyStopRules=False, allowedFailsTopology=1 << 30, thresholdLogLKtopology=1.0,
             thresholdLogLKoptimizationTopology=math.inf, thresholdLogLKconsecutivePlacement=1.0)
USUAL = dict(strictTopologyStopRules=True, allowedFailsTopology=2, thresholdLogLKtopology=10.0,
             thresholdLogLKoptimizationTopology=1.0, thresholdLogLKconsecutivePlacement=0.01)


def fixture_device(f):
    from maple_amd.runtime import Device
    ctx = f["context"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
                 thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
                 defaultBLen=ctx["defaultBLen"], arena_bytes=256 << 20)
    dev.set_model(**model_args(f["model"]))
    return dev


def fixture_tree(f, dev):
    from maple_amd.tree_host import HostTree
    t = f["tree"]
    return HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"], t["probVectUpRight"],
                    t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)


def recorded_sets(f):
    ctx = f["context"]
    return [dict(strictTopologyStopRules=rec["strict"], allowedFailsTopology=rec["fails"], thresholdLogLKtopology=rec["thr"],
                 thresholdLogLKoptimizationTopology=ctx["thresholdLogLKoptimizationTopology"],
                 thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"]) for rec in S.load_update(f["name"])["find_best_root"]]


def same(a, b):
    """two 4-tuples of find_best_root, bit for bit, the dicts in the same order"""
    return (a[0] == b[0] and a[3] == b[3] and float(a[1]).hex() == float(b[1]).hex()
            and [(k, float(v).hex()) for k, v in a[2].items()] == [(k, float(v).hex()) for k, v in b[2].items()])


def below_roots_children(tree):
    """the branches the level loop scores when nothing is abandoned: every node at depth >= 2"""
    out, stack = [], [(c, 1) for c in tree.children[tree.root]]
    while stack:
        v, d = stack.pop()
        if d >= 2:
            out.append(v)
        stack += [(c, d + 1) for c in tree.children[v]]
    return sorted(out)


@pytest.fixture(scope="module", params=S.NAMES)
def env(request):
    """a search_* fixture uploaded, with the Python path's answers on it computed once: per recorded parameter set, and with rules
    that keep every scored branch"""
    from maple_amd.tree_host import find_best_root
    f = S.load(request.param)
    dev = fixture_device(f)
    tree = fixture_tree(f, dev)
    sets = recorded_sets(f)
    want = [find_best_root(dev, tree, **kw) for kw in sets]
    every = find_best_root(dev, tree, **EVERY)
    yield f, dev, tree, sets, want, every
    dev.close()


def test_recorded_parameter_sets(env):
    from maple_amd.tree_host import find_best_root_native
    f, dev, tree, sets, want, _ = env
    recs = S.load_update(f["name"])["find_best_root"]
    assert len(sets) == len(recs) == 2
    for kw, py, rec in zip(sets, want, recs):
        got = find_best_root_native(dev, tree, **kw)
        print(f"{f['name']}: native {got[0]} {got[1]!r} visited {got[3]} kept {len(got[2])}; python path {py[0]} {py[1]!r}; "
              f"reference {rec['bestNode']} {rec['bestLKdiff']!r} visited {rec['visited']}")
        assert same(got, py), (got[0], got[1], got[3], py[0], py[1], py[3])
        assert list(got[2])[0] == tree.root and got[2][tree.root] == 0.0
        assert got[0] == rec["bestNode"] and got[3] == rec["visited"]
        assert close(got[1], rec["bestLKdiff"], 1e-9, 1e-9)
        ref = {int(k): v for k, v in rec["bestNodes"].items()}
        assert set(got[2]) == set(ref) and len(ref) > 50
        assert all(close(got[2][k], ref[k], 1e-7, 1e-7) for k in ref)


def test_every_score(env):
    f, dev, tree, _, _, every = env
    best, diff, visited, score, nodes, scores, n_best = dev.tree_find_best_root(tree.n_minor, **EVERY)
    assert n_best == len(nodes) == len(every[2]) and (best, visited) == (every[0], every[3]) and diff == every[1]
    scored = np.nonzero(~np.isnan(score))[0]
    py = dict(every[2])
    assert py.pop(tree.root) == 0.0 and nodes[0] == tree.root and scores[0] == 0.0
    assert sorted(py) == scored.tolist() and len(py) > 50
    assert all(float(score[v]).hex() == float(x).hex() for v, x in py.items())                      # the same bits
    assert [(int(v), float(x).hex()) for v, x in zip(nodes[1:], scores[1:])] == [(v, float(x).hex()) for v, x in py.items()]
    # NaN exactly for the root, its children and what the root does not reach (nothing is abandoned on the fixtures)
    assert scored.tolist() == below_roots_children(tree)


def test_the_fixtures_cover_both_root_probability_paths_and_the_models():
    """what the tests above rely on: mutation lists on children and on the root (newRootProbVect is materialised and passed up),
    items with no mutation list up to the root (the sink: no search_* fixture is free of mutation lists altogether, the
    synthetic trees below are), the error model, and minor sequences under the error model"""
    have_mat_items = have_sink_items = have_root_mat = have_child_mat = have_err = have_minor_under_err = False
    for name in S.NAMES:
        f = S.load(name)
        t = f["tree"]
        ch, mu, root = t["children"], t["mutations"], t["root"]
        have_root_mat |= bool(mu[root])
        have_child_mat |= any(m for v, m in enumerate(mu) if v != root)
        stack = [(c, bool(mu[root])) for c in ch[root]]
        while stack:
            v, m = stack.pop()
            m = m or bool(mu[v])
            if ch[v]:
                have_mat_items |= m
                have_sink_items |= not m
                stack += [(c, m) for c in ch[v]]
        have_err |= bool(f["model"]["usingErrorRate"])
        if f["model"]["usingErrorRate"]:
            have_minor_under_err |= any(t["nMinor"])
    assert have_mat_items and have_sink_items and have_root_mat and have_child_mat and have_err and have_minor_under_err


def test_minor_sequences_are_read_under_the_error_model():
    names = [nm for nm in S.NAMES if S.load(nm)["model"]["usingErrorRate"] and any(S.load(nm)["tree"]["nMinor"])]
    assert names
    for nm in names:
        f = S.load(nm)
        dev = fixture_device(f)
        tree = fixture_tree(f, dev)
        with_counts = dev.tree_find_best_root(tree.n_minor, **EVERY)
        without = dev.tree_find_best_root(None, **EVERY)
        assert with_counts[1] != without[1] or not np.array_equal(with_counts[3], without[3], equal_nan=True), nm
        dev.close()


# ---- hand-made trees --------------------------------------------------------------------------------------------------------------
def synth_device(l_ref_data, rate_variation=False):
    from maple_amd.host import reference_tables
    from maple_amd.runtime import Device
    ref_idx, root_freqs = reference_tables(l_ref_data.ref)
    dev = Device(ref_idx, root_freqs, arena_bytes=256 << 20)
    if rate_variation:
        dev.set_model(**S._model_for("ratevar", len(ref_idx)))
    else:
        dev.set_model(Q_SMOKE)
    return dev, ref_idx


def synth_tree(tips, parent=None, blen=None, rate_variation=False):
    """tips samples of the synthetic generator on its own tree, or on the topology ``parent`` / ``blen`` (parents precede children)"""
    from maple_amd.host import tip_genome_list
    from maple_amd.synth import make_dataset
    from maple_amd.tree_host import HostTree
    from maple_amd.tree_mirror import TreeMirror
    d = make_dataset(n_samples=max(tips, 2), l_ref=3000, seed=5, mean_diffs=12.0, frac_with_n=0.3, frac_ambig=0.3, n_run_len=(5, 80),
                     rate_variation=rate_variation)
    dev, ref_idx = synth_device(d, rate_variation)
    if tips == 1:                                                         # a root without children
        tree = HostTree(0, [None], [[]], [0.0], [[]], [0], [tip_genome_list(d.diffs[0], ref_idx)], [None], [None], [None]).upload(dev)
        return dev, tree
    if parent is None:
        m = TreeMirror(dev, d.parent, d.blen, {int(v): tip_genome_list(dl, ref_idx) for v, dl in zip(d.tip_node, d.diffs)}).build()
    else:
        leaves = [v for v in range(len(parent)) if v not in set(parent)]
        assert len(leaves) == tips
        m = TreeMirror(dev, parent, blen, {v: tip_genome_list(dl, ref_idx) for v, dl in zip(leaves, d.diffs)}).build()
    return dev, HostTree.from_mirror(m, dev)


def caterpillar(tips):
    """internal node i is node 2i, its tip 2i + 1, the last tip 2(tips - 1)"""
    m = tips - 1
    parent = [-1] + [0] * (2 * m)
    for i in range(m):
        parent[2 * i + 1] = 2 * i
        parent[2 * i + 2] = 2 * i
    return parent, [0.0] + [2e-4 + 1e-5 * (v % 7) for v in range(1, 2 * m + 1)]


def level_sizes(tree):
    sizes, cur = [], [c for c in tree.children[tree.root] if tree.children[c]]
    while cur:
        sizes.append(len(cur))
        cur = [c for v in cur for c in tree.children[v] if tree.children[c]]
    return sizes


@pytest.mark.parametrize("shape", ["root_alone", "two_tips", "five_nodes", "tips_3000_ratevar", "caterpillar_300"])
def test_smallest_shapes(shape):
    from maple_amd.tree_host import find_best_root, find_best_root_native
    if shape == "root_alone":
        dev, tree = synth_tree(1)
    elif shape == "two_tips":
        dev, tree = synth_tree(2)
    elif shape == "five_nodes":                                            # one internal child: one item, two sides
        dev, tree = synth_tree(3, parent=[-1, 0, 0, 1, 1], blen=[0.0, 3e-4, 2e-4, 1e-4, 5e-4])
        assert level_sizes(tree) == [1]
    elif shape == "tips_3000_ratevar":
        dev, tree = synth_tree(3000, rate_variation=True)                  # (2 000 tips: no level above 219 items)
        sizes = level_sizes(tree)
        print("levels:", sizes)
        assert max(sizes) > 256 and min(sizes) <= 2                        # more than one block of lanes in every kernel; nearly empty levels
    else:
        dev, tree = synth_tree(300, *caterpillar(300))
        assert level_sizes(tree) == [1] * 298
    for kw in (EVERY, USUAL):
        py = find_best_root(dev, tree, **kw)
        before = dev.stats()
        got = find_best_root_native(dev, tree, **kw)
        assert dev.stats() == before
        assert same(got, py), (shape, got[0], got[1], got[3], py[0], py[1], py[3])
    if shape in ("root_alone", "two_tips"):
        assert (got[0], got[1], got[3]) == (tree.root, 0.0, 1) and got[2] == {tree.root: 0.0}
        assert np.isnan(dev.tree_find_best_root(None, **EVERY)[3]).all()
    else:
        score = dev.tree_find_best_root(None, **EVERY)[3]
        assert np.nonzero(~np.isnan(score))[0].tolist() == below_roots_children(tree)
        assert len(find_best_root(dev, tree, **EVERY)[2]) == 1 + len(below_roots_children(tree))
    dev.close()


def abandoned_tree(dev, ref_idx):
    """root 8 -> (A = 4, X = 7); A -> (B = 2, C = 3); B -> (0, 1); X -> (5, 6).  C shows t at site 7 (the reference has g there) and
    both tips below X show c; the branches above A, C and X have length zero.  At A what comes from above is X's list, c at no
    distance: rooting above B merges it with C's t over a distance of zero, which has no result (M:4757-4762), and rooting above C
    meets the same pair one merge later -- both sides of A are abandoned and nothing below B is scored.  The two branches below X
    are: its tips sit at a distance."""
    from maple_amd.host import tip_genome_list
    from maple_amd.tree_host import HostTree
    lc, lx = tip_genome_list([("t", 7)], ref_idx), tip_genome_list([("c", 7)], ref_idx)
    l0, l1 = tip_genome_list([("a", 3)], ref_idx), tip_genome_list([("t", 12)], ref_idx)
    up = [2, 2, 4, 4, 8, 7, 7, 8, None]
    children = [[], [], [0, 1], [], [2, 3], [], [], [5, 6], [4, 7]]
    dist = [1e-3, 2e-3, 1e-3, 0.0, 0.0, 1e-3, 2e-3, 0.0, 0.0]
    tree = HostTree(8, up, children, dist, [[] for _ in range(9)], [0] * 9, [l0, l1, l0, lc, l0, lx, lx, l0, l0], [None] * 9, [None] * 9,
                    [None] * 9).upload(dev)
    for v in (2, 4, 7, 8):                                                 # the internal nodes' lower lists, bottom up
        a, b = children[v]
        ids = dev.merge_batch([tree.id_lower[a]], [dist[a]], [not children[a]], [tree.id_lower[b]], [dist[b]], [not children[b]], False)
        assert (ids[0] >= 0) == (v != 8)                                   # (the root's own merge has no result either: it keeps a stand-in)
        if ids[0] >= 0:
            tree.id_lower[v] = ids[0]
    return tree.upload_topology(dev)


def test_an_abandoned_rooting():
    from maple_amd.host import reference_tables
    from maple_amd.runtime import Device
    from maple_amd.tree_host import find_best_root, find_best_root_native
    ref_idx, root_freqs = reference_tables("acgtacgtacgtacgtacgt")
    dev = Device(ref_idx, root_freqs, arena_bytes=16 << 20)
    dev.set_model(Q_SMOKE)
    tree = abandoned_tree(dev, ref_idx)
    py = find_best_root(dev, tree, **EVERY)
    assert below_roots_children(tree) == [0, 1, 2, 3, 5, 6]
    assert sorted(py[2]) == [5, 6, 8]                                      # fewer than the six branches below the root's children
    before = dev.stats()
    got = find_best_root_native(dev, tree, **EVERY)                        # (it returns: MAPLE_OK)
    assert dev.stats() == before
    assert same(got, py)
    score = dev.tree_find_best_root(None, **EVERY)[3]
    assert np.isnan(score[[2, 3]]).all() and np.isnan(score[[0, 1]]).all()     # the abandoned branches, and those below one
    assert score[5] == py[2][5] and score[6] == py[2][6] and np.isnan(score[[4, 7, 8]]).all()
    dev.close()


def test_after_tree_patch():
    """a stale plan or stale columns would show here: a recorded branch-length change goes in through maple_tree_patch"""
    from maple_amd.tree_host import find_best_root, find_best_root_native, update_genome_lists
    f = S.load("synth_siteerr")
    dev = fixture_device(f)
    tree = fixture_tree(f, dev)
    kw = recorded_sets(f)[1]
    first = find_best_root_native(dev, tree, **kw)
    assert same(first, find_best_root(dev, tree, **kw))
    first_scores = dev.tree_find_best_root(tree.n_minor, **EVERY)[3]
    case = next(c for c in S.load_update("synth_siteerr")["cases"] if c["change"]["kind"] == "dist" and c["change"]["node"] != tree.root
                and c["change"]["dist"] != tree.dist[c["change"]["node"]])
    v = case["change"]["node"]
    tree.dist[v] = case["change"]["dist"]
    update_genome_lists(dev, tree, [v])
    assert tree.sync(dev) > 0                                              # patched, not uploaded again
    second = find_best_root_native(dev, tree, **kw)
    assert same(second, find_best_root(dev, tree, **kw))
    a = dev.tree_find_best_root(tree.n_minor, **EVERY)[3]
    tree.upload_topology(dev)
    b = dev.tree_find_best_root(tree.n_minor, **EVERY)[3]
    assert np.array_equal(a, b, equal_nan=True)                            # the patched tree is the uploaded one
    assert not np.array_equal(a, first_scores, equal_nan=True)             # the change is seen
    dev.close()


def test_arena_neutral_and_repeatable(env):
    f, dev, tree, sets, want, _ = env
    before = dev.stats()
    a = dev.tree_find_best_root(tree.n_minor, **sets[0])
    assert dev.stats() == before
    b = dev.tree_find_best_root(tree.n_minor, **sets[0])
    assert dev.stats() == before
    assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2] and a[6] == b[6]
    assert np.array_equal(a[3], b[3], equal_nan=True) and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
    mark = dev.mark()                                                      # between a mark and its release of the caller
    extra = dev.upload([tup(f["tree"]["probVect"][tree.root])])
    inside = dev.stats()
    c = dev.tree_find_best_root(tree.n_minor, **sets[0])
    assert dev.stats() == inside and np.array_equal(a[3], c[3], equal_nan=True)
    assert dev.download(extra)[0] is not None
    dev.release(mark)
    assert dev.stats() == before


def test_with_announced_samples():
    """announce, place one sample, maple_tree_find_best_root, place the next: the rows made ahead go on as without the call"""
    from maple_amd.tree_host import find_best_root, find_best_root_native, update_genome_lists
    import gzip
    import json
    import os
    name = next(n for n in S.E2E_NAMES if not S._has_mat(json.load(gzip.open(os.path.join(S.GOLDEN, f"e2e_{n}.json.gz"), "rt"))))

    def run(announce, with_call):
        f, dev = S._e2e_env(name)
        ctx = f["context"]
        dev.set_model(**model_args(f["model"]))
        tree = S._tree_from_topology(dev, f["online_start"], f["tips"])
        pkw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"], thresholdLogLK=ctx["thresholdLogLK"],
                   thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
                   thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], allowedFails=ctx["allowedFails"],
                   strictStopRules=ctx["strictStopRules"])
        tree.upload_topology(dev)
        recs = f["online"][:3]
        qids = [int(x) for x in dev.upload([tup(r["query"]) for r in recs])]
        s0 = dev.placement_ahead_stats()
        outs, res = [], None
        for k, rec in enumerate(recs[:2]):
            tree.sync(dev)
            dev.placement_prepare(**pkw)
            if k == 0 and announce:
                assert dev.placement_ahead(np.asarray(qids, dtype=np.int32), **pkw) == len(qids)
            if k == 1 and with_call:
                res = find_best_root_native(dev, tree, **USUAL)
            mark = dev.mark()
            out = dev.placement_search_batch(np.asarray([qids[k]], dtype=np.int32), **pkw)
            dev.release(mark)
            outs.append({kk: vv.copy() for kk, vv in out.items()})
            assert int(out["bestNode"][0]) == rec["ret"]["bestNode"]
            if k == 0:
                after = rec["after"]
                changed = tree.apply_topology(after["root"], after["up"], after["children"], after["dist"], after["nMinor"],
                                              after.get("mutations"), dev)
                for v, lst in rec["new_tips"].items():
                    tree.id_lower[int(v)] = dev.upload([tup(lst)])[0]
                    if int(v) not in changed:
                        changed.append(int(v))
                update_genome_lists(dev, tree, changed)
        s1 = dev.placement_ahead_stats()
        if with_call:
            assert same(res, find_best_root(dev, tree, **USUAL))           # (the tree has not changed since the call)
        dev.close()
        return outs, {k: s1[k] - s0[k] for k in ("searches", "fallbacks", "expanded_items")}, res

    with_call, rows_with, res = run(True, True)
    without_call, rows_without, _ = run(True, False)
    assert res is not None and res[3] > 1
    assert rows_with == rows_without and rows_with["searches"] == 2
    for a, b in zip(with_call, without_call):
        for key in a:
            assert np.array_equal(a[key], b[key]), key


def test_errors_and_capacity(env):
    from maple_amd.abi import MapleError
    f, dev, tree, sets, want, every = env
    with pytest.raises(MapleError) as e:
        dev.tree_find_best_root(tree.n_minor, struct_size=0, **sets[0])
    assert e.value.code == MapleError.ERR_ARG
    bad = np.asarray(tree.n_minor, dtype=np.int32).copy()
    bad[tree.root] = -1
    with pytest.raises(MapleError) as e:
        dev.tree_find_best_root(bad, **sets[0])
    assert e.value.code == MapleError.ERR_ARG
    full = dev.tree_find_best_root(tree.n_minor, **EVERY)
    cut = dev.tree_find_best_root(tree.n_minor, cap_best=5, **EVERY)
    assert cut[6] == full[6] == len(every[2]) > 5 and len(cut[4]) == 5
    assert np.array_equal(cut[4], full[4][:5]) and np.array_equal(cut[5], full[5][:5]) and cut[:3] == full[:3]
    none = dev.tree_find_best_root(tree.n_minor, cap_best=0, **EVERY)
    assert none[6] == full[6] and len(none[4]) == 0 and none[:3] == full[:3]
    # a struct that ends before thresholdLogLKconsecutivePlacement is read for what it has: that threshold is 0.0
    short = dev.tree_find_best_root(tree.n_minor, struct_size=32, **sets[0])
    zero = dev.tree_find_best_root(tree.n_minor, **dict(sets[0], thresholdLogLKconsecutivePlacement=0.0))
    assert short[:3] == zero[:3] and np.array_equal(short[4], zero[4])


def test_errors_without_a_tree_or_a_model():
    from maple_amd.abi import MapleError
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree
    ref_idx, root_freqs = reference_tables("acgtacgtacgtacgtacgt")
    fresh = Device(ref_idx, root_freqs, arena_bytes=16 << 20)
    with pytest.raises(MapleError) as e:                                  # no tree (and no model) yet
        fresh.tree_find_best_root(None, **USUAL)
    assert e.value.code == MapleError.ERR_STATE
    fresh.set_model(Q_SMOKE)
    with pytest.raises(MapleError) as e:                                  # a model, still no tree
        fresh.tree_find_best_root(None, **USUAL)
    assert e.value.code == MapleError.ERR_STATE
    fresh.close()
    nomodel = Device(ref_idx, root_freqs, arena_bytes=16 << 20)
    la, lb = tip_genome_list([("t", 7)], ref_idx), tip_genome_list([("c", 7)], ref_idx)
    HostTree(2, [2, 2, None], [[], [], [0, 1]], [1e-3, 1e-3, 0.0], [[], [], []], [0, 0, 0], [la, lb, la], [None] * 3, [None] * 3,
             [None] * 3).upload(nomodel)
    with pytest.raises(MapleError) as e:                                  # a tree, no model
        nomodel.tree_find_best_root(None, **USUAL)
    assert e.value.code == MapleError.ERR_STATE
    nomodel.set_model(Q_SMOKE)                                            # ... and with one: a root whose children are both leaves
    assert nomodel.tree_find_best_root(None, **USUAL)[:3] == (2, 0.0, 1)
    nomodel.close()
