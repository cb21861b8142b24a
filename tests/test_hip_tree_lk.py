"""maple_tree_log_lk (maple_amd/csrc/tree_lk.hip): calculateTreeLikelihood (M:9721-9779) inside the library, on the tree the
library holds.  The contract is bit identity with the path it stands next to -- tree_host.tree_log_likelihood, i.e.
maple_merge_batch(returnLK) over every internal node plus maple_root_prob_batch, summed in the reference's post-order -- so every
comparison with that path below is `==`; against the unmodified reference's records the tolerances are those of the existing
tests (test_tree_log_likelihood_matches_reference, test_applied_spr_moves_tree_likelihood)."""
import numpy as np
import pytest

import test_hip_search as S
from golden_util import close, tup

pytestmark = pytest.mark.gpu
Q_SMOKE = [[-0.9, 0.2, 0.5, 0.2], [0.3, -1.4, 0.1, 1.0], [0.8, 0.1, -1.3, 0.4], [0.1, 0.6, 0.1, -0.8]]


def lk_order(tree):
    """internal nodes reachable from the root in the order the reference adds their contribution (M:9735-9770)"""
    order, stack = [], [(tree.root, False)]
    while stack:
        v, done = stack.pop()
        if not tree.children[v]:
            continue
        if done:
            order.append(v)
        else:
            stack += [(v, True), (tree.children[v][1], False), (tree.children[v][0], False)]
    return order


def merge_contributions(dev, tree):
    """(order, Lkcontribution of every node of it) through maple_merge_batch(returnLK), as tree_log_likelihood makes them"""
    order = lk_order(tree)
    mark = dev.mark()
    try:
        c0 = np.asarray([tree.children[v][0] for v in order])
        c1 = np.asarray([tree.children[v][1] for v in order])
        l0, l1 = tree.id_lower[c0].copy(), tree.id_lower[c1].copy()
        for arr, ch in ((l0, c0), (l1, c1)):
            need = np.nonzero(tree.id_mut[ch] >= 0)[0]
            if len(need):
                arr[need] = dev.pass_branch_batch(arr[need], tree.id_mut[ch[need]], True)
        dist = np.asarray(tree.dist)
        tip = np.asarray([(not c) and (m == 0) for c, m in zip(tree.children, tree.n_minor)])
        nminor = np.asarray(tree.n_minor, dtype=np.int32)
        out, lk = dev.merge_batch(l0, dist[c0], tip[c0], l1, dist[c1], tip[c1], False, returnLK=True, numMinor1=nminor[c0],
                                  numMinor2=nminor[c1])
        assert (out >= 0).all()
        return order, lk.copy()
    finally:
        dev.release(mark)


@pytest.fixture(scope="module", params=S.NAMES)
def env(request):
    """a search_* fixture uploaded, with the Python path's value on it computed once"""
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree, tree_log_likelihood
    from golden_util import model_args, ref_indices
    f = S.load(request.param)
    ctx, t = f["context"], f["tree"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
                 thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
                 defaultBLen=ctx["defaultBLen"], arena_bytes=256 << 20)
    dev.set_model(**model_args(f["model"]))
    tree = HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"], t["probVectUpRight"],
                    t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
    want = tree_log_likelihood(dev, tree)
    yield f, dev, tree, want
    dev.close()


def test_the_fixtures_cover_mat_lists_the_error_model_and_minor_sequences():
    """what test_per_node_contributions relies on: a fixture with MAT mutation lists (children and the root), one with the error
    model, and, under the error model (where numMinor enters the value, M:4489-4493), a merged child with minor sequences"""
    have_mat = have_root_mat = have_err = have_minor_under_err = have_tree_lk = False
    for name in S.NAMES:
        f = S.load(name)
        t = f["tree"]
        have_tree_lk |= "treeLK" in f
        have_mat |= any(m for v, m in enumerate(t["mutations"]) if v != t["root"])
        have_root_mat |= bool(t["mutations"][t["root"]])
        have_err |= bool(f["model"]["usingErrorRate"])
        if f["model"]["usingErrorRate"]:
            have_minor_under_err |= any(ch and (t["nMinor"][ch[0]] or t["nMinor"][ch[1]]) for ch in t["children"])
    assert have_tree_lk and have_mat and have_root_mat and have_err and have_minor_under_err


def test_reference_fixtures(env):
    from maple_amd.tree_host import tree_log_likelihood_native
    f, dev, tree, want = env
    assert "treeLK" in f
    got, got_root = tree_log_likelihood_native(dev, tree)
    print(f"native {got!r} root {got_root!r}; python path {want[0]!r} root {want[1]!r}; reference {f['treeLK']!r} root {f['rootLK']!r}")
    assert got == want[0] and got_root == want[1]
    assert close(got_root, f["rootLK"], 1e-12), (got_root, f["rootLK"])
    assert close(got, f["treeLK"], 1e-11), (got, f["treeLK"])


def test_per_node_contributions(env):
    f, dev, tree, want = env
    order, lk = merge_contributions(dev, tree)
    total, root, node = dev.tree_log_lk(tree.n_minor, per_node=True)
    assert node.shape == (tree.n,)
    assert np.array_equal(node[np.asarray(order)], lk)                    # bit for bit
    rest = np.ones(tree.n, dtype=bool)
    rest[np.asarray(order)] = False
    assert (node[rest] == 0.0).all()                                      # leaves, and slots the root does not reach
    assert all(node[v] == 0.0 for v in range(tree.n) if not tree.children[v])
    assert len(order) >= 50 and (lk != 0.0).sum() > len(order) // 2      # (identical children on zero-length branches give 0.0)
    s = 0.0
    for x in lk.tolist():
        s += x
    assert total == s + root == want[0]
    if f["model"]["usingErrorRate"]:                                      # the minor-sequence counts are read: without them another value
        assert any(tree.n_minor[tree.children[v][0]] or tree.n_minor[tree.children[v][1]] for v in order)
        assert dev.tree_log_lk(None)[0] != total


def synth_tree(tips):
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_host import HostTree
    from maple_amd.tree_mirror import TreeMirror
    d = make_dataset(n_samples=max(tips, 2), l_ref=3000, seed=5, mean_diffs=12.0, frac_with_n=0.3, frac_ambig=0.3, n_run_len=(5, 80))
    ref_idx, root_freqs = reference_tables(d.ref)
    dev = Device(ref_idx, root_freqs, arena_bytes=64 << 20)
    dev.set_model(Q_SMOKE)
    if tips == 1:                                                         # a root without children
        lst = tip_genome_list(d.diffs[0], ref_idx)
        tree = HostTree(0, [None], [[]], [0.0], [[]], [0], [lst], [None], [None], [None]).upload(dev)
        return dev, tree
    m = TreeMirror(dev, d.parent, d.blen, {int(v): tip_genome_list(dl, ref_idx) for v, dl in zip(d.tip_node, d.diffs)}).build()
    return dev, HostTree.from_mirror(m, dev)


@pytest.mark.parametrize("tips", [1, 2, 3, 257, 258])
def test_block_edges(tips):
    """1, 2, 256 and 257 internal nodes: one lane, two, a full block of 256, one lane of a second block; and no item at all"""
    from maple_amd.tree_host import tree_log_likelihood, tree_log_likelihood_native
    dev, tree = synth_tree(tips)
    got, got_root = tree_log_likelihood_native(dev, tree)
    if tips == 1:
        assert got == got_root == float(dev.root_prob_batch([tree.id_lower[0]])[0])
        assert dev.tree_log_lk(None, per_node=True)[2].tolist() == [0.0]
    else:
        assert len(lk_order(tree)) == tips - 1
        assert (got, got_root) == tree_log_likelihood(dev, tree)
    assert np.isfinite(got) and got < 0.0
    dev.close()


def test_after_a_changed_branch_length():
    """a stale cached order or stale columns would show here: the tree changes through maple_tree_patch (HostTree.sync)"""
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree, tree_log_likelihood, tree_log_likelihood_native, update_genome_lists
    from golden_util import model_args, ref_indices
    f = S.load("synth_siteerr")
    ctx, t = f["context"], f["tree"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
                 thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
                 defaultBLen=ctx["defaultBLen"], arena_bytes=256 << 20)
    dev.set_model(**model_args(f["model"]))
    tree = HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"], t["probVectUpRight"],
                    t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
    first = tree_log_likelihood_native(dev, tree)
    assert first == tree_log_likelihood(dev, tree)
    order = lk_order(tree)
    v = next(w for w in order if tree.up[w] is not None and tree.up[w] != tree.root and tree.dist[w] > 0 and not tree.mutations[w])
    tree.dist[v] = 3.0 * tree.dist[v] + 1e-4
    update_genome_lists(dev, tree, [v])
    assert tree.sync(dev) > 0                                             # patched, not uploaded again
    second = tree_log_likelihood_native(dev, tree)
    assert second == tree_log_likelihood(dev, tree)
    assert second[0] != first[0]
    dev.close()


@pytest.mark.parametrize("name", S.E2E_NAMES)
def test_after_one_online_addition(name):
    """the recorded placement of one more sample: the patch adds nodes (two on every fixture here, unless the sample became a
    minor sequence, which changes a tip flag and a count instead)"""
    from maple_amd.tree_host import tree_log_likelihood, tree_log_likelihood_native, update_genome_lists
    from golden_util import model_args
    f, dev = S._e2e_env(name)
    dev.set_model(**model_args(f["model"]))
    tree = S._tree_from_topology(dev, f["online_start"], f["tips"])
    tree.upload_topology(dev)
    first = tree_log_likelihood_native(dev, tree)
    assert first == tree_log_likelihood(dev, tree)
    assert close(first[0], f["online_start_LK"], 1e-9), (first[0], f["online_start_LK"])
    n_before = tree.n
    for rec in f["online"]:                                               # (in order, up to the first that adds nodes: usually the first)
        after = rec["after"]
        changed = tree.apply_topology(after["root"], after["up"], after["children"], after["dist"], after["nMinor"], after.get("mutations"), dev)
        for v, lst in rec["new_tips"].items():
            tree.id_lower[int(v)] = dev.upload([tup(lst)])[0]
            if int(v) not in changed:
                changed.append(int(v))
        if changed:
            update_genome_lists(dev, tree, changed)
        how = tree.sync(dev)
        if tree.n > n_before:
            break
    assert tree.n > n_before and dev.n_nodes == tree.n
    second = tree_log_likelihood_native(dev, tree)
    print(f"{name}: sync -> {how}; {first[0]!r} -> {second[0]!r}")
    assert second == tree_log_likelihood(dev, tree)
    assert second[0] != first[0]
    node = dev.tree_log_lk(tree.n_minor, per_node=True)[2]
    order, lk = merge_contributions(dev, tree)
    assert any(v >= n_before for v in order)                              # the new internal node is among the items
    assert len(node) == tree.n and np.array_equal(node[np.asarray(order)], lk)
    assert all(node[v] == 0.0 for v in range(tree.n) if not tree.children[v])
    dev.close()


def test_arena_neutral_and_repeatable(env):
    f, dev, tree, want = env
    assert any(tree.mutations)                                            # (every search_* fixture has MAT lists: temporaries are made)
    before = dev.stats()
    a = dev.tree_log_lk(tree.n_minor)
    assert dev.stats() == before
    b = dev.tree_log_lk(tree.n_minor)
    assert dev.stats() == before
    assert a == b == want
    mark = dev.mark()                                                     # between a mark and its release of the caller
    extra = dev.upload([tup(f["tree"]["probVect"][tree.root])])
    inside = dev.stats()
    c = dev.tree_log_lk(tree.n_minor)
    assert dev.stats() == inside and c == want
    assert dev.download(extra)[0] is not None
    dev.release(mark)
    assert dev.stats() == before
    assert dev.tree_log_lk(tree.n_minor) == want


def test_after_applied_moves():
    from maple_amd.tree_host import tree_log_likelihood_native
    name = next(n for n in S.E2E_NAMES if S._has_moves(n))
    f, dev = S._e2e_env(name)
    assert len(f["spr_moves"]) >= 5
    for k, mv in enumerate(f["spr_moves"][:5]):
        dev.set_model(mv["Q"])
        mark = dev.mark()
        tree = S._tree_from_topology(dev, mv["after"], f["tips"])
        tree.upload_topology(dev)                                         # (the rebuilt lists' ids: the library's copy is the caller's job)
        lk, _ = tree_log_likelihood_native(dev, tree)
        dev.release(mark)
        print(f"{name} move {k}: {lk!r} reference {mv['lk_after_fresh']!r}")
        assert close(lk, mv["lk_after_fresh"], 1e-9), (k, lk, mv["lk_after_fresh"])
    dev.close()


def test_errors():
    from maple_amd.abi import MapleError
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree, tree_log_likelihood, tree_log_likelihood_native
    ref = "acgtacgtacgtacgtacgt"
    ref_idx, root_freqs = reference_tables(ref)
    dev = Device(ref_idx, root_freqs, arena_bytes=16 << 20)
    dev.set_model(Q_SMOKE)
    with pytest.raises(MapleError) as e:                                  # no tree yet
        dev.tree_log_lk()
    assert e.value.code == MapleError.ERR_STATE
    # nodes 0 and 1: tips with t and c at site 7 (the reference has g there), both on zero-length branches below the root, node 2:
    # mergeVectors has no result (M:4757-4762)
    la, lb = tip_genome_list([("t", 7)], ref_idx), tip_genome_list([("c", 7)], ref_idx)
    assert la != lb
    tree = HostTree(2, [2, 2, None], [[], [], [0, 1]], [0.0, 0.0, 0.0], [[], [], []], [0, 0, 0], [la, lb, la], [None] * 3, [None] * 3,
                    [None] * 3).upload(dev)
    before = dev.stats()
    with pytest.raises(MapleError) as e:
        tree_log_likelihood_native(dev, tree)
    assert e.value.code == MapleError.ERR_FATAL and "node 2" in str(e.value), str(e.value)
    assert dev.stats() == before
    tree.dist[0] = tree.dist[1] = 1e-3                                    # the same tree with room for the difference
    tree.upload_topology(dev)
    got = tree_log_likelihood_native(dev, tree)
    assert got == tree_log_likelihood(dev, tree) and np.isfinite(got[0])
    dev.close()


def test_with_announced_samples():
    """announce, place one sample, maple_tree_log_lk, place the next: the rows made ahead go on as without the call"""
    from maple_amd.tree_host import tree_log_likelihood, tree_log_likelihood_native, update_genome_lists
    from golden_util import model_args
    import gzip
    import json
    import os
    name = next(n for n in S.E2E_NAMES if not S._has_mat(json.load(gzip.open(os.path.join(S.GOLDEN, f"e2e_{n}.json.gz"), "rt"))))

    def run(announce, with_lk):
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
        outs, lk = [], None
        for k, rec in enumerate(recs[:2]):
            tree.sync(dev)
            dev.placement_prepare(**pkw)
            if k == 0 and announce:
                assert dev.placement_ahead(np.asarray(qids, dtype=np.int32), **pkw) == len(qids)
            if k == 1 and with_lk:
                lk = tree_log_likelihood_native(dev, tree)
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
        if with_lk:
            assert lk == tree_log_likelihood(dev, tree)                   # (the tree has not changed since the call)
        dev.close()
        return outs, {k: s1[k] - s0[k] for k in ("searches", "fallbacks", "expanded_items")}, lk

    with_call, rows_with, lk = run(True, True)
    without_call, rows_without, _ = run(True, False)
    plain, rows_plain, _ = run(False, False)
    assert lk is not None and np.isfinite(lk[0])
    assert rows_with == rows_without and rows_with["searches"] == 2 and rows_plain["searches"] == 0
    for a, b, c in zip(with_call, without_call, plain):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
        for key in ("bestNode", "bestScore", "blen", "status"):           # the placement itself: that of the search without rows
            assert np.array_equal(a[key], c[key]), key
