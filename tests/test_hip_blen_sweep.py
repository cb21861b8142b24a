"""maple_tree_optimize_blens (maple_amd/csrc/blen_sweep.hip): traverseTreeToOptimizeBranchLengths inside the library, against
the unmodified reference's records -- the first sweep (update_*.json.gz: blen_full_sweeps, blen_sweeps), successive sweeps from
the dirty flags the one before left (blen_rounds_*.json.gz) -- against the Python sweep of maple_amd/tree_host.py, and against
itself under every scheduling choice.  Fixture trees only (120-1 199 nodes)."""
import ctypes as C
import functools
import gzip
import json
import os

import numpy as np
import pytest

from golden_util import GOLDEN, close, model_args, ref_indices

pytestmark = pytest.mark.gpu
NAMES = sorted(f[len("update_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("update_"))
MAT_NAMES = [n for n in NAMES if n.startswith(("b1429_", "synth_"))]


@functools.lru_cache(maxsize=None)
def load(kind, name):
    with gzip.open(os.path.join(GOLDEN, f"{kind}_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


def make(name, dist_in, rebuild=True, set_model=True):
    """a Device and the fixture tree with the lengths dist_in, its lists recomputed for them (as the reference did)"""
    from maple_amd.runtime import Device
    from maple_amd.tree_host import HostTree, rebuild_genome_lists
    f = load("search", name)
    ctx, t = f["context"], f["tree"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
                 thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
                 defaultBLen=ctx["defaultBLen"], arena_bytes=512 << 20)
    if set_model:
        dev.set_model(**model_args(f["model"]))
    tree = HostTree(t["root"], t["up"], t["children"], list(dist_in), t["mutations"], t["nMinor"], t["probVect"], t["probVectUpRight"],
                    t["probVectUpLeft"], t["probVectTotUp"]).upload(dev)
    if rebuild:
        tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp = rebuild_genome_lists(dev, tree)
    return dev, tree


def swept(tree):
    """the nodes the sweep visits: everything below the root's children"""
    kids = set(tree.children[tree.root])
    return [v for v in tree.preorder() if v != tree.root and v not in kids]


def check_lengths(tree, want, reach, rel=1e-6, abs_=1e-12):
    bad = [(v, float(tree.dist[v]), want[v]) for v in reach if not close(float(tree.dist[v]), want[v], rel, abs_)]
    assert not bad, bad[:5]


def dirty_diff(got, want, reach):
    """nodes of `reach` whose flag differs: (set in the library only, set in the reference only)"""
    return sorted(v for v in reach if got[v] and not want[v]), sorted(v for v in reach if want[v] and not got[v])


# ---- 1. the first sweep, every node dirty ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["converged", "perturbed"])
@pytest.mark.parametrize("name", NAMES)
def test_first_sweep_matches_reference(name, which):
    from maple_amd.tree_host import optimize_branch_lengths_native, tree_log_likelihood
    upd = load("update", name)
    rec = upd["blen_full_sweeps"][which]
    dev, tree = make(name, rec["dist_in"])
    lk_in, _ = tree_log_likelihood(dev, tree)
    assert close(lk_in, rec["treeLK_in"], 1e-9), (lk_in, rec["treeLK_in"])
    updates, dirty, order = optimize_branch_lengths_native(dev, tree, upd["effectivelyNon0BLen"])
    lk_out, _ = tree_log_likelihood(dev, tree)
    reach = tree.preorder()
    print(f"{name}[{which}]: {updates} updates (reference {rec['updates']}), LK {lk_in:.6f} -> {lk_out:.6f} (reference "
          f"{rec['treeLK_out']:.6f}), dirty out {sum(dirty[v] for v in reach)} (reference {sum(rec['dirty_out'][v] for v in reach)}), "
          f"dirty difference {dirty_diff(dirty, rec['dirty_out'], reach)}, stats {dev.optimize_blens_stats()}")
    assert updates == rec["updates"]
    assert order == rec["update_order"]
    check_lengths(tree, rec["dist_out"], reach)
    assert close(lk_out, rec["treeLK_out"], 1e-9), (lk_out, rec["treeLK_out"])
    assert dirty_diff(dirty, rec["dirty_out"], reach) == ([], [])
    # maple_update_partials_touched: the union over the sweep
    touched = set(dev.update_partials_touched(cap=tree.n).tolist())
    assert set(order) <= touched
    dev.close()


# ---- 3. successive sweeps, each from the flags the one before left ------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_successive_sweeps_match_reference(name):
    from maple_amd.tree_host import optimize_branch_lengths_native, tree_log_likelihood
    rounds = load("blen_rounds", name)
    assert 2 <= len(rounds["sweeps"]) <= 21 and rounds["sweeps"][-1]["updates"] == 0
    dev, tree = make(name, rounds["dist_in"])
    reach = tree.preorder()
    lk_in, _ = tree_log_likelihood(dev, tree)
    assert close(lk_in, rounds["treeLK_in"], 1e-9), (lk_in, rounds["treeLK_in"])
    want_dist = list(rounds["dist_in"])
    dirty = None
    for k, rec in enumerate(rounds["sweeps"]):
        want_in, want_out = set(rec["dirty_in"]), set(rec["dirty_out"])
        if dirty is not None:
            assert dirty_diff(dirty, [v in want_in for v in range(tree.n)], reach) == ([], []), k
        updates, dirty, order = optimize_branch_lengths_native(dev, tree, rounds["effectivelyNon0BLen"], dirty=dirty)
        lk, _ = tree_log_likelihood(dev, tree)
        diff = dirty_diff(dirty, [v in want_out for v in range(tree.n)], reach)
        print(f"{name} sweep {k + 1}: {updates} updates (reference {rec['updates']}), LK {lk:.6f} (reference {rec['treeLK']:.6f}), "
              f"dirty difference {diff}")
        assert updates == rec["updates"], k
        assert order == rec["update_order"], k
        for v, d in rec["dist_changed"].items():
            want_dist[int(v)] = d
        check_lengths(tree, want_dist, reach)
        assert close(lk, rec["treeLK"], 1e-9), (k, lk, rec["treeLK"])
        assert diff == ([], []), k
    assert updates == 0
    dev.close()


# ---- 4. the fast pass: every dirty branch from the frozen lists ----------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["converged", "perturbed"])
@pytest.mark.parametrize("name", NAMES)
def test_fast_pass_matches_reference(name, which):
    from maple_amd.tree_host import optimize_branch_lengths_native
    upd = load("update", name)
    rec = upd["blen_sweeps"][which]
    dev, tree = make(name, rec["dist_in"], rebuild=False)                   # (the reference left the lists as they were)
    ids = [a.copy() for a in (tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp)]
    lists_before = dev.download(np.concatenate([a[a >= 0] for a in ids]))
    n_lists = dev.stats()["n_lists"]
    updates, dirty, order = optimize_branch_lengths_native(dev, tree, upd["effectivelyNon0BLen"], fast_pass=True)
    assert dev.stats()["n_lists"] == n_lists                               # the estimates allocate nothing, the grid search gives back
    assert updates == rec["updates"]
    reach = tree.preorder()
    check_lengths(tree, rec["dist_out"], reach, 1e-7, 1e-15)
    low = swept(tree)
    assert [dirty[v] for v in low] == [rec["dirty_out"][v] for v in low]
    for a, b in zip(ids, (tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp)):
        assert np.array_equal(a, b)
    assert dev.download(np.concatenate([a[a >= 0] for a in ids])) == lists_before
    moved = [v for v in low if float(tree.dist[v]) != float(rec["dist_in"][v])]
    assert sorted(v for v in order if v in set(low)) == sorted(moved) and len(moved) == updates   # order: the nodes whose length changed
    assert dev.optimize_blens_stats()["repairs"] == 0
    dev.close()


# ---- 5. scheduling never changes results ---------------------------------------------------------------------------------------------
SCHEDULES = {"chunk1": dict(chunk=1), "chunk7": dict(chunk=7), "chunk256": dict(chunk=256), "adaptive": dict(chunk=0),
             "lanes": dict(chunk=0, wave=-1), "waves": dict(chunk=0, wave=1 << 20), "chunk256_lanes": dict(chunk=256, wave=-1)}
_sched = {}


def three_sweeps(name, chunk, wave=0):
    from maple_amd.tree_host import optimize_branch_lengths_native
    rec = load("update", name)["blen_full_sweeps"][1]
    dev, tree = make(name, rec["dist_in"])
    if wave:
        dev.set_tuning(wave_per_item_max=wave)
    out, dirty = [], None
    for _ in range(3):
        updates, dirty, order = optimize_branch_lengths_native(dev, tree, load("update", name)["effectivelyNon0BLen"], dirty=dirty, chunk=chunk)
        out.append((updates, list(order), list(dirty), tree.dist.copy()))
    stats = dev.optimize_blens_stats()
    dev.close()
    return out, stats


@pytest.mark.parametrize("schedule", [s for s in SCHEDULES if s != "chunk1"])
@pytest.mark.parametrize("name", ["b1429_scrambled", "synth_siteerr"])
def test_scheduling_never_changes_results(name, schedule):
    if name not in _sched:
        _sched[name] = three_sweeps(name, **SCHEDULES["chunk1"])
    base, base_stats = _sched[name]
    assert base_stats["computed"] == base_stats["used"] == base_stats["launches"] and base_stats["sweeps"] == 3
    assert sum(b[0] for b in base) > 50
    got, stats = three_sweeps(name, **SCHEDULES[schedule])
    print(f"{name} {schedule}: {stats} (one at a time: {base_stats})")
    for k, (g, w) in enumerate(zip(got, base)):
        assert g[0] == w[0] and g[1] == w[1] and g[2] == w[2], (k, g[0], w[0])
        assert np.array_equal(g[3], w[3]), k                              # == on the float64 columns
    assert stats["computed"] >= stats["used"] == base_stats["used"]
    assert stats["repairs"] == base_stats["repairs"] and stats["launches"] <= base_stats["launches"]


# ---- 6. agreement with the Python sweep ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["example_siteerr", "synth_unrest", "b1429_unrest"])
def test_native_sweep_equals_python_sweep(name):
    from maple_amd.tree_host import optimize_branch_lengths, optimize_branch_lengths_native
    upd = load("update", name)
    rec = upd["blen_full_sweeps"][1]
    dev_a, tree_a = make(name, rec["dist_in"])
    up_a, _, order_a = optimize_branch_lengths_native(dev_a, tree_a, upd["effectivelyNon0BLen"])
    dev_b, tree_b = make(name, rec["dist_in"])
    up_b, _, order_b = optimize_branch_lengths(dev_b, tree_b, upd["effectivelyNon0BLen"])
    kids = set(tree_a.children[tree_a.root])
    assert up_a == up_b and [v for v in order_a if v not in kids] == list(order_b)
    assert np.array_equal(tree_a.dist, tree_b.dist)                        # bit for bit
    dev_a.close()
    dev_b.close()


# ---- 7. the fused pass arm ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MAT_NAMES)
def test_swept_branches_with_mutation_lists(name):
    """the kernels' pass arm runs in tests 1-5: these trees have swept branches that carry a MAT mutation list"""
    t = load("search", name)["tree"]
    root = t["root"]
    kids = set(t["children"][root])
    stack, low = [root], []
    while stack:
        v = stack.pop()
        if v != root and v not in kids:
            low.append(v)
        stack.extend(t["children"][v])
    assert sum(1 for v in low if t["mutations"][v]) >= 2


# ---- 8. arguments -----------------------------------------------------------------------------------------------------------------
def raw_call(dev, tree, *, root=None, up=None, dirty="flags", struct_size=None, cap_order=0, order=None, eff=1e-8):
    from maple_amd.runtime import MapleBlenSweepParams, _ptr
    cu, c0, c1, tip, depth = tree.columns()
    up = cu if up is None else up
    flags = np.ones(tree.n, dtype=np.uint8)
    ids = [np.ascontiguousarray(a, dtype=np.int32).copy() for a in (tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp)]
    dist = tree.dist.copy()
    mut = np.ascontiguousarray(tree.id_mut, dtype=np.int32)
    p = MapleBlenSweepParams(C.sizeof(MapleBlenSweepParams) if struct_size is None else struct_size, eff, 0, 0)
    n_upd, n_ord = C.c_int32(-7), C.c_int32(-7)
    rc = dev.lib.maple_tree_optimize_blens(dev.h, tree.n, int(tree.root if root is None else root), _ptr(up), _ptr(c0), _ptr(c1), _ptr(tip),
                                           _ptr(mut), _ptr(depth), _ptr(dist), _ptr(ids[0]), _ptr(ids[1]), _ptr(ids[2]), _ptr(ids[3]),
                                           _ptr(flags) if dirty == "flags" else None, C.byref(p), C.byref(n_upd), cap_order,
                                           None if order is None else _ptr(order), C.byref(n_ord))
    return rc, n_upd.value, n_ord.value, dist, ids


def test_arguments():
    from maple_amd.runtime import MapleError
    from maple_amd.tree_host import HostTree
    name = "example_jc"
    rec = load("update", name)["blen_full_sweeps"][1]
    dev, tree = make(name, rec["dist_in"])
    before = (tree.dist.copy(), tree.id_lower.copy())
    assert raw_call(dev, tree, struct_size=0)[0] == MapleError.ERR_ARG
    assert raw_call(dev, tree, dirty=None)[0] == MapleError.ERR_ARG
    assert raw_call(dev, tree, root=tree.n)[0] == MapleError.ERR_ARG
    assert raw_call(dev, tree, root=-1)[0] == MapleError.ERR_ARG
    up = tree.columns()[0].copy()
    victim = swept(tree)[3]
    up[victim] = tree.root
    rc, _, _, dist, ids = raw_call(dev, tree, up=up)
    assert rc == MapleError.ERR_ARG
    assert np.array_equal(dist, before[0]) and np.array_equal(ids[0], before[1])       # refused before anything was changed
    # capOrder 0 and no order array: the count alone
    rc, n_upd, n_ord, _, _ = raw_call(dev, tree, cap_order=0, order=None)
    assert rc == 0 and n_upd == rec["updates"] and n_ord == len(rec["update_order"]) > 0
    # capOrder below the count: the first capOrder nodes
    order = -np.ones(8, dtype=np.int32)
    rc, n_upd, n_ord, _, _ = raw_call(dev, tree, cap_order=5, order=order)
    assert rc == 0 and n_ord == len(rec["update_order"]) and order[:5].tolist() == rec["update_order"][:5] and (order[5:] == -1).all()
    # a short struct is read for what it has: structSize 16 ends after effectivelyNon0BLen (fastPass and chunk: 0)
    rc, n_upd, n_ord, _, _ = raw_call(dev, tree, struct_size=16)
    assert rc == 0 and n_upd == rec["updates"]
    # a root without children
    lone = HostTree(0, [None], [[]], [0.0], [[]], [0], [None], [None], [None], [None])
    lone.id_lower = lone.id_upRight = lone.id_upLeft = lone.id_totUp = lone.id_mut = -np.ones(1, dtype=np.int32)
    rc, n_upd, n_ord, _, _ = raw_call(dev, lone)
    assert (rc, n_upd, n_ord) == (0, 0, 0)
    dev.close()
    # before maple_set_model
    from maple_amd.runtime import Device
    ctx = load("search", name)["context"]
    dev = Device(ref_indices(ctx), ctx["rootFreqs"], arena_bytes=16 << 20)
    three = HostTree(0, [None, 0, 0], [[1, 2], [], []], [0.0, 1e-4, 1e-4], [[], [], []], [0, 0, 0], [None] * 3, [None] * 3, [None] * 3, [None] * 3)
    three.id_lower = three.id_upRight = three.id_upLeft = three.id_totUp = np.zeros(3, dtype=np.int32)
    three.id_mut = -np.ones(3, dtype=np.int32)
    assert raw_call(dev, three)[0] == MapleError.ERR_STATE
    dev.close()
