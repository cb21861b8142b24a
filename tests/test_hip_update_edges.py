"""GPU differential tests of the list repair (maple_update_partials, maple_tree_rebuild_lists; maple_amd/csrc/update.hip and
update_plan.h) against the C oracle, on the debug library:

(a) the fused item kernels k_update_items / k_update_items_wave on explicit lists (maple_debug_update_items, which is update_items of
    update.hip itself) over list_edges.fam_update_items -- every item in the three modes, as uploaded (a wavefront per item), one lane
    per item (wave_per_item_max = -1) and tiled past 4 096 items (the lane kernel, grid-stride);
(b) the repair on the gadgets of tests/update_trees.py against the oracle twin of the reference's LIFO updatePartials, with the
    counters of maple_debug_update_partials_stats showing that the arm a gadget is named for was taken, and the fatal exits;
(c) maple_tree_rebuild_lists with and without bumpLen on the gadget whose cherry has no merge at length 0.

Bars (those of the rest of the suite): None flags, verdicts and integer structure exact, doubles within 1e-9 relative
(test_hip_parity.REL); the fused kernels bit for bit what maple_merge_batch -> maple_shorten_batch -> maple_differ_batch leave on
the same lists; kernel forms bit for bit against each other.

The bodies shared with the CPU file (tests/test_update_trees.py runs the parts that need no fused kernel on the CPU twin of the
library) are in tests/update_trees.py: item_shapes, check_items, compare_with_twin, twin_lk.
"""
import numpy as np
import pytest

import list_edges as le
import update_trees as ut
from golden_util import close, lists_match

pytestmark = pytest.mark.gpu
REL = 1e-9
STD_MODES = le.MODES[:5]
WORST = {}                                                         # the largest deviation from the oracle per field (printed at the end)


@pytest.fixture(scope="module")
def ctx():
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref = le.reference()
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20, debug=True)
    o = Oracle(ref, le.ROOT_FREQS)
    yield dev, o
    print("largest deviation from the oracle per field:", {k: float(f"{v:.3g}") for k, v in sorted(WORST.items())})
    dev.close()


def use(ctx, mode):
    dev, o = ctx
    for x in (dev, o):
        x.set_model(**le.model(mode))
    dev.set_tuning()
    return dev, o


def note(field, value):
    WORST[field] = max(WORST.get(field, 0.0), value)


# ---- (a) the fused kernels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", STD_MODES)
def test_fused_update_items_every_form(ctx, mode):
    dev, o = use(ctx, mode)
    fam = le.fam_update_items(mode, o)
    shapes = ut.item_shapes(*fam)
    assert all(shapes.values()), [k for k, v in shapes.items() if not v]
    ut.check_items(dev, o, mode, fam, worst=WORST)


# ---- (b) the repair on the gadgets ------------------------------------------------------------------------------------------------------
def check_gadget(dev, o, g, stats=True, forms=(0, -1)):
    """One gadget through maple_update_partials in the given kernel forms against the twin: the bars of (b)."""
    from maple_amd.tree_host import tree_log_likelihood, update_genome_lists
    twin, res = ut.run_twin(o, g)
    want_lk = ut.twin_lk(o, twin)
    left = []
    for wave in forms:
        dev.set_tuning(wave_per_item_max=wave)
        count0 = dev.stats()["n_lists"]
        mark = dev.mark()
        host = g.before.copy().host_tree().upload(dev)
        pre = {a: getattr(host, a).copy() for a in ut.ATTRS.values()}
        pre_dist = host.dist.copy()
        update_genome_lists(dev, host, [g.changed])
        touched = set(int(v) for v in dev.update_partials_touched())
        visited = set(int(v) for v in dev.debug_update_partials_visited())
        assert (set(res["popped"]) | res["dirty"]) <= visited, (g.name, sorted(set(res["popped"]) | res["dirty"]), sorted(visited))
        assert all(v in visited and twin.up[v] in visited for v in res["lengths"]), (g.name, res["lengths"], sorted(visited))
        if stats:
            st = dev.debug_update_partials_stats()
            for k, v in g.stats.items():
                assert st[k] >= v, (g.name, k, st)
            assert all(st[k] == 0 for k in g.never), (g.name, g.never, st)
        ut.compare_with_twin(dev, o, host, twin, g.before, REL, WORST, tag=(g.name, wave))
        got_lk, _ = tree_log_likelihood(dev, host)
        assert close(got_lk, want_lk, REL), (g.name, got_lk, want_lk)
        note("treeLK", abs(got_lk - want_lk) / abs(want_lk))
        moved = {v for a in ut.ATTRS.values() for v in np.nonzero(getattr(host, a) != pre[a])[0].tolist()}
        moved |= set(np.nonzero(host.dist != pre_dist)[0].tolist())
        assert moved <= touched, (g.name, moved, touched)
        ids = [getattr(host, a).tolist() for a in ut.ATTRS.values()]
        flat = [i for c in ids for i in c if i >= 0]
        left.append((ids, dev.download_packed(flat), host.dist.copy()))
        dev.release(mark)
        assert dev.stats()["n_lists"] == count0
    dev.set_tuning()
    for ids, pk, dist in left[1:]:                                  # form against form: ids, lists and lengths bit for bit
        assert ids == left[0][0], g.name
        assert all(np.array_equal(getattr(pk, a), getattr(left[0][1], a)) for a in ("ent_off", "pos", "meta", "aux_off")), g.name
        assert np.array_equal(pk.aux.view(np.uint64), left[0][1].aux.view(np.uint64)), g.name
        assert np.array_equal(dist.view(np.uint64), left[0][2].view(np.uint64)), g.name


@pytest.mark.parametrize("mutations", [False, True], ids=["plain", "mutations"])
@pytest.mark.parametrize("mode", STD_MODES)
def test_update_partials_on_the_gadgets(ctx, mode, mutations):
    dev, o = use(ctx, mode)
    gs = ut.gadgets(o, mode, mutations)
    assert len(gs) >= 20
    for g in gs.values():
        check_gadget(dev, o, g)


@pytest.mark.parametrize("mode", le.MODES[5:])
def test_update_partials_fatal_exits(ctx, mode):
    """A None from non-zero lengths in the lower and in the upper merge: MAPLE_ERR_FATAL naming the node, exactly where the twin
    raises; the next call on a fresh upload of the same context succeeds."""
    from maple_amd.abi import MapleError
    from maple_amd.tree_host import update_genome_lists
    dev, o = use(ctx, mode)
    gs = ut.zero_gadgets(o, mode)
    for name in ("lower_raise", "upper_raise"):
        g = gs[name]
        with pytest.raises(ut.RepairError) as twin_err:
            ut.run_twin(o, g)
        assert g.raises in str(twin_err.value)
        for wave in (0, -1):
            dev.set_tuning(wave_per_item_max=wave)
            mark = dev.mark()
            host = g.before.copy().host_tree().upload(dev)
            with pytest.raises(MapleError) as err:
                update_genome_lists(dev, host, [g.changed])
            assert err.value.code == MapleError.ERR_FATAL and g.raises in str(err.value) and "non-zero distances" in str(err.value), str(err.value)
            dev.release(mark)
            check_gadget(dev, o, gs["no_change"], forms=(wave,))
    dev.set_tuning()


# ---- (c) maple_tree_rebuild_lists ---------------------------------------------------------------------------------------------------------
def rebuild(dev, t, bump):
    """maple_tree_rebuild_lists on the tips' lists of t (the internal nodes' lists dropped): (the four id columns, dist, bad)"""
    host = t.copy()
    for v in range(host.n):
        if host.children[v]:
            host.probVect[v] = None
        host.probVectUpRight[v] = host.probVectUpLeft[v] = host.probVectTotUp[v] = None
    h = host.host_tree().upload(dev)
    up, c0, c1, tip, _ = h.columns()
    dist = np.ascontiguousarray(h.dist.copy())
    lo, ur, ul, tu, bad = dev.tree_rebuild_lists(h.root, up, c0, c1, tip, h.id_mut, dist, h.id_lower, bump_len=bump)
    return (lo, ur, ul, tu), dist, bad


def check_rebuild(dev, o, mode, mutations):
    from maple_amd.abi import MapleError
    gs = ut.gadgets(o, mode, mutations)
    # a consistent tree: the lists the twin rebuild makes with the oracle's operators in the same order
    for name in ("plain_tip", "long_lists", "zero_len_tip"):
        t = gs[name].before
        want = ut.consistent(o, t.copy())
        mark = dev.mark()
        cols, dist, bad = rebuild(dev, t, 0.0)
        assert len(bad) == 0 and np.array_equal(dist, np.asarray(t.dist))
        for key, ids in zip(ut.KEYS, cols):
            got = dev.download(ids)
            for v in t.reachable():
                assert lists_match(got[v], getattr(want, key)[v], REL), (name, key, v)
                if got[v] is not None:
                    note("rebuild " + key, ut.deviation(got[v], getattr(want, key)[v]))
        dev.release(mark)
    # the cherry without a merge at length 0: fatal without bumpLen; with it both lengths become max(dist, bumpLen)
    t = gs["lower_none_child"].before
    mark = dev.mark()
    with pytest.raises(MapleError) as err:
        rebuild(dev, t, 0.0)
    assert err.value.code == MapleError.ERR_FATAL and f"node {ut.INNER}" in str(err.value), str(err.value)
    dev.release(mark)
    for bump in (1e-5, 3e-4):
        want = ut.consistent(o, t.copy(), bump=bump)
        assert want.dist[ut.TA] == bump and want.dist[ut.TB] == bump
        mark = dev.mark()
        cols, dist, bad = rebuild(dev, t, bump)
        assert len(bad) == 0
        assert dist.tolist() == want.dist, (dist, want.dist)
        for key, ids in zip(ut.KEYS, cols):
            got = dev.download(ids)
            for v in t.reachable():
                assert lists_match(got[v], getattr(want, key)[v], REL), (key, v, bump)
        dev.release(mark)


@pytest.mark.parametrize("mutations", [False, True], ids=["plain", "mutations"])
@pytest.mark.parametrize("mode", STD_MODES)
def test_tree_rebuild_lists_on_the_gadgets(ctx, mode, mutations):
    dev, o = use(ctx, mode)
    for wave in (0, -1):
        dev.set_tuning(wave_per_item_max=wave)
        check_rebuild(dev, o, mode, mutations)
    dev.set_tuning()
