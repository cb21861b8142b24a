"""GPU differential tests of the branch-length sweep (maple_tree_optimize_blens; maple_amd/csrc/blen_sweep.hip, sweep_plan.h)
against the C oracle, on the debug library and on explicit inputs -- never the fixture trees:

(a) the fused estimate kernels k_sweep_estimate / k_sweep_estimate_wave on explicit items (maple_debug_sweep_estimate, which is
    sweep_estimate of blen_sweep.hip itself) over list_edges.fam_sweep_items, ONE shuffled batch per mode, against
    estimateBranchLengthWithDerivative(passGenomeListThroughBranch(upper, mutations), lower, fromTipC) of the oracle;
(b) the same items bit for bit against maple_pass_branch_batch followed by maple_blen_batch, form against form (a wavefront per
    item, a lane per item by tuning and by count), every item alone against the item inside the batch; nothing is left in the arena;
(c) the gadgets of tests/sweep_trees.py (5 and 13 nodes) through maple_tree_optimize_blens under four schedules, with and without
    fastPass, against the oracle twin of the reference's sweep; a second sweep from the flags the first left;
(d) where the reference raises: MAPLE_ERR_FATAL, never a device fault;
(e) the hook's arguments.

Bars (those of the rest of the suite): False flags, 0.1, update counts, repair order and dirty flags exact; lengths of single
estimates within 1e-9 relative (test_hip_list_edges.REL), lengths after a sweep within check_lengths of test_hip_blen_sweep.py
(1e-6 relative); kernel forms and schedules bit for bit against each other.  tests/test_sweep_trees.py shows on the CPU that no
verdict of a gadget hangs on rounding, so no difference here can be excused by it.
"""
import numpy as np
import pytest

import list_edges as le
import sweep_trees as sw
import update_trees as ut
from golden_util import close

pytestmark = pytest.mark.gpu
REL = 1e-9                                                         # test_hip_list_edges.REL
STD_MODES = le.MODES[:5]
EFF = 1e-8                                                         # effectivelyNon0BLen of the gadget sweeps
WORST = {}


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


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- (a), (b) the fused estimate kernels ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", le.MODES)
def test_sweep_estimate_items_every_form(ctx, mode):
    dev, o = use(ctx, mode)
    lists, muts, items = le.fam_sweep_items(mode, o)
    n = len(items)
    assert 64 < n <= 1024
    before = dev.stats()
    mark = dev.mark()
    ids, mids = dev.upload(lists), dev.upload_mutations(muts)
    col = lambda k: np.asarray([it[k] for it in items])                            # noqa: E731
    up, low, tip = ids[col("iup")], ids[col("ilow")], col("tip").astype(np.uint8)
    imut = col("imut")
    ml = np.where(imut >= 0, mids[np.maximum(imut, 0)], -1).astype(np.int32)
    loaded = dev.stats()
    tw, fw = dev.debug_sweep_estimate(up, ml, low, tip)                                  # a wavefront per item
    assert dev.stats() == loaded                                                         # the pass goes to scratch: no list is made
    # (a) against the oracle
    seen = set()
    for k, it in enumerate(items):
        _, want = le.sweep_item_expect(o, lists, muts, it)
        if want is False:
            assert fw[k], (it["name"], tw[k])
        elif want == 0.1:
            assert not fw[k] and tw[k] == 0.1, (it["name"], tw[k], fw[k])
        else:
            assert not fw[k] and close(float(tw[k]), want, REL), (it["name"], tw[k], want)
            note("estimate", abs(float(tw[k]) - want) / want)
        seen.add("False" if want is False else ("0.1" if want == 0.1 else "length"))
    assert seen == {"False", "0.1", "length"}
    # (b) against the two-call chain, bit for bit
    has = ml >= 0
    passed = up.copy()
    passed[has] = dev.pass_branch_batch(up[has], ml[has], False)
    for it, pid in zip(items, passed):
        if "want_passed" in it:
            assert dev.sizes([pid])[0][0] == it["want_passed"], it["name"]
    tb, fb = dev.blen_batch(passed, low, tip)
    assert np.array_equal(fw, fb) and np.array_equal(bits(tw), bits(tb)), [items[k]["name"] for k in np.nonzero(bits(tw) != bits(tb))[0]][:5]
    # form against form: a lane per item by tuning, and by count
    dev.set_tuning(wave_per_item_max=-1)
    tl, fl = dev.debug_sweep_estimate(up, ml, low, tip)
    dev.set_tuning()
    assert np.array_equal(fw, fl) and np.array_equal(bits(tw), bits(tl)), [items[k]["name"] for k in np.nonzero(bits(tw) != bits(tl))[0]][:5]
    reps = 1024 // n + 1
    tile = np.tile(np.arange(n), reps)
    assert len(tile) > 1024
    tt, ft = dev.debug_sweep_estimate(up[tile], ml[tile], low[tile], tip[tile])
    assert np.array_equal(ft.reshape(reps, n), np.tile(fw, (reps, 1))) and np.array_equal(bits(tt).reshape(reps, n), np.tile(bits(tw), (reps, 1)))
    # every item alone
    for k in range(n):
        t1, f1 = dev.debug_sweep_estimate(up[k:k + 1], ml[k:k + 1], low[k:k + 1], tip[k:k + 1])
        assert f1[0] == fw[k] and bits(t1)[0] == bits(tw)[k], items[k]["name"]
    dev.release(mark)
    assert dev.stats() == before


# ---- (e) the hook's arguments -------------------------------------------------------------------------------------------------------------
def test_sweep_estimate_arguments(ctx):
    from maple_amd.abi import MapleError
    dev, o = use(ctx, "unrest")
    mark = dev.mark()
    ref = le.reference()
    ids = dev.upload([[(4, le.L_REF)], le.Builder(ref, False).nuc(400, le.other(np.random.default_rng(0), int(ref[399]))).done()])
    mids = dev.upload_mutations([[le.mutation(ref, 100, False, (int(ref[99]) + 1) % 4)]])
    n_lists = dev.stats()["n_lists"]
    good = ([ids[0], ids[0]], [mids[0], -1], [ids[1], ids[1]], [0, 1])
    t0, f0 = dev.debug_sweep_estimate(*good)
    for k, bad in ((0, n_lists), (0, -1), (2, n_lists), (2, -1), (1, int(mids[-1]) + 1), (1, 1 << 30), (1, -2)):
        args = [list(a) for a in good]
        args[k][1] = bad
        with pytest.raises(MapleError) as err:
            dev.debug_sweep_estimate(*args)
        assert err.value.code == MapleError.ERR_ARG, (k, bad, str(err.value))
    t1, f1 = dev.debug_sweep_estimate(*good)                                             # the context is as it was
    assert np.array_equal(bits(t0), bits(t1)) and np.array_equal(f0, f1) and not f0.any()
    dev.release(mark)


# ---- (c) the gadgets through maple_tree_optimize_blens ------------------------------------------------------------------------------------
SCHEDULES = {"chunk1": dict(chunk=1, wave=0), "adaptive": dict(chunk=0, wave=0), "lanes": dict(chunk=0, wave=-1), "chunk7": dict(chunk=7, wave=0)}


def upload(dev, g):
    host = g.tree.copy().host_tree()
    if host.n == 1:                                                 # a lone root: no list of it is read, no topology to upload
        host.id_lower = host.id_upRight = host.id_upLeft = host.id_totUp = host.id_mut = -np.ones(1, dtype=np.int32)
        return host
    return host.upload(dev)


def check_sweeps(dev, o, g, fast):
    """One gadget under every schedule against the twin (and schedule against schedule bit for bit): the bars of (c)."""
    from maple_amd.tree_host import optimize_branch_lengths_native
    from test_hip_blen_sweep import check_lengths
    sweeps = sw.sweeps_to_compare(o, g, fast)
    assert sweeps == 2 or g.name not in sw.SECOND_SWEEP
    twin, want = sw.run_twin(o, g, fastPass=fast, sweeps=sweeps)
    reach = twin.reachable()
    left = []
    for name, sched in SCHEDULES.items():
        dev.set_tuning(wave_per_item_max=sched["wave"])
        count0 = dev.stats()["n_lists"]
        mark = dev.mark()
        host = upload(dev, g)
        ids0 = [getattr(host, a).copy() for a in ut.ATTRS.values()]
        loaded = dev.stats()["n_lists"]
        repairs0 = dev.optimize_blens_stats()["repairs"]
        dirty, got = list(g.dirty), []
        for k in range(sweeps):
            updates, dirty, order = optimize_branch_lengths_native(dev, host, sw.EFF, dirty=dirty, fast_pass=fast, chunk=sched["chunk"])
            assert updates == want[k]["updates"], (g.name, name, k, updates, want[k]["updates"])
            assert order == want[k]["order"], (g.name, name, k, order, want[k]["order"])
            assert [bool(dirty[v]) for v in reach] == [bool(want[k]["dirty"][v]) for v in reach], (g.name, name, k)
            check_lengths(host, want[k]["dist"], reach)
            for v in reach:
                if want[k]["dist"][v]:
                    note("sweep dist", abs(float(host.dist[v]) - want[k]["dist"][v]) / want[k]["dist"][v])
            got.append((updates, list(order), [bool(dirty[v]) for v in reach], host.dist.copy()))
        ids = [getattr(host, a).tolist() for a in ut.ATTRS.values()]
        if fast:                                                    # lists and ids untouched, no repairs, nothing left in the arena
            assert all(np.array_equal(a, getattr(host, b)) for a, b in zip(ids0, ut.ATTRS.values())), (g.name, name)
            assert dev.optimize_blens_stats()["repairs"] == repairs0 and dev.stats()["n_lists"] == loaded, (g.name, name)
        elif host.n > 1:
            ut.compare_with_twin(dev, o, host, twin, g.tree, REL, WORST, tag=(g.name, name))
        flat = [i for c in ids for i in c if i >= 0]
        left.append((got, ids, dev.download_packed(flat) if flat else None))
        dev.release(mark)
        assert dev.stats()["n_lists"] == count0
    dev.set_tuning()
    for (got, ids, pk), name in zip(left[1:], list(SCHEDULES)[1:]):
        for a, b in zip(got, left[0][0]):
            assert a[:3] == b[:3] and np.array_equal(bits(a[3]), bits(b[3])), (g.name, name)
        assert ids == left[0][1], (g.name, name)
        if pk is not None:
            assert all(np.array_equal(getattr(pk, a), getattr(left[0][2], a)) for a in ("ent_off", "pos", "meta", "aux_off")), (g.name, name)
            assert np.array_equal(bits(pk.aux), bits(left[0][2].aux)), (g.name, name)


_GADGETS = {}


def gadget(o, mode, mutations, name):
    if (mode, mutations) not in _GADGETS:
        _GADGETS[(mode, mutations)] = sw.gadgets(o, mode, mutations)
        assert list(_GADGETS[(mode, mutations)]) == sw.gadget_names(mode, mutations)
    return _GADGETS[(mode, mutations)][name]


CASES = [(mode, mutations, name) for mode in STD_MODES for mutations in (False, True) for name in sw.gadget_names(mode, mutations)]


@pytest.mark.parametrize("fast", [False, True], ids=["full", "fastPass"])
@pytest.mark.parametrize("mode,mutations,name", CASES, ids=[f"{m}-{'mutations' if x else 'plain'}-{n}" for m, x, n in CASES])
def test_optimize_blens_on_the_gadgets(ctx, mode, mutations, name, fast):
    """Every gadget under every schedule against the twin (the root step's repair of the second child: DESIGN.md section 15)."""
    dev, o = use(ctx, mode)
    check_sweeps(dev, o, gadget(o, mode, mutations, name), fast)


# ---- (d) where the reference raises --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", le.MODES[5:])
def test_grid_without_a_root_vector_is_an_error_return(ctx, mode):
    """No root vector at a grid point: MAPLE_ERR_FATAL where the twin raises, nothing repaired, and the next sweep on the same
    context works.  The same for a repair of the root's branches that raises."""
    from maple_amd.abi import MapleError
    from maple_amd.tree_host import optimize_branch_lengths_native
    dev, o = use(ctx, mode)
    g = sw.zero_gadgets(o, mode)["grid_none"]
    with pytest.raises(sw.SweepError):
        sw.run_twin(o, g)
    for fast in (False, True):
        mark = dev.mark()
        host = upload(dev, g)
        ids0 = [getattr(host, a).copy() for a in ut.ATTRS.values()]
        dist0 = host.dist.copy()
        with pytest.raises(MapleError) as err:
            optimize_branch_lengths_native(dev, host, sw.EFF, fast_pass=fast)
        assert err.value.code == MapleError.ERR_FATAL, str(err.value)
        assert np.array_equal(bits(host.dist), bits(dist0)) and all(np.array_equal(a, getattr(host, b)) for a, b in zip(ids0, ut.ATTRS.values()))
        dev.release(mark)
    # a repair of the root's branches that raises (the reference's except: arm would raise again): an error return as well,
    # naming the node; the fast pass makes no repair and goes through
    g = sw.zero_gadgets(o, mode)["step_raises"]
    with pytest.raises(sw.SweepError):
        sw.run_twin(o, g)
    mark = dev.mark()
    host = upload(dev, g)
    with pytest.raises(MapleError) as err:
        optimize_branch_lengths_native(dev, host, sw.EFF)
    assert err.value.code == MapleError.ERR_FATAL and f"node {sw.INNER}" in str(err.value), str(err.value)
    dev.release(mark)
    check_sweeps(dev, o, g, True)
    dev, o = use(ctx, "unrest")
    check_sweeps(dev, o, sw.gadgets(o, "unrest")["perturbed"], False)
