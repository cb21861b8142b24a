"""The oracle twin of the list repair (tests/update_trees.py) against the reference's own records, the arms the records and the
gadgets take, and a dry run of the GPU file's bars (tests/test_hip_update_edges.py) on the CPU twin of the library: no GPU.

The twin takes the reference's own order of work, so it is compared with the 112 recorded repairs of tests/golden/update_*.json.gz
list for list at the suite's bar for oracle against record: structure exact, doubles to 1e-9 relative; the tree log-likelihood of
the repaired tree (sink_trees.oracle_tree_lk) to 1e-9.  Measured: all 108 221 lists, every length and every log-likelihood of the
112 repairs agree with their records to the last bit (largest deviation 0 in every field), so the test also
holds them to 1e-12.
"""
import ctypes as C
import gzip
import json
import os
import subprocess

import pytest

import list_edges as le
import sink_trees as st
import update_trees as ut
from golden_util import GOLDEN, close, lists_match, model_args, ref_indices, tup
from oracle.oracle_py import Oracle

REL = 1e-9
NAMES = sorted(f[len("update_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("update_"))
ORACLE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")

# The arms of the 112 recorded repairs (the table of DESIGN.md section 9), per tree; an arm that is not named was never taken.
RECORDED = {
    "b1429_scrambled": dict(stop_upper_same=29, stop_lower_same=14, from_child_at_root=1, from_child_lower_none_child_lengthened=1,
                            from_parent_totup_zero_len=4),
    "b1429_unrest": dict(stop_upper_same=46, stop_lower_same=15, from_child_at_root=1, from_child_lower_none_child_lengthened=1,
                         from_parent_totup_zero_len=23, from_parent_upleft_none_node_lengthened=1),
    "example_jc": dict(stop_upper_same=41, stop_lower_same=13, from_child_at_root=1, from_child_lower_none_child_lengthened=4,
                       from_parent_totup_zero_len=16),
    "example_siteerr": dict(stop_upper_same=50, stop_lower_same=12, from_child_at_root=2, from_parent_totup_zero_len=89),
    "example_unrest": dict(stop_upper_same=47, stop_lower_same=15, from_parent_totup_zero_len=18, from_parent_upleft_none_node_lengthened=1),
    "synth_scrambled": dict(stop_upper_same=76, stop_lower_same=14, from_child_at_root=1, from_child_lower_none_child_lengthened=2,
                            from_parent_totup_zero_len=47),
    "synth_siteerr": dict(stop_upper_same=74, stop_lower_same=14, from_parent_totup_zero_len=68),
    "synth_unrest": dict(stop_upper_same=104, stop_lower_same=13, from_child_at_root=3, from_child_lower_none_child_lengthened=1,
                         from_parent_totup_zero_len=47),
}
# Arms the gadgets of the standard modes cannot reach, each with its proof in update_trees.gadgets / zero_gadgets: they stay 0.
OUT_OF_REACH = {"from_parent_totup_none", "from_parent_raise", "from_child_lower_none_other_lengthened", "from_child_lower_raise",
                "from_child_totup_none", "from_child_upvect_none_child_lengthened", "from_child_upvect_raise"}
ZERO_RATE_ARMS = {"from_child_lower_raise", "from_parent_raise", "stop_lower_same"}     # what the zero-rate gadgets are for


def load(kind, name):
    with gzip.open(os.path.join(GOLDEN, f"{kind}_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def cpu_lib():
    subprocess.check_call(["make", "-C", ORACLE, "-s"])
    lib = C.CDLL(os.path.join(ORACLE, "libmaple_cpu.so"))
    lib.maple_last_error.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def plain():
    from maple_amd.runtime import Device  # noqa: F401  (the package must import without a GPU)
    return Oracle(le.reference(), le.ROOT_FREQS)


@pytest.mark.parametrize("name", NAMES)
def test_twin_matches_the_recorded_repairs(name):
    f, upd = load("search", name), load("update", name)
    ctx = f["context"]
    o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
               thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
               defaultBLen=ctx["defaultBLen"])
    o.set_model(**model_args(f["model"]))
    base = ut.fixture_lists(f)
    counts, worst, n_lists = {}, dict(lists=0.0, dist=0.0, treeLK=0.0), 0
    assert len(upd["cases"]) == 14
    for case in upd["cases"]:
        t = base.copy()
        ch = case["change"]
        v = ch["node"]
        if ch["kind"] == "dist":
            t.dist[v] = ch["dist"]
        else:
            t.probVect[v] = tup(ch["probVect"])
        ut.oracle_update_partials(o, t, ut.changed_node_list(t, v), counts)       # nodeList as make_golden_update.py pushed it
        for w in t.reachable():
            for key in ut.KEYS:
                want = case["lists"].get(str(w), {}).get(key, f["tree"][key][w])
                if w == v and key == "probVect" and ch["kind"] == "tip":
                    want = ch["probVect"]
                want = tup(want) if want else None
                got = getattr(t, key)[w]
                assert lists_match(got, want, REL), (ch, w, key)
                if got is not None:
                    worst["lists"] = max(worst["lists"], ut.deviation(got, want))
                    n_lists += 1
            want = float(case["dist"].get(str(w), f["tree"]["dist"][w]) or 0.0)
            assert close(float(t.dist[w]), want, REL), (ch, w, t.dist[w], want)
            if want:
                worst["dist"] = max(worst["dist"], abs(t.dist[w] - want) / want)
        assert set(case["dist"]) <= {str(w) for w in t.reachable()}
        _, contrib, root = st.oracle_tree_lk(o, t)
        lk = 0.0
        for x in contrib:
            lk += x
        lk += root
        assert close(lk, case["treeLK"], REL), (ch, lk, case["treeLK"])
        worst["treeLK"] = max(worst["treeLK"], abs(lk - case["treeLK"]) / abs(case["treeLK"]))
    print(f"{name}: {n_lists} lists, largest deviation from the record {worst}, arms {counts}")
    assert n_lists > 3000
    assert worst["lists"] <= 1e-12 and worst["dist"] <= 1e-12 and worst["treeLK"] <= 1e-12, worst     # far below the bar: the same order of work
    assert counts == RECORDED[name], counts


def test_the_records_leave_most_none_arms_untouched():
    """what the gadgets are for: over the 112 records 11 repairs take a None arm at all, of two kinds"""
    total = {}
    for c in RECORDED.values():
        for k, v in c.items():
            total[k] = total.get(k, 0) + v
    assert set(total) <= set(ut.ARMS)
    none_arms = {k: v for k, v in total.items() if "_none_" in k}
    assert none_arms == dict(from_child_lower_none_child_lengthened=9, from_parent_upleft_none_node_lengthened=2)
    assert [a for a in ut.ARMS if a not in total] == [
        "from_parent_totup_none", "from_parent_upright_none_node_lengthened", "from_parent_upright_none_child_lengthened",
        "from_parent_upleft_none_child_lengthened", "from_parent_raise", "from_child_lower_none_other_lengthened", "from_child_lower_raise",
        "from_child_totup_none", "from_child_upvect_none_node_lengthened", "from_child_upvect_none_child_lengthened",
        "from_child_upvect_raise", "other_upper_absent", "old_lower_absent"]


@pytest.mark.parametrize("mutations", [False, True], ids=["plain", "mutations"])
@pytest.mark.parametrize("mode", le.MODES[:5])
def test_gadgets_reach_every_arm_within_reach(plain, mode, mutations):
    o = plain
    o.set_model(**le.model(mode))
    total = {}
    for g in ut.gadgets(o, mode, mutations).values():
        counts = {}
        twin, res = ut.run_twin(o, g, counts)
        assert all(counts.get(a, 0) > 0 for a in g.arms), (g.name, counts)
        assert g.changed in res["popped"] and res["lengths"] <= res["dirty"]
        if g.complete:                                               # the finished repair is the tree rebuilt from its leaves
            want = ut.consistent(o, twin.copy())
            for key in ut.KEYS:
                for v in twin.reachable():
                    got = getattr(twin, key)[v]
                    assert lists_match(None if got is None else o.shorten(got), getattr(want, key)[v], REL), (g.name, key, v)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    for a in ut.ARMS:
        assert (total.get(a, 0) == 0) == (a in OUT_OF_REACH), (a, total)


@pytest.mark.parametrize("mode", le.MODES[5:])
def test_zero_rate_gadgets(plain, mode):
    o = plain
    o.set_model(**le.model(mode))
    total = {}
    for g in ut.zero_gadgets(o, mode).values():
        counts = {}
        if g.raises:
            with pytest.raises(ut.RepairError) as err:
                ut.run_twin(o, g, counts)
            assert g.raises in str(err.value) and "non-zero distances" in str(err.value)
        else:
            ut.run_twin(o, g, counts)
        assert all(counts.get(a, 0) > 0 for a in g.arms), (g.name, counts)
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    assert ZERO_RATE_ARMS <= set(total)
    assert not set(total) & (OUT_OF_REACH - ZERO_RATE_ARMS), total


@pytest.mark.parametrize("mutations", [False, True], ids=["plain", "mutations"])
@pytest.mark.parametrize("mode", le.MODES[:5])
def test_python_level_loop_on_the_gadgets(cpu_lib, plain, mode, mutations):
    """The bars of test_hip_update_edges.py (b) on the Python level loop over the CPU twin of the library: the gadgets, the twin and
    the comparison are proved where there is no GPU.  The Python loop raises in the upper-pass None arm (the library's loop has
    it): those gadgets assert just that."""
    from maple_amd.runtime import Device
    o = plain
    o.set_model(**le.model(mode))
    dev = Device(le.reference(), le.ROOT_FREQS, lib=cpu_lib)
    dev.set_model(**le.model(mode))
    raised = 0
    for g in ut.gadgets(o, mode, mutations).values():
        twin, _ = ut.run_twin(o, g)
        if g.python_loop_raises:
            with pytest.raises(RuntimeError, match="updateBLen"):
                ut.repaired_by_library(dev, g.before, g.changed, native=False)
            raised += 1
            continue
        host = ut.repaired_by_library(dev, g.before, g.changed, native=False)
        ut.compare_with_twin(dev, o, host, twin, g.before, REL)
        from maple_amd.tree_host import tree_log_likelihood
        assert close(tree_log_likelihood(dev, host)[0], ut.twin_lk(o, twin), REL), g.name
    assert raised == 5
    dev.close()


@pytest.mark.parametrize("mode", le.MODES[:5])
def test_rebuild_twin_against_the_python_level_loop(cpu_lib, plain, mode):
    """update_trees.consistent (the twin of the list rebuild) against rebuild_genome_lists(native=False) on the CPU twin"""
    from maple_amd.runtime import Device
    from maple_amd.tree_host import rebuild_genome_lists
    o = plain
    o.set_model(**le.model(mode))
    dev = Device(le.reference(), le.ROOT_FREQS, lib=cpu_lib)
    dev.set_model(**le.model(mode))
    for mutations in (False, True):
        gs = ut.gadgets(o, mode, mutations)
        for name in ("plain_tip", "long_lists", "zero_len_tip"):
            t = gs[name].before
            want = ut.consistent(o, t.copy())
            host = t.copy().host_tree().upload(dev)
            cols = rebuild_genome_lists(dev, host, native=False)
            for key, ids in zip(ut.KEYS, cols):
                got = dev.download(ids)
                for v in t.reachable():
                    assert lists_match(got[v], getattr(want, key)[v], REL), (name, key, v)
        with pytest.raises(RuntimeError, match="updateBLen"):
            rebuild_genome_lists(dev, gs["lower_none_child"].before.copy().host_tree().upload(dev), native=False)
    dev.close()


@pytest.mark.parametrize("mode", le.MODES[:5])
def test_update_items_family(cpu_lib, plain, mode):
    """The family of the fused item kernels: grammar, every shape edge named in test_hip_update_edges.item_shapes present, every
    form of `old`, at least 3/4 of the threshold cases with a verdict that is stable under +-1e-9 (the GPU test asserts those exactly
    against the oracle; the others against the stand-alone kernels only), and the chain merge -> shorten -> differ on the CPU twin
    of the library against the oracle at the GPU file's bars."""
    from maple_amd.runtime import Device
    o = plain
    o.set_model(**le.model(mode))
    lists, items = fam = le.fam_update_items(mode, o)
    u = bool(le.model(mode).get("usingErrorRate"))
    for gl in lists:
        le.check_grammar(gl, le.L_REF, u)
    shapes = ut.item_shapes(lists, items)
    assert all(shapes.values()), [k for k, v in shapes.items() if not v]
    forms = {it["name"][1] if isinstance(it["name"][1], str) else it["name"][1][:2] for it in items}
    kinds = {"d0_far", "d0_near", "d1_far", "d1_near", "len", "bare_to_tail", "nuc_type", "N_to_R", "O", "O_to_nuc"} | ({"flag"} if u else set())
    assert {"absent", "own", "own_unshortened"} <= forms and {("moved", k) for k in kinds} <= forms, forms
    assert {f[1] for f in forms if isinstance(f, tuple) and f[0] == "moved_unshortened"} >= {"d0_far", "d0_near"}
    assert sum(it["m"] is not None and it["m"] != it["s"] for it in items) > 100            # shorten after the merge absorbs
    thr = [(it, md) for it in items if it["threshold"] for md in (0, 2)]
    stable = sum(le.verdict_stable(o, it, lists[it["iold"]], md) for it, md in thr)
    print(f"{mode}: {len(items)} items, {len(lists)} lists, {stable} of {len(thr)} threshold verdicts stable")
    assert len(thr) > 200 and 4 * stable >= 3 * len(thr), (stable, len(thr))
    dev = Device(le.reference(), le.ROOT_FREQS, lib=cpu_lib)
    dev.set_model(**le.model(mode))
    ut.check_items(dev, o, mode, fam, fused=False)
    dev.close()
