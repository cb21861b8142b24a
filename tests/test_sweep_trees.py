"""The oracle twin of the branch-length sweep (tests/sweep_trees.py) against the reference's own records, the arms the records and
the gadgets take, and the items of list_edges.fam_sweep_items at the seams they are named for: no GPU.

The twin takes the reference's own order of work and work lists, so it is compared with every recorded sweep of
tests/golden/update_*.json.gz (blen_full_sweeps, blen_sweeps: the first sweep, converged and perturbed, with and without fastPass) and
of blen_rounds_*.json.gz (successive sweeps from the flags the one before left): return value, repair order and every reachable
dirty flag exact.  Measured: every length of all 8 x (2 + 2) first sweeps and all 29 successive sweeps agrees with its record to
the last bit (largest deviation 0), so the test asks for equality.  The whole set takes about 15 s.
"""
import functools
import gzip
import json
import os

import pytest

import list_edges as le
import sweep_trees as sw
import update_trees as ut
from golden_util import GOLDEN, model_args, ref_indices
from oracle.oracle_py import Oracle

NAMES = sorted(f[len("update_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("update_"))
STD_MODES = le.MODES[:5]
# The counters the 8 x 4 first sweeps and 29 successive sweeps of the records leave at 0: what the gadgets are for.
RECORDS_NEVER = ("root_no_children", "root_grid_round_half_even", "root_grid_equal_costs", "root_best2_clamped", "root_step_raises",
                 "est_positive_len_zero", "est_tenth")
# root_step_raises needs a repair that raises -- a None over a positive length, a zero rate of Q: the zero-rate gadget reaches it.
ZERO_RATE_ONLY = ("root_step_raises",)

def load(kind, name):
    with gzip.open(os.path.join(GOLDEN, f"{kind}_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def replay(name):
    """every recorded sweep of a tree through the twin: (what disagrees with the records, the arms taken, sweeps replayed)"""
    f, upd, rounds = load("search", name), load("update", name), load("blen_rounds", name)
    ctx = f["context"]
    o = Oracle(ref_indices(ctx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"], minBLenSensitivity=ctx["minBLenSensitivity"],
               thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"], thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"],
               defaultBLen=ctx["defaultBLen"])
    o.set_model(**model_args(f["model"]))
    base = ut.fixture_lists(f)
    reach = base.reachable()
    kids = set(base.children[base.root])
    low = [v for v in reach if v != base.root and v not in kids]
    bad, counts, n = [], {}, 0

    def check(tag, t, res, dirty, want_dist, want_dirty, rec, nodes, order=True):
        if res["updates"] != rec["updates"]:
            bad.append((tag, "updates", res["updates"], rec["updates"]))
        if order and res["order"] != rec["update_order"]:
            bad.append((tag, "order"))
        if [bool(dirty[v]) for v in nodes] != [bool(want_dirty[v]) for v in nodes]:
            bad.append((tag, "dirty", [v for v in nodes if bool(dirty[v]) != bool(want_dirty[v])][:5]))
        off = [(v, t.dist[v], want_dist[v]) for v in reach if t.dist[v] != float(want_dist[v] or 0.0)]
        if off:
            bad.append((tag, "lengths", off[:3]))

    for which in (0, 1):
        for fast, key in ((False, "blen_full_sweeps"), (True, "blen_sweeps")):
            rec = upd[key][which]
            t = base.copy()
            t.dist = [float(x) for x in rec["dist_in"]]
            if which and not fast:                                  # (the reference recomputed the lists for the perturbed lengths)
                ut.consistent(o, t)
            dirty = [True] * t.n
            res = sw.oracle_optimize_blens(o, t, dirty, upd["effectivelyNon0BLen"], fast, counts)
            check((key, which), t, res, dirty, rec["dist_out"], rec["dirty_out"], rec, low if fast else reach, order=not fast)
            n += 1
    t = base.copy()
    t.dist = [float(x) for x in rounds["dist_in"]]
    ut.consistent(o, t)
    dirty, want = [True] * t.n, list(t.dist)
    for k, rec in enumerate(rounds["sweeps"]):
        flags_in, flags_out = set(rec["dirty_in"]), set(rec["dirty_out"])
        if any(dirty[v] != (v in flags_in) for v in reach):
            bad.append((("rounds", k), "dirty going in"))
        res = sw.oracle_optimize_blens(o, t, dirty, rounds["effectivelyNon0BLen"], False, counts)
        for v, d in rec["dist_changed"].items():
            want[int(v)] = d
        check(("rounds", k), t, res, dirty, want, [v in flags_out for v in range(t.n)], rec, reach)
        n += 1
    return bad, counts, n


@pytest.mark.parametrize("name", NAMES)
def test_twin_matches_the_recorded_sweeps(name):
    bad, counts, n = replay(name)
    print(f"{name}: {n} sweeps, arms {counts}")
    assert n >= 6
    assert not bad, bad[:5]


def test_the_arms_the_records_leave_untouched():
    total, n = {}, 0
    for name in NAMES:
        _, counts, k = replay(name)
        n += k
        for a, c in counts.items():
            total[a] = total.get(a, 0) + c
    never = tuple(a for a in sw.ARMS if not total.get(a))
    print(f"{n} recorded sweeps: {total}; never taken: {never}")
    assert n == 8 * 4 + 29
    assert set(total) <= set(sw.ARMS)
    assert never == RECORDS_NEVER


@functools.lru_cache(maxsize=None)
def gadget_runs(mode, mutations):
    """{gadget: (gadget, counters of the first full sweep, counters of everything, sweeps compared full / fast)} over what the GPU
    file runs: a full sweep and a fast pass, and a second sweep of each where sweep_trees.sweeps_to_compare allows it"""
    o = Oracle(le.reference(), le.ROOT_FREQS)
    o.set_model(**le.model(mode))
    out = {}
    for g in sw.gadgets(o, mode, mutations).values():
        first, every, n = {}, {}, []
        for fast in (False, True):
            watch = {}
            sw.run_twin(o, g, fastPass=fast, counts=every if fast else first, watch=watch)
            # the first sweep of every gadget is clear of rounding: this is what the GPU comparison cannot be excused by
            assert sw.clear_of_rounding(g, watch.get("ratios", []), watch.get("grids", [])), (g.name, fast, watch)
            n.append(sw.sweeps_to_compare(o, g, fast))
            if n[-1] == 2:
                sw.run_twin(o, g, fastPass=fast, counts=every, sweeps=2)
        for a, c in first.items():
            every[a] = every.get(a, 0) + c
        out[g.name] = (g, first, every, tuple(n))
    return out


@pytest.mark.parametrize("mutations", [False, True], ids=["plain", "mutations"])
@pytest.mark.parametrize("mode", STD_MODES)
def test_gadgets_take_their_arms_and_no_verdict_hangs_on_rounding(mode, mutations):
    runs = gadget_runs(mode, mutations)
    assert len(runs) >= 14
    for name, (g, first, every, n) in runs.items():
        missing = [a for a in g.arms if not (every if a == "node_clean" else first).get(a)]
        assert not missing, (name, missing, first)
        assert all(not every.get(a) for a in ZERO_RATE_ONLY), (name, every)
        assert n == (2, 2) or name not in sw.SECOND_SWEEP, (name, n)
    print({name: r[3] for name, r in runs.items()})
    assert ("grid_equal" in runs) == (mode in ("jc", "unrest", "ratevar") and not mutations)
    assert bool(runs["grid_best2_clamped"][1].get("root_best2_clamped")) == ((mode, mutations) in sw.BEST2_CLAMPED)
    assert list(runs) == sw.gadget_names(mode, mutations)


def test_second_sweeps_are_compared_where_repairs_set_flags():
    """over all modes, a second full sweep is compared on gadgets whose first sweep repairs and moves lengths, not only on the
    converged ones"""
    two = {}
    for mode in STD_MODES:
        for mutations in (False, True):
            for name, (g, first, every, n) in gadget_runs(mode, mutations).items():
                if n[0] == 2 and first.get("moved"):
                    two.setdefault(name, []).append((mode, mutations))
    print(two)
    assert len(two) >= 4 and sum(len(v) for v in two.values()) >= 20, two


@pytest.mark.parametrize("mode", le.MODES[5:])
def test_zero_rate_gadgets_raise_where_they_say(mode):
    o = Oracle(le.reference(), le.ROOT_FREQS)
    o.set_model(**le.model(mode))
    gs = sw.zero_gadgets(o, mode)
    counts = {}
    with pytest.raises(sw.SweepError, match="root grid"):
        sw.run_twin(o, gs["grid_none"], counts=counts)
    assert not counts.get("root_step_raises")
    with pytest.raises(sw.SweepError, match=f"non-zero distances at node {sw.INNER}"):
        sw.run_twin(o, gs["step_raises"], counts=counts)
    assert counts.get("root_step_raises") == 1
    sw.run_twin(o, gs["step_raises"], fastPass=True)                # (no repair, nothing raises)


def test_every_arm_is_reached_by_a_record_or_a_gadget():
    total = {}
    for name in NAMES:
        for a, c in replay(name)[1].items():
            total[a] = total.get(a, 0) + c
    by_gadgets = {}
    for mode in STD_MODES:
        for mutations in (False, True):
            for name, (g, first, every, _) in gadget_runs(mode, mutations).items():
                for a in every:
                    by_gadgets.setdefault(a, set()).add(name)
    print({a: sorted(v) for a, v in by_gadgets.items()})
    for a in sw.ARMS:
        if a in ZERO_RATE_ONLY:                                     # (test_zero_rate_gadgets_raise_where_they_say)
            assert not total.get(a) and a not in by_gadgets, a
        else:
            assert total.get(a) or a in by_gadgets, a
    assert all(a in by_gadgets for a in RECORDS_NEVER if a not in ZERO_RATE_ONLY)     # what only the gadgets reach


# ---- the items of the fused estimate kernels --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", le.MODES)
def test_sweep_items_sit_at_the_seams_they_name(mode):
    o = Oracle(le.reference(), le.ROOT_FREQS)
    o.set_model(**le.model(mode))
    u = bool(le.model(mode).get("usingErrorRate"))
    lists, muts, items = le.fam_sweep_items(mode, o)
    for gl in lists:
        le.check_grammar(gl, le.L_REF, u)
    results, passed_sizes, kinds = set(), {}, set()
    for it in items:
        passed, want = le.sweep_item_expect(o, lists, muts, it)
        results.add("False" if want is False else ("0.1" if want == 0.1 else "length"))
        assert len(lists[it["iup"]]) <= 256 or it["imut"] < 0, it["name"]          # the stored list of a passed one fits the staging
        if "want_passed" in it:
            assert len(passed) == it["want_passed"], (it["name"], len(passed))
            passed_sizes.setdefault(it["want_passed"], set()).add(len(lists[it["ilow"]]))
        if "want_low" in it:
            assert len(lists[it["ilow"]]) == it["want_low"], it["name"]
        if "want_steps" in it:
            assert le.walk_steps(passed, lists[it["ilow"]]) == it["want_steps"], it["name"]
        if "same_nuc_steps" in it:                                              # the same nucleotide on both sides at the last lane of a round
            for step in it["same_nuc_steps"]:
                a, b = le.entry_at(passed, step)[0], le.entry_at(lists[it["ilow"]], step)[0]
                assert a[0] == b[0] < 4 and le.walk_steps(passed[:step], lists[it["ilow"]][:1]) >= step - 1
        if "want_ais" in it:
            assert sum(1 for _, e in le.sites_of(lists[it["ilow"]]) if e[0] < 4 and len(e) > 2) == it["want_ais"] > 64
        kinds.add(it.get("on"))
        kinds.update(it.get("on_kinds", ()))
    assert results == {"False", "0.1", "length"}
    assert set(le.SWEEP_SEAM) <= set(passed_sizes) and all(min(passed_sizes[n]) <= 8 for n in le.SWEEP_SEAM)      # ... against a short lower list
    assert {256, 257} <= {len(lists[it["ilow"]]) for it in items if it.get("want_passed", 999) <= 9}               # long lower, short passed
    assert any(it.get("want_passed") == 300 and it.get("want_low") == 257 for it in items)                          # both long
    assert {it["want_steps"] for it in items if "want_steps" in it} == set(le.SWEEP_STEPS)
    assert {"R_inside", "R_edge", "nuc"} <= kinds and (mode.startswith("zeroq") or {"O", "nuc_to_R"} <= kinds), kinds
    if u:                                                                       # both values of fromTipC on the same lists
        by_lists = {}
        for it in items:
            by_lists.setdefault((repr(lists[it["iup"]]), repr(lists[it["ilow"]]), it["imut"] >= 0 and repr(muts[it["imut"]])), set()).add(it["tip"])
        assert sum(1 for v in by_lists.values() if v == {True, False}) >= 7      # (the seven seam items at least)
    # neighbours: a run of at least 8 mutation-carrying items, and very different scratch slices next to each other
    size = lambda it: len(lists[it["iup"]]) + 2 * len(muts[it["imut"]])                                             # noqa: E731
    run = best = 0
    ratio = 1.0
    for a, b in zip(items, items[1:] + [dict(imut=-1)]):
        run = run + 1 if a["imut"] >= 0 else 0
        best = max(best, run)
        if a["imut"] >= 0 and b["imut"] >= 0:
            ratio = max(ratio, size(a) / size(b), size(b) / size(a))
    assert best >= 8 and ratio >= 20, (best, ratio)
