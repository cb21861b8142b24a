"""maple_tree_mutation_events (maple_amd/csrc/mat_events.hip) against the reference's
expectationMaximizationCalculationRates(tree, root, trackMutations=True) (M:10077-10850) and stringForNode (M:2673-2809) as recorded
in tests/golden/mat_*.json.gz, on the trees of the em_ fixtures they name (tests/test_mat_fixtures.py checks the fixtures themselves).

The three offset arrays, positions, alleles and the Ns records must be the recorded ones exactly; probabilities within 1e-12
relative of the recorded value (the tolerance tests/test_hip_error_probs.py and tests/test_oracle_golden.py hold values to against
the reference's records), and the test prints how many are the same bits."""
import hashlib

import numpy as np
import pytest

import em_util
import mat_util as mu
from golden_util import model_args
from test_hip_error_probs import fill_arena, host_tree, make_device, permuted

pytestmark = pytest.mark.gpu

NAMES = mu.fixture_names()
REL = 1e-12
MAT_NAME = "synth_siteerr"               # pair items below MAT reference branches: their parents' lists are passed down first


def check(got, rec, n, label, node_map=None):
    """(probabilities, of them bit-identical): the arrays of one call against one threshold's record"""
    ev_t, ns_t = mu.dtypes()
    want = mu.arrays(rec, n, node_map)
    for g, w in zip(got[:3], want[:3]):
        assert g.dtype == np.int64 and np.array_equal(g, w), label
    mut, ns, err = got[3:]
    w_mut, w_ns, w_err = want[3:]
    assert mut.dtype == err.dtype == ev_t and ns.dtype == ns_t
    assert ns.tobytes() == w_ns.tobytes(), label
    n_all = same = 0
    for g, w, stream in ((mut, w_mut, "mutationsInf"), (err, w_err, "errors")):
        for f in ("pos", "from", "to", "zero"):
            assert np.array_equal(g[f], w[f]), (label, stream, f)
        same_s = int(np.count_nonzero(g["prob"].view(np.uint64) == w["prob"].view(np.uint64)))
        worst = float(np.max(np.abs(g["prob"] - w["prob"]) / np.abs(w["prob"]))) if len(w) else 0.0
        print(f"{label} {stream}: {len(w)} records, {same_s} bit-identical, worst relative difference {worst:.3g}")
        assert np.all(np.abs(g["prob"] - w["prob"]) <= REL * np.abs(w["prob"])), (label, stream, worst)
        n_all, same = n_all + len(w), same + same_s
    return n_all, same


@pytest.fixture(scope="module", params=NAMES)
def env(request):
    fx = mu.load(request.param)
    em = mu.em_of(fx)
    dev = make_device(em)
    dev.set_model(**model_args(em["model"]))
    tree = host_tree(em["tree"]).upload(dev)
    yield fx, em, dev, tree
    dev.close()


def test_parity(env):
    fx, em, dev, tree = env
    arena = dev.stats()
    n = same = 0
    for rec in fx["thresholds"]:
        a, b = check(dev.mutation_events(tree.n_minor, rec["minMutProb"]), rec, tree.n, f"{fx['name']} minMutProb {rec['minMutProb']}")
        n, same = n + a, same + b
    print(f"{fx['name']}: {same} of {n} probabilities bit-identical")
    assert dev.stats() == arena                                          # the call's temporaries are released


def test_shape_coverage():
    """The shapes the kernel can go wrong at are in the fixtures: a few lanes of one wavefront (cat_zero), less than a block
    (cat_a), two blocks with a ragged last wavefront and single-list items scattered among pair items (cat_b), pair and single-list
    items under a mutation list (the pass-down path), the root's own records (mat_root_ns)."""
    def shape(name):
        em = em_util.load(name)
        t = em["tree"]
        pair, single = mu.items(t, bool(em["model"]["usingErrorRate"]))
        order = []
        st = [t["root"]]
        while st:                                                        # the launch's item order: depth first
            v = st.pop()
            order.append(v)
            st.extend(reversed(t["children"][v]))
        return t, pair, single, order
    for mode in ("plain", "ratevar", "gerr", "full"):
        t, pair, single, _ = shape(f"cat_zero_{mode}")
        assert (len(pair), len(single)) == (6, 1) and t["n"] == 7
    for name in ("cat_a_plain", "cat_a_ratevar", "cat_a_gerr", "cat_a_full", "cat_a_plain_gtr", "cat_a_gerr_gtr"):
        t, pair, single, _ = shape(name)
        assert len(pair) + len(single) == t["n"] == 109 == 64 + 45       # one wavefront and part of a second
        assert (len(pair), len(single)) == ((99, 10) if "gerr" in name or "full" in name else (86, 23))
    for mode in ("plain", "ratevar", "gerr", "full"):
        t, pair, single, order = shape(f"cat_b_{mode}")
        assert len(order) == t["n"] == 489 and 489 - 256 == 3 * 64 + 41  # two blocks, the second 3 wavefronts and a ragged 41
        assert len(single) in (49, 99) and len(pair) + len(single) == 489
        at = sorted(order.index(v) for v in single)
        assert at[0] < 64 and at[-1] >= 256 + 192 and any(64 <= k < 256 for k in at)   # scattered among the pair items
    for name in NAMES:
        t, pair, single, _ = shape(name)
        under = [v for v in pair if t["mutations"][v]]
        if name.startswith("cat_zero"):
            assert not under
        elif name.startswith("cat_"):
            assert len(under) == 2, name
        else:
            assert 14 <= len(under) <= 16 or (name == "example_siteerr" and not under), (name, len(under))
    assert any(t["mutations"][v] for name in NAMES for t, _, single, _ in [shape(name)] for v in single)
    root_ns = mu.load(mu.ROOT_NS)
    assert all(case["thresholds"][0]["Ns"][case["tree"]["root"]] for case in root_ns["cases"])


def test_root_ns():
    """the hand-built trees: the root's and a zero-length internal child's N runs, one-site N runs and O entries"""
    from maple_amd.ops import TreeOps
    fx = mu.load(mu.ROOT_NS)
    for case in fx["cases"]:
        dev = make_device(fx, arena=8 << 20)
        try:
            dev.set_model(**model_args(fx["model"]))
            tree = host_tree(case["tree"]).upload(dev)
            for rec in case["thresholds"]:
                check(dev.mutation_events(tree.n_minor, rec["minMutProb"]), rec, tree.n, f"root_ns {case['label']}")
                texts = TreeOps(dev, tree).estimateMAT(rec["minMutProb"], **fx["output"])
                assert texts == rec["texts"], case["label"]
        finally:
            dev.close()


def test_negative_probability_is_fatal():
    """cat_a_ratevar_negq: the reference raises Exception('exit') (M:10336 and its kin); the context goes on working"""
    from maple_amd.runtime import MapleError
    neg = mu.load(mu.NEGQ)
    em = em_util.load(mu.NEGQ)
    good = mu.load("cat_a_ratevar")
    dev = make_device(em)
    try:
        dev.set_model(**model_args(em["model"]))
        tree = host_tree(em["tree"]).upload(dev)
        arena = dev.stats()
        for r in neg["perThreshold"]:
            rc = dev.tree_mutation_events(tree.n_minor, r["minMutProb"], 0, 0, 0)[0]
            assert rc == MapleError.ERR_FATAL and "negative probability" in dev.last_error()
        with pytest.raises(MapleError) as e:
            dev.mutation_events(tree.n_minor, 0.01)
        assert e.value.code == MapleError.ERR_FATAL
        assert dev.stats() == arena
        dev.set_model(**model_args(mu.em_of(good)["model"]))             # the same tree under the model that does not raise
        assert mu.em_of(good)["tree"] == em["tree"]
        check(dev.mutation_events(tree.n_minor, 0.01), good["thresholds"][1], tree.n, "after the fatal call")
    finally:
        dev.close()


def test_sizing_protocol(env):
    from maple_amd.runtime import MapleError
    fx, em, dev, tree = env
    rec = fx["thresholds"][0]
    want = mu.arrays(rec, tree.n)
    tot = [int(want[k][-1]) for k in range(3)]
    rc, mo, no, eo, mut, ns, err, n_rec = dev.tree_mutation_events(tree.n_minor, 0.0, 0, 0, 0)                 # counted only
    assert rc == 0 and mut is None and ns is None and err is None and n_rec.tolist() == tot
    assert all(np.array_equal(g, w) for g, w in zip((mo, no, eo), want[:3]))
    full = dev.tree_mutation_events(tree.n_minor, 0.0, *tot)                                                  # the full call
    assert full[0] == 0 and full[7].tolist() == tot
    got = [full[1], full[2], full[3]] + [np.zeros(0, w.dtype) if g is None else g for g, w in zip(full[4:7], want[3:])]
    check(got, rec, tree.n, fx["name"] + " full call")
    for k in range(3):                                                                                        # each cap one short
        if tot[k] == 0:
            continue
        caps = list(tot)
        caps[k] -= 1
        short = dev.tree_mutation_events(tree.n_minor, 0.0, *caps)
        assert short[0] == MapleError.ERR_ARG and str(tot[k]) in dev.last_error()
        assert short[7].tolist() == tot and all(np.array_equal(g, w) for g, w in zip(short[1:4], want[:3]))
    check(dev.mutation_events(tree.n_minor, 0.0), rec, tree.n, fx["name"] + " after the refusals")


def test_two_calls_return_the_same_bytes(env):
    fx, em, dev, tree = env
    a = dev.mutation_events(tree.n_minor, 0.0)
    b = dev.mutation_events(tree.n_minor, 0.0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("name", ["cat_a_full", MAT_NAME])
def test_node_ids_permuted(name):
    """every node keeps its records under its new id"""
    fx = mu.load(name)
    em = mu.em_of(fx)
    dev = make_device(em)
    try:
        dev.set_model(**model_args(em["model"]))
        t, new_of = permuted(em["tree"], 7)
        assert t["root"] != em["tree"]["root"] or t["up"] != em["tree"]["up"]
        tree = host_tree(t).upload(dev)
        for rec in fx["thresholds"]:
            check(dev.mutation_events(tree.n_minor, rec["minMutProb"]), rec, tree.n, f"{name} permuted", node_map=new_of)
    finally:
        dev.close()


def test_error_paths():
    from maple_amd.runtime import MapleError
    fx = mu.load(MAT_NAME)
    em = mu.em_of(fx)
    rec = fx["thresholds"][1]
    n = em["tree"]["n"]
    dev = make_device(em, arena=8 << 20)
    try:
        with pytest.raises(MapleError) as e:                             # no tree (and no model)
            dev.mutation_events()
        assert e.value.code == MapleError.ERR_STATE
        dev.set_model(**model_args(em["model"]))
        with pytest.raises(MapleError) as e:                             # a model, no tree
            dev.mutation_events()
        assert e.value.code == MapleError.ERR_STATE
        tree = host_tree(em["tree"]).upload(dev)
        check(dev.mutation_events(tree.n_minor, 0.01), rec, n, "after no tree")
        bad = list(tree.n_minor)
        bad[em["tree"]["children"][em["tree"]["root"]][0]] = -1          # a negative nMinor
        with pytest.raises(MapleError) as e:
            dev.mutation_events(bad, 0.01)
        assert e.value.code == MapleError.ERR_ARG and "nMinor" in str(e.value)
        check(dev.mutation_events(tree.n_minor, 0.01), rec, n, "after a negative nMinor")
        # an arena with no room for the parent list passed down to a pair item under a reference branch
        pair, _ = mu.items(em["tree"], True)
        assert any(em["tree"]["mutations"][v] for v in pair)
        mark = dev.mark()
        fill_arena(dev, em_util.ref_idx(em))
        full = dev.stats()
        with pytest.raises(MapleError) as e:
            dev.mutation_events(tree.n_minor, 0.01)
        assert e.value.code == MapleError.ERR_NOMEM
        assert dev.stats() == full
        dev.release(mark)
        check(dev.mutation_events(tree.n_minor, 0.01), rec, n, "after a full arena")
    finally:
        dev.close()
    # a model without an error rate: an empty errors stream, not an error
    fx = mu.load("synth_unrest")
    em = mu.em_of(fx)
    assert not em["model"]["usingErrorRate"] and fx["thresholds"][1]["errors"] is None
    dev = make_device(em)
    try:
        with pytest.raises(MapleError) as e:                             # a tree, no model
            host_tree(em["tree"]).upload(dev)
            dev.mutation_events()
        assert e.value.code == MapleError.ERR_STATE
        dev.set_model(**model_args(em["model"]))
        tree = host_tree(em["tree"]).upload(dev)
        got = dev.mutation_events(tree.n_minor, 0.01)
        assert len(got[5]) == 0 and not got[2].any() and len(got[3]) > 0
        check(got, fx["thresholds"][1], em["tree"]["n"], "a model without an error rate")
    finally:
        dev.close()


def test_ops_adapter(env):
    """TreeOps.estimateMAT: where every probability has the reference's bits the per-node text has the recorded SHA-256; the
    rootState text likewise when the root vector's values have them, otherwise positions and alleles exactly, values within REL"""
    import re

    from maple_amd.ops import TreeOps
    fx, em, dev, tree = env
    n = tree.n
    root = em["tree"]["root"]
    for rec in fx["thresholds"]:
        texts = TreeOps(dev, tree).estimateMAT(rec["minMutProb"], **fx["output"])
        assert len(texts) == n
        got = dev.mutation_events(tree.n_minor, rec["minMutProb"])
        want = mu.arrays(rec, n)
        bits = all(g["prob"].tobytes() == w["prob"].tobytes() for g, w in zip((got[3], got[5]), (want[3], want[5])))
        split = lambda s: re.split(r"(?<=:)([0-9.e+-]+)", s)             # noqa: E731  (text, value, text, value, ...)
        g_root, w_root = split(texts[root]), split(rec["rootText"])
        assert g_root[0::2] == w_root[0::2]                              # positions and alleles
        assert all(abs(float(a) - float(b)) <= REL * abs(float(b)) for a, b in zip(g_root[1::2], w_root[1::2]))
        root_bits = g_root == w_root
        if bits:
            rest = [x for v, x in enumerate(texts) if v != root]
            if rec["texts"] is not None:
                assert rest == [x for v, x in enumerate(rec["texts"]) if v != root]
            if root_bits:
                assert hashlib.sha256("\n".join(texts).encode()).hexdigest() == rec["sha256"]
        if not (bits and root_bits):
            print(f"{fx['name']} minMutProb {rec['minMutProb']}: records bit-identical {bits}, rootState bit-identical {root_bits}")


def test_em_unchanged():
    """maple_em_expectation's totals are the same bytes before and after a mutation_events call on the same context"""
    em = em_util.load("cat_b_full")
    dev = make_device(em)
    try:
        dev.set_model(**model_args(em["model"]))
        tree = host_tree(em["tree"]).upload(dev)
        keys = ("counts", "waitingTimes", "errorCount", "totTreeLength", "observedTotNucsSites", "numTips", "observedNucsSites")
        before = dev.em_expectation(tree.n_minor)
        assert len(dev.mutation_events(tree.n_minor, 0.01)[3]) > 0
        after = dev.em_expectation(tree.n_minor)
        for k in keys:
            assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
    finally:
        dev.close()


def test_with_announced_samples():
    """announce, place one sample, maple_tree_mutation_events, place the next: the rows made ahead and the next announced search are
    what they are without the call in between.  (A tree without MAT references -- rows are made only there -- under a global error
    rate.)"""
    import gzip
    import json
    import os

    import test_hip_search as S
    from golden_util import tup
    from maple_amd.tree_host import update_genome_lists
    name = next(n for n in S.E2E_NAMES if not S._has_mat(json.load(gzip.open(os.path.join(S.GOLDEN, f"e2e_{n}.json.gz"), "rt"))))

    def run(announce, with_call):
        f, dev = S._e2e_env(name)
        ctx = f["context"]
        dev.set_model(**dict(model_args(f["model"]), usingErrorRate=True, errorRateGlobal=1e-3))
        tree = S._tree_from_topology(dev, f["online_start"], f["tips"])
        pkw = dict(oneMutBLen=ctx["oneMutBLen"], effectivelyNon0BLen=ctx["effectivelyNon0BLen"], thresholdLogLK=ctx["thresholdLogLK"],
                   thresholdLogLKoptimization=ctx["thresholdLogLKoptimization"],
                   thresholdLogLKconsecutivePlacement=ctx["thresholdLogLKconsecutivePlacement"], allowedFails=ctx["allowedFails"],
                   strictStopRules=ctx["strictStopRules"])
        tree.upload_topology(dev)
        recs = f["online"][:3]
        qids = [int(x) for x in dev.upload([tup(r["query"]) for r in recs])]
        s0 = dev.placement_ahead_stats()
        outs, report = [], None
        for k, rec in enumerate(recs[:2]):
            tree.sync(dev)
            dev.placement_prepare(**pkw)
            if k == 0 and announce:
                assert dev.placement_ahead(np.asarray(qids, dtype=np.int32), **pkw) == len(qids)
            if k == 1 and with_call:
                report = dev.mutation_events(tree.n_minor, 0.0)
            mark = dev.mark()
            out = dev.placement_search_batch(np.asarray([qids[k]], dtype=np.int32), **pkw)
            dev.release(mark)
            outs.append({kk: vv.copy() for kk, vv in out.items()})
            if k == 0:                                                   # the recorded placement of the first sample, then its lists
                after = rec["after"]
                changed = tree.apply_topology(after["root"], after["up"], after["children"], after["dist"], after["nMinor"],
                                              after.get("mutations"), dev)
                for v, lst in rec["new_tips"].items():
                    tree.id_lower[int(v)] = dev.upload([tup(lst)])[0]
                    if int(v) not in changed:
                        changed.append(int(v))
                update_genome_lists(dev, tree, changed)
        s1 = dev.placement_ahead_stats()
        dev.close()
        return outs, {k: s1[k] - s0[k] for k in ("searches", "fallbacks", "expanded_items")}, report

    with_call, rows_with, report = run(True, True)
    without_call, rows_without, _ = run(True, False)
    assert report is not None and len(report[0]) > 100 and len(report[3]) > 0
    assert rows_with == rows_without and rows_with["searches"] == 2
    for a, b in zip(with_call, without_call):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
