"""maple_tree_error_probs (maple_amd/csrc/error_probs.hip) against the reference's calculateErrorProbabilities (M:9783-10020) as
recorded in tests/golden/errprob_*.json.gz, on the trees of the em_ fixtures they name (tests/test_errprob_fixtures.py checks the
fixtures themselves).

Leaf order, offsets, positions and allele codes must be the recorded ones exactly; probabilities within 1e-12 relative of the
recorded value (the tolerance tests/test_oracle_golden.py holds values to against the reference's records), and the test prints how
many are the same bits."""
import hashlib
import io

import numpy as np
import pytest

import em_util
import errprob_util as eu
from golden_util import model_args

pytestmark = pytest.mark.gpu

NAMES = eu.fixture_names()
REL = 1e-12
MAT_NAME = "synth_siteerr"               # a leaf below a MAT reference branch: its parent's list is passed down first


def make_device(fx, arena=256 << 20):
    from maple_amd.runtime import Device
    ctx = fx["context"]
    return Device(em_util.ref_idx(fx), ctx["rootFreqs"], thresholdProb=ctx["thresholdProb"],
                  minBLenSensitivity=ctx["minBLenSensitivity"], thresholdDiffForUpdate=ctx["thresholdDiffForUpdate"],
                  thresholdFoldChangeUpdate=ctx["thresholdFoldChangeUpdate"], defaultBLen=ctx["defaultBLen"], arena_bytes=arena)


def host_tree(t):
    from maple_amd.tree_host import HostTree
    return HostTree(t["root"], t["up"], t["children"], t["dist"], t["mutations"], t["nMinor"], t["probVect"],
                    t["probVectUpRight"], t["probVectUpLeft"], t["probVectTotUp"])


def walked(tree):
    """the leaves the kernel has a lane for, in the report's order"""
    return [v for v in eu.dfs_leaves(tree) if tree["nMinor"][v] == 0 and tree["up"][v] is not None]


def check(got, rec, label, node_map=None):
    """(records, of them bit-identical): the arrays of one call against one threshold's record"""
    leaf, off, pos, al, pr = got
    w_leaf, w_off, w_pos, w_al, w_pr = eu.arrays(rec)
    if node_map is not None:
        w_leaf = np.asarray([node_map[v] for v in w_leaf], np.int32)
    assert leaf.dtype == np.int32 and off.dtype == np.int64 and pos.dtype == np.int32 and al.dtype == np.uint8 and pr.dtype == np.float64
    assert np.array_equal(leaf, w_leaf), label
    assert np.array_equal(off, w_off), label
    assert np.array_equal(pos, w_pos), label
    assert np.array_equal(al, w_al), label
    same = int(np.count_nonzero(pr.view(np.uint64) == w_pr.view(np.uint64)))
    worst = float(np.max(np.abs(pr - w_pr) / np.abs(w_pr))) if len(w_pr) else 0.0
    print(f"{label}: {len(w_pr)} records, {same} bit-identical, worst relative difference {worst:.3g}")
    assert np.all(np.abs(pr - w_pr) <= REL * np.abs(w_pr)), (label, worst)
    return len(w_pr), same


@pytest.fixture(scope="module", params=NAMES)
def env(request):
    fx = eu.load(request.param)
    em = eu.em_of(fx)
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
        a, b = check(dev.error_probabilities(tree.n_minor, rec["minErrorProb"]), rec, f"{fx['name']} minErrorProb {rec['minErrorProb']}")
        n, same = n + a, same + b
    print(f"{fx['name']}: {same} of {n} probabilities bit-identical")
    assert dev.stats() == arena                                          # the call's temporaries are released


def test_shape_coverage():
    """The shapes the kernel can go wrong at are in the fixtures: a few lanes of one wavefront (cat_zero), less than a block
    (cat_a), several wavefronts with a ragged last one and leaves with minor sequences in between (cat_b), a leaf under a MAT
    reference branch (synth_siteerr: the pass-down path); more than one block is test_two_blocks' tree."""
    t = eu.em_of(eu.load("cat_zero_full"))["tree"]
    assert 0 < len(walked(t)) < 64 and len(eu.dfs_leaves(t)) == 4
    t = eu.em_of(eu.load("cat_a_full"))["tree"]
    assert 0 < len(walked(t)) < 256 and len(walked(t)) % 64 != 0 and len(eu.dfs_leaves(t)) == 55
    for mode in ("gerr", "full"):
        t = eu.em_of(eu.load(f"cat_b_{mode}"))["tree"]
        order, w = eu.dfs_leaves(t), walked(t)
        assert len(order) == 245 and 128 < len(w) < 256 and len(w) % 64 != 0
        minor = [k for k, v in enumerate(order) if t["nMinor"][v] > 0]
        assert minor and 0 < minor[0] and minor[-1] < len(order) - 1     # ... between walked leaves
    t = eu.em_of(eu.load(MAT_NAME))["tree"]
    assert any(t["mutations"][v] for v in walked(t))
    for name in ("synth_siteerr", "example_siteerr", "synth_gtr_err"):
        t = eu.em_of(eu.load(name))["tree"]
        assert t["n"] <= 312 and any(t["nMinor"][v] > 0 for v in eu.dfs_leaves(t))


def doubled(t, L):
    """Two copies of the tree below a new root: the function reads, per leaf, its parent's upper list, its own lower list, its
    distance, its mutation list and its minor sequences -- nothing else of the tree -- so every leaf keeps the reference's records."""
    n = t["n"]
    out = dict(root=2 * n, n=2 * n + 1)
    for k in ("dist", "mutations", "nMinor", "probVect", "probVectUpRight", "probVectUpLeft", "probVectTotUp"):
        out[k] = list(t[k]) + list(t[k]) + [None]
    out["up"] = list(t["up"]) + [None if u is None else u + n for u in t["up"]] + [None]
    out["children"] = [list(c) for c in t["children"]] + [[c + n for c in ch] for ch in t["children"]] + [[t["root"], t["root"] + n]]
    out["up"][t["root"]] = out["up"][t["root"] + n] = 2 * n
    out["dist"][2 * n], out["mutations"][2 * n], out["nMinor"][2 * n] = 0.0, [], 0
    for k in ("probVect", "probVectUpRight", "probVectUpLeft"):
        out[k][2 * n] = [[4, L]]
    return out


def test_two_blocks():
    """More than one block of 256 lanes with a ragged last wavefront: cat_b_full twice below one root."""
    fx = eu.load("cat_b_full")
    em = eu.em_of(fx)
    t = doubled(em["tree"], em["context"]["lRef"])
    n = em["tree"]["n"]
    assert len(walked(t)) == 2 * len(walked(em["tree"])) > 256 and len(walked(t)) % 64 != 0
    dev = make_device(em)
    try:
        dev.set_model(**model_args(em["model"]))
        tree = host_tree(t).upload(dev)
        for rec in fx["thresholds"]:
            twice = dict(leaves=rec["leaves"] + [v + n for v in rec["leaves"]], records=rec["records"] + rec["records"])
            check(dev.error_probabilities(tree.n_minor, rec["minErrorProb"]), twice, f"cat_b_full twice, minErrorProb {rec['minErrorProb']}")
    finally:
        dev.close()


def test_sizing_protocol(env):
    from maple_amd.runtime import MapleError
    fx, em, dev, tree = env
    rec = fx["thresholds"][0]
    w_leaf, w_off, _, _, _ = eu.arrays(rec)
    nL, total = len(w_leaf), int(w_off[-1])
    rc, leaf, off, n_leaves, pos, al, pr, n_rec = dev.tree_error_probs(tree.n_minor, 0.0, nL, 0)          # counted only
    assert rc == 0 and pos is None and n_leaves == nL and n_rec == total
    assert np.array_equal(leaf, w_leaf) and np.array_equal(off, w_off)
    rc, leaf2, off2, n_leaves2, pos, al, pr, n_rec2 = dev.tree_error_probs(tree.n_minor, 0.0, nL, total)   # the full call: the same
    assert rc == 0 and n_leaves2 == nL and n_rec2 == total and np.array_equal(leaf2, leaf) and np.array_equal(off2, off)
    check((leaf2, off2, pos, al, pr), rec, fx["name"] + " full call")
    rc, leaf3, off3, n_leaves3, _, _, _, n_rec3 = dev.tree_error_probs(tree.n_minor, 0.0, nL, total - 1)   # one record short
    assert rc == MapleError.ERR_ARG and str(total) in dev.last_error()
    assert n_leaves3 == nL and n_rec3 == total and np.array_equal(leaf3, leaf) and np.array_equal(off3, off)
    rc, _, _, n_leaves4, _, _, _, _ = dev.tree_error_probs(tree.n_minor, 0.0, nL - 1, total)              # one leaf short
    assert rc == MapleError.ERR_ARG and n_leaves4 == nL
    check(dev.error_probabilities(tree.n_minor, 0.0), rec, fx["name"] + " after the refusals")


def test_two_calls_return_the_same_bytes(env):
    fx, em, dev, tree = env
    a = dev.error_probabilities(tree.n_minor, 0.0)
    b = dev.error_probabilities(tree.n_minor, 0.0)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def permuted(t, seed):
    """(the tree snapshot with its node ids permuted at random, new id of every node)"""
    n = t["n"]
    new_of = np.random.default_rng(seed).permutation(n)
    out = dict(root=int(new_of[t["root"]]), n=n)
    for k in ("up", "children", "dist", "mutations", "nMinor", "probVect", "probVectUpRight", "probVectUpLeft", "probVectTotUp"):
        col = [None] * n
        for v in range(n):
            col[int(new_of[v])] = t[k][v]
        out[k] = col
    out["up"] = [None if u is None else int(new_of[u]) for u in out["up"]]
    out["children"] = [[int(new_of[c]) for c in ch] for ch in out["children"]]
    return out, [int(x) for x in new_of]


@pytest.mark.parametrize("name", ["cat_a_full", MAT_NAME])
def test_node_ids_permuted(name):
    """every leaf keeps its records, matched by its original id (the order of the leaves is the tree's shape, which stays)"""
    fx = eu.load(name)
    em = eu.em_of(fx)
    dev = make_device(em)
    try:
        dev.set_model(**model_args(em["model"]))
        t, new_of = permuted(em["tree"], 7)
        assert t["root"] != em["tree"]["root"] or t["up"] != em["tree"]["up"]
        tree = host_tree(t).upload(dev)
        for rec in fx["thresholds"]:
            check(dev.error_probabilities(tree.n_minor, rec["minErrorProb"]), rec, f"{name} permuted", node_map=new_of)
    finally:
        dev.close()


def fill_arena(dev, ref_idx):
    """lists that take every free entry of the arena"""
    L = len(ref_idx)
    s = dev.stats()
    free = s["cap_entries"] - s["n_entries"]
    big = [((int(r) + 1) % 4, int(r)) for r in ref_idx]                  # L single-site entries, no lengths
    ids = dev.upload([big] * (free // L) + [[(4, L)]] * (free % L))
    s = dev.stats()
    assert s["cap_entries"] == s["n_entries"]
    return ids


def test_error_paths():
    from maple_amd.runtime import MapleError
    fx = eu.load(MAT_NAME)
    em = eu.em_of(fx)
    rec = fx["thresholds"][1]
    dev = make_device(em, arena=8 << 20)
    try:
        with pytest.raises(MapleError) as e:                             # no tree (and no model)
            dev.error_probabilities()
        assert e.value.code == MapleError.ERR_STATE
        dev.set_model(**model_args(em["model"]))
        with pytest.raises(MapleError) as e:                             # a model, no tree
            dev.error_probabilities()
        assert e.value.code == MapleError.ERR_STATE
        tree = host_tree(em["tree"]).upload(dev)
        check(dev.error_probabilities(tree.n_minor, 0.01), rec, "after no tree")
        plain = dict(model_args(em["model"]), usingErrorRate=False, errorRates=None)
        dev.set_model(**plain)                                           # a model without error rates
        with pytest.raises(MapleError) as e:
            dev.error_probabilities(tree.n_minor, 0.01)
        assert e.value.code == MapleError.ERR_STATE and "error rate" in str(e.value)
        dev.set_model(**model_args(em["model"]))
        check(dev.error_probabilities(tree.n_minor, 0.01), rec, "after a model without error rates")
        bad = list(tree.n_minor)
        bad[eu.dfs_leaves(em["tree"])[3]] = -1                           # a negative nMinor
        with pytest.raises(MapleError) as e:
            dev.error_probabilities(bad, 0.01)
        assert e.value.code == MapleError.ERR_ARG and "nMinor" in str(e.value)
        check(dev.error_probabilities(tree.n_minor, 0.01), rec, "after a negative nMinor")
        # an arena with no room for the parent list passed down to the leaf under a reference branch
        assert any(em["tree"]["mutations"][v] for v in walked(em["tree"]))
        mark = dev.mark()
        fill_arena(dev, em_util.ref_idx(em))
        full = dev.stats()
        with pytest.raises(MapleError) as e:
            dev.error_probabilities(tree.n_minor, 0.01)
        assert e.value.code == MapleError.ERR_NOMEM
        assert dev.stats() == full
        dev.release(mark)
        check(dev.error_probabilities(tree.n_minor, 0.01), rec, "after a full arena")
    finally:
        dev.close()
    zd = eu.load("zero_div")                                             # a tree, no model (lists without lengths: they pack under any model)
    dev = make_device(zd, arena=8 << 20)
    try:
        with pytest.raises(MapleError) as e:
            host_tree(zd["tree"]).upload(dev)
            dev.error_probabilities()
        assert e.value.code == MapleError.ERR_STATE
    finally:
        dev.close()


def test_zero_denominator_is_fatal():
    """Where the reference raises ZeroDivisionError (error rate 0, a leaf at distance 0 under a parent entry without lengths):
    MAPLE_ERR_FATAL naming the node and the position; the same context goes on working."""
    from maple_amd.runtime import MapleError
    fx = eu.load("zero_div")
    dev = make_device(fx, arena=8 << 20)
    try:
        dev.set_model(**model_args(fx["model"]))
        tree = host_tree(fx["tree"]).upload(dev)
        arena = dev.stats()
        with pytest.raises(MapleError) as e:
            dev.error_probabilities(tree.n_minor, 0.0)
        assert e.value.code == MapleError.ERR_FATAL, str(e.value)
        assert f"node {fx['node']}," in str(e.value) and f"position {fx['position']}:" in str(e.value), str(e.value)
        assert dev.stats() == arena
        # with an error rate the same site is an error for certain: errorRate * 0.33333 / (errorRate * 0.33333 + q * 0.0)
        dev.set_model(**dict(model_args(fx["model"]), errorRateGlobal=1e-3))
        leaf, off, pos, al, pr = dev.error_probabilities(tree.n_minor, 0.0)
        assert leaf.tolist() == eu.dfs_leaves(fx["tree"]) == [1, 3, 4]
        assert off.tolist() == [0, 0, 1, 1] and pos.tolist() == [fx["position"]] and pr.tolist() == [1.0]
        sub = next(e for e in fx["tree"]["probVect"][fx["node"]] if e[0] < 4)
        assert al.tolist() == [sub[0]]
    finally:
        dev.close()


def test_ops_adapter(env):
    from maple_amd.ops import TreeOps
    fx, em, dev, tree = env
    for rec in fx["thresholds"]:
        out = io.StringIO()
        TreeOps(dev, tree).calculateErrorProbabilities(out, rec["minErrorProb"], fx["namesInTree"], name=fx["nodeName"],
                                                       minorSequences=fx["minorIds"])
        text = out.getvalue()
        # parsed back: the leaves' own name lines in order, and each one's records
        own = {fx["namesInTree"][fx["nodeName"][v]]: v for v in rec["leaves"]}
        leaves, recs = [], []
        for line in text.splitlines():
            if line.startswith(">"):
                if line[1:] in own:
                    leaves.append(own[line[1:]])
                    recs.append([])
            else:
                p, a, x = line.split("\t")
                recs[-1].append([int(p), "ACGTX".index(a), float(x)])
        assert leaves == rec["leaves"]
        assert [[r[:2] for r in rl] for rl in recs] == [[r[:2] for r in rl] for rl in rec["records"]]
        got = [r[2] for rl in recs for r in rl]
        want = [r[2] for rl in rec["records"] for r in rl]
        assert all(abs(g - w) <= REL * abs(w) for g, w in zip(got, want))
        if got == want:                                                  # every probability the same bits: the same text
            assert hashlib.sha256(text.encode()).hexdigest() == rec["sha256"]
        else:
            print(f"{fx['name']} minErrorProb {rec['minErrorProb']}: {sum(g != w for g, w in zip(got, want))} probabilities differ in bits")


def test_with_announced_samples():
    """announce, place one sample, maple_tree_error_probs, place the next: the rows made ahead and the next announced search are what
    they are without the call in between.  (A tree without MAT references -- rows are made only there -- under a global error rate.)"""
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
                report = dev.error_probabilities(tree.n_minor, 0.0)
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
    assert report is not None and len(report[0]) > 100 and len(report[2]) > 0
    assert rows_with == rows_without and rows_with["searches"] == 2
    for a, b in zip(with_call, without_call):
        for key in a:
            assert np.array_equal(a[key], b[key]), key
