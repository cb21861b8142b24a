"""maple_tree_log_lk and maple_tree_find_best_root against the C oracle on the rare arms of the merge and of findProbRoot, inside
the kernels that run them with a sink for an output: k_tree_lk, k_root_children (CountSink), k_root_up, k_root_new_list (a Writer
into per-slot scratch) and k_root_new (RootProbSink).  The reference's own records (tests/golden/search_*) never take these
kernels into the carry-over of the running factor, its underflow, flagged entries at the root or long lists: the trees here are
made of the adversarial corpus (tests/list_edges.py) by tests/sink_trees.py, whose oracle twin of the two calls gives every
expected value; tests/test_sink_trees.py pins that twin to the reference's records and gates what the trees reach.

Bars: a likelihood contribution within 1e-9 relative of the oracle's (test_mergeVectors_every_form); a branch score within 1e-9 of
the sum of the magnitudes of its four terms (the suite's 1e-9 per operator value, applied to the terms: on these trees' k0 and k1
the terms' magnitudes sum to up to 8.5 x 10^5 times the score, the figure tests/test_sink_trees.py prints per model); NaN, fatal
and abandoned outcomes exactly; the Python path next to each call bit for bit.
"""
import math
import re

import numpy as np
import pytest

import list_edges as le
import sink_trees as st
from golden_util import close
from test_hip_root_search import EVERY, USUAL, same

pytestmark = pytest.mark.gpu
REL = 1e-9
MODELS = st.MODELS                                                           # the five standard modes and two local models
WORST = {}                                                                   # call -> the largest deviation over its bound seen


@pytest.fixture(scope="module")
def ctx():
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref = le.reference()
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20)
    o = Oracle(ref, le.ROOT_FREQS)
    yield dev, o, {}
    print("\nlargest deviation from the oracle over its bound, per call:", {k: f"{v:.3g}" for k, v in WORST.items()})
    dev.close()


def use(ctx, name):
    dev, o, corp = ctx
    mode, kw = MODELS[name]
    dev.set_model(**kw)
    o.set_model(**kw)
    if mode not in corp:
        corp[mode] = le.corpus(mode)
    return dev, o, corp[mode]


class Uploaded:
    """a tree of sink_trees in the arena and in the library, under an arena mark of its own"""

    def __init__(self, dev, t):
        self.dev, self.t = dev, t

    def __enter__(self):
        self.mark = self.dev.mark()
        return self.t.host_tree().upload(self.dev)

    def __exit__(self, *exc):
        self.dev.release(self.mark)


def note(call, deviation, bound):
    deviation = abs(float(deviation))
    WORST[call] = max(WORST.get(call, 0.0), 0.0 if deviation == 0.0 else deviation / bound if bound else math.inf)


def check_root_search(dev, o, t, must_score=None):
    """the per-branch scores of maple_tree_find_best_root on t against the twin, and its 4-tuple against the Python path's"""
    from maple_amd.tree_host import find_best_root, find_best_root_native
    why = {}
    want = st.oracle_root_scores(o, t, why=why)
    with Uploaded(dev, t) as tree:
        nm = tree.n_minor if any(tree.n_minor) else None
        before = dev.stats()
        score = dev.tree_find_best_root(nm, **EVERY)[3]                      # (it returns: MAPLE_OK)
        assert dev.stats() == before
        assert sorted(np.nonzero(~np.isnan(score))[0].tolist()) == sorted(want)
        for v, (sc, terms) in want.items():
            bound = REL * sum(abs(x) for x in terms)
            note("find_best_root", score[v] - sc, bound)
            assert abs(score[v] - sc) <= bound, (v, score[v], sc, terms)
        for kw in (EVERY, USUAL):
            py = find_best_root(dev, tree, **kw)
            got = find_best_root_native(dev, tree, **kw)
            assert dev.stats() == before
            assert same(got, py), (got[0], got[1], got[3], py[0], py[1], py[3])
    if must_score is not None:
        assert len(want) >= must_score
    return want, why


FAMILIES = [(m, f) for m in MODELS for f in st.GADGET_FAMS if f != "sink_flag" or MODELS[m][1].get("usingErrorRate")]


@pytest.mark.parametrize("mode,fam", FAMILIES)
def test_find_best_root_on_gadgets(ctx, mode, fam):
    """One five-node tree per case of the family.  The carry families score both sides of every tree, merge_underflow none;
    sink_abandon gives up exactly the sides it is built to give up, for the reason it is built for, and leaves what is below
    them unscored."""
    dev, o, corp = use(ctx, mode)
    gadgets = st.family_gadgets(o, corp, fam)
    scored = 0
    for c, t in zip(corp[fam], gadgets):
        want, why = check_root_search(dev, o, t)
        k0, k1 = st.gadget_sides(t)
        scored += (k0 in want) + (k1 in want)
        if fam == "sink_abandon":
            for name, v in (("k0", k0), ("k1", k1)):
                assert (why.get(v, "scored") == c["expect"][name]) and ((v in want) == (c["expect"][name] == "scored")), c["name"]
                below = t.children[v]
                assert below and all((w in want) == (v in want) for w in below), c["name"]
    assert scored == (0 if fam == "merge_underflow" else 2 if fam == "sink_abandon" else 2 * len(gadgets))


@pytest.mark.parametrize("mode", list(MODELS))
def test_find_best_root_minor_sequences(ctx, mode):
    """The merge_carry trees whose non-tip sides are leaves with two minor sequences: c2's count reaches k_root_up as what is handed
    from above (pmin), k0's and k1's reach every kernel.  Under an error model a count enters every merge its node takes part in
    (M:4489-4493); c2's is in the root's own merge and in upVect's, so it cancels in a score unless one of the two drops it."""
    dev, o, corp = use(ctx, mode)
    trees = st.family_gadgets(o, corp, "merge_carry", minor=(0, 1, 2))
    assert sum(t.n_minor[t.mark["c2"]] == 2 for t in trees) >= 4 and sum(t.n_minor[t.mark["k1"]] == 2 for t in trees) >= 4
    for t in trees:
        check_root_search(dev, o, t, must_score=2)


@pytest.mark.parametrize("mode", list(MODELS))
def test_find_best_root_materialising(ctx, mode):
    """The merge_carry and long trees with a mutation list on the root: no item may use the sink, every new root's list is written
    (k_root_new_list), committed, passed up (maple_pass_branch_batch) and summed (maple_root_prob_batch); the tree log-likelihood's
    root term goes through the same pass."""
    from maple_amd.tree_host import tree_log_likelihood
    dev, o, corp = use(ctx, mode)
    rng = np.random.default_rng(7)
    for fam in ("merge_carry", "long"):
        for t in st.family_gadgets(o, corp, fam):
            st.with_root_mutations(t, rng)
            want, _ = check_root_search(dev, o, t, must_score=2)
            _, contrib, root_term = st.oracle_tree_lk(o, t)
            with Uploaded(dev, t) as tree:
                total, root = dev.tree_log_lk(None)
                assert (total, root) == tree_log_likelihood(dev, tree)
            note("tree_log_lk root", root - root_term, REL * abs(root_term))
            assert close(root, root_term, REL), (root, root_term)


@pytest.mark.parametrize("mode", list(MODELS))
def test_find_best_root_deep(ctx, mode):
    """A caterpillar of heavy lists: upVect handed down four levels, lists of several hundred entries committed and read again, the
    scratch slots of k_root_up nearly full."""
    dev, o, corp = use(ctx, mode)
    deep = st.deep_gadget(o, corp)
    assert min(len(deep.probVect[v]) for v in deep.mark["inner"]) > 300
    check_root_search(dev, o, deep, must_score=12)


@pytest.mark.parametrize("mode", list(MODELS))
def test_find_best_root_wide(ctx, mode):
    """Forty five-node trees (44 under an error model) below one balanced backbone: more than 32 items on a level, so more than
    64 slots in one launch of k_root_up / k_root_new."""
    dev, o, corp = use(ctx, mode)
    wide = st.gadget_grove(o, corp)
    assert len(wide.mark["roots"]) >= 40 and max(st.level_sizes(wide)) > 32
    check_root_search(dev, o, wide, must_score=300)


@pytest.mark.parametrize("mode", list(MODELS))
def test_tree_log_lk_cherry_comb(ctx, mode):
    from maple_amd.tree_host import tree_log_likelihood
    dev, o, corp = use(ctx, mode)
    t = st.standard_comb(o, corp)
    order, contrib, root_term = st.oracle_tree_lk(o, t, known=t.mark["contrib"])
    want = dict(zip(order, contrib))
    cherries = t.mark["cherry"]
    assert len(cherries) == st.N_COMB and len(order) > 3 * 256 and len(order) % 64 != 0
    with Uploaded(dev, t) as tree:
        assert any(tree.n_minor[a] or tree.n_minor[b] for _, a, b in cherries)
        before = dev.stats()
        total, root, node = dev.tree_log_lk(tree.n_minor, per_node=True)
        assert dev.stats() == before
        for v in order:                                                      # the cherries, and the backbone and the trivial pairs as well
            note("tree_log_lk node", node[v] - want[v], REL * abs(want[v]))
            assert close(float(node[v]), want[v], REL), (v, node[v], want[v])
        assert all(node[v] == 0.0 for v in range(t.n) if v not in want)
        note("tree_log_lk root", root - root_term, REL * abs(root_term))
        assert close(root, root_term, REL)
        a = np.asarray([x[1] for x in cherries])
        b = np.asarray([x[2] for x in cherries])
        tip, nm, dist = np.asarray(t.tips()), np.asarray(t.n_minor, dtype=np.int32), np.asarray(t.dist)
        mark = dev.mark()
        out, lk = dev.merge_batch(tree.id_lower[a], dist[a], tip[a], tree.id_lower[b], dist[b], tip[b], False, returnLK=True,
                                  numMinor1=nm[a], numMinor2=nm[b])
        dev.release(mark)
        assert (out >= 0).all() and np.array_equal(node[np.asarray([x[0] for x in cherries])], lk)     # bit for bit
        s = 0.0
        for v in order:
            s += float(node[v])
        assert total == s + root == tree_log_likelihood(dev, tree)[0]
        if MODELS[mode][1].get("usingErrorRate"):                            # the minor-sequence counts are read
            assert dev.tree_log_lk(None)[0] != total


@pytest.mark.parametrize("mode", list(MODELS))
def test_tree_log_lk_underflow(ctx, mode):
    """Two cherries whose running factor falls below DBL_MIN: the call fails naming the one the reference meets first, which has
    the larger node id; with real branch lengths the same tree has a value."""
    from maple_amd.abi import MapleError
    from maple_amd.tree_host import tree_log_likelihood, tree_log_likelihood_native
    dev, o, corp = use(ctx, mode)
    t = st.underflow_comb(o, corp)
    first, second = (t.mark["cherry"][k] for k in st.UNDERFLOW_AT)
    order = st.lk_order(t)
    assert order.index(first[0]) < order.index(second[0]) and first[0] > second[0]
    with pytest.raises(RuntimeError):
        st.oracle_tree_lk(o, t)
    with Uploaded(dev, t) as tree:
        before = dev.stats()
        with pytest.raises(MapleError) as e:
            tree_log_likelihood_native(dev, tree)
        assert e.value.code == MapleError.ERR_FATAL
        assert [int(x) for x in re.findall(r"node (\d+)", str(e.value))] == [first[0]], str(e.value)
        assert dev.stats() == before
        for _, a, b in (first, second):
            tree.dist[a] = tree.dist[b] = t.dist[a] = t.dist[b] = 1e-4
        tree.upload_topology(dev)
        got = tree_log_likelihood_native(dev, tree)
        assert got == tree_log_likelihood(dev, tree) and math.isfinite(got[0])
        _, contrib, root_term = st.oracle_tree_lk(o, t)
        s = 0.0
        for x in contrib:
            s += x
        assert abs(got[0] - (s + root_term)) <= REL * (sum(abs(x) for x in contrib) + abs(root_term))
