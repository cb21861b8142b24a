"""maple_spr_search_batch against the C oracle's search (Oracle.spr_worker) on the search's own rare arms: the None merges of
findBestParentTopology going down, crawling up and over the root, both stop rules, the five exits of the refinement, status -1
with its count of calls, status 2, the vetoes of the worker's accept rule and the in-place shorten of the removed list.  The
reference's recorded trees take none of the -1 exits and none of the vetoes (tests/test_search_trees.py holds the table); the
thirteen-node gadgets of tests/search_trees.py do, in every model mode, and once more with a mutation list on the root, which
makes the library run its instantiations for trees with local references.

Every gadget is searched in every form the header says cannot change results (FORMS).  Bars: status, bestNode, placement and
nAppend exact; bestScore, currentLK, improvement and blen within rtol 1e-11, atol 1e-15 of the oracle's (the bar of
test_hip_search.py); bestRemovedPartials at lists_match's 1e-9; form against form and call against call bit for bit.  The
forms meant to stay in the frontier tier must not hand a search to the one-lane kernel (maple_debug_frontier_handbacks), but
the shorten gadgets for the reason they are built for.  No call changes the arena's counts, with one exception the library
documents where it makes them (ensure_cand_root, spr_batch.hip): on a tree with mutation lists the first call that scores
whole-tree searches keeps the candidates' root-frame copies in the arena, once per uploaded tree; the call after it adds nothing.
"""
import numpy as np
import pytest

import list_edges as le
import search_trees as sts
from golden_util import lists_match

pytestmark = pytest.mark.gpu
FIELDS_EXACT = ("status", "bestNode", "placement", "nAppend")
FIELDS_CLOSE = ("bestScore", "currentLK", "improvement", "blen")
# name -> (maple_tuning, search parameters)
FORMS = {
    "auto": ({}, {}),
    "wave_all": (dict(wave_all_below=1 << 30), {}),
    "wave_none": (dict(wave_all_below=-1), {}),
    "no_wide": ({}, dict(wide_search_budget=-1)),
    "one_lane": ({}, dict(search_tier=1)),
    "wide": ({}, dict(wide_search_budget=1)),
    "wide_outside": (dict(wide_outside_frontier=True), dict(wide_search_budget=1)),
    "wide_dense": (dict(dense_wide_scoring=True), dict(wide_search_budget=1)),
    "wide_no_scan": (dict(no_clade_scan=True), dict(wide_search_budget=1)),
}
FRONTIER_FORMS = ("auto", "wave_all", "wave_none", "no_wide")       # the frontier tier itself has to answer
WIDE_FORMS = ("wide", "wide_outside", "wide_dense", "wide_no_scan")
LARGE = 70
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref = le.reference()
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=64 << 20, debug=True)
    o = Oracle(ref, le.ROOT_FREQS)
    yield dev, o
    print("\nlargest deviation from the oracle over its bound, per field:", {k: f"{v:.3g}" for k, v in WORST.items()})
    dev.set_tuning()
    dev.close()


def same_bits(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in FIELDS_EXACT + FIELDS_CLOSE)


def diff(a, b):
    """the first search two results differ in, field by field"""
    for i in range(len(a["status"])):
        if any(np.asarray(a[k][i]).tobytes() != np.asarray(b[k][i]).tobytes() for k in FIELDS_EXACT + FIELDS_CLOSE):
            return i, {k: (a[k][i].tolist(), b[k][i].tolist()) for k in FIELDS_EXACT + FIELDS_CLOSE}


def check_gadget(dev, o, g):
    """Every form on a batch of the gadget's own searches and on one of LARGE of them (the same searches over and over): above 64
    searches k_fr_replay walks the laid-out items, the form that emulates an exact shorten and names its hand-backs."""
    few = np.asarray(g.nodes, dtype=np.int32)
    batches = (("few", few, g.handback[0]), ("many", np.resize(few, LARGE), g.handback[1]))
    want = {"few": o.spr_worker(g.tree.oracle_tree(o), few, want_removed_partials=True, **g.params)}
    want["many"] = {k: (v * LARGE)[:LARGE] if isinstance(v, list) else np.resize(v, (LARGE,) + v.shape[1:])
                    for k, v in want["few"].items()}                         # (the same searches: the same answers, in the same order)
    has_mut, copies_made = any(g.tree.mutations), False
    mark = dev.mark()
    try:
        g.tree.host_tree().upload(dev)
        for size, nodes, reason in batches:
            w = want[size]
            first = None
            for form, (tuning, extra) in FORMS.items():
                dev.set_tuning(**tuning)
                before = dev.stats()
                got = dev.spr_search_batch(nodes, **g.params, **extra)
                where = (g.name, size, form)
                if dev.stats() != before:                                   # (see the module's docstring)
                    assert has_mut and (form in WIDE_FORMS or g.whole_tree) and not copies_made, \
                        ("the arena changed", where, before, dev.stats())
                    copies_made = True
                if form in FRONTIER_FORMS:
                    n_back, reasons = dev.frontier_handbacks()
                    if reason is None:
                        assert n_back == 0, (where, n_back, reasons)
                    else:
                        assert n_back >= 1 and reasons[reason] == n_back, (where, n_back, reasons)
                    if np.any((w["status"] == 0) | (w["status"] == -1)) and (form == "no_wide" or not g.whole_tree):
                        assert dev.frontier_levels()[0].sum() > 0, ("no updating item", where)
                for k in FIELDS_EXACT:
                    assert np.array_equal(got[k], w[k]), (where, k, got[k], w[k])
                for k in FIELDS_CLOSE:
                    bound = 1e-15 + 1e-11 * np.abs(w[k])
                    with np.errstate(invalid="ignore"):
                        over = np.where(got[k] == w[k], 0.0, np.abs(got[k] - w[k]) / bound)
                    WORST[k] = max(WORST.get(k, 0.0), float(np.max(over)))
                    assert np.allclose(got[k], w[k], rtol=1e-11, atol=1e-15), (where, k, got[k], w[k])
                before = dev.stats()
                again = dev.spr_search_batch(nodes, **g.params, **extra)
                assert dev.stats() == before, ("the arena changed", where, before, dev.stats())
                assert same_bits(got, again), ("two calls differ", where, diff(got, again))
                if first is None:
                    first = got
                assert same_bits(got, first), ("two forms differ", where, diff(got, first))
                if size == "many" and form != "auto":
                    continue
                inner = dev.mark()
                with_rpr = dev.spr_search_batch(nodes, want_removed_partials=True, **g.params, **extra)
                assert same_bits(got, with_rpr), ("with removed partials", where, diff(got, with_rpr))
                rpr = dev.download(with_rpr["removedPartials"])
                dev.release(inner)
                for k in range(len(nodes)):
                    if w["status"][k] == 0:
                        assert lists_match(rpr[k], w["removedPartials"][k], 1e-9), (where, k, rpr[k], w["removedPartials"][k])
        return want["few"]
    finally:
        dev.set_tuning()
        dev.release(mark)


@pytest.mark.parametrize("mat", [False, True], ids=["plain", "root_mutations"])
@pytest.mark.parametrize("mode", le.MODES[:5])
def test_spr_search_on_gadgets(ctx, mode, mat):
    dev, o = ctx
    kw = le.model(mode)
    dev.set_model(**kw)
    o.set_model(**kw)
    status = []
    for g in sts.gadgets(o, mode, mat):
        want = check_gadget(dev, o, g)
        status += want["status"].tolist()
    assert {0, -1, 2} <= set(status)
