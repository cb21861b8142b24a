"""The EM step on the GPU (maple_em_expectation / maple_em_rates, maple_amd/csrc/em.hip) against the reference's
expectationMaximizationCalculationRates (M:10077-10947) as recorded in tests/golden/em_*.json.gz: trees of the reference's own
runs and hand-built caterpillar trees that reach every arm of its walk (tests/test_em_fixtures.py checks that they do).

Whole-number statistics must match exactly; floats must satisfy |a - b| <= 1e-9 * max(|b|, scale), scale = the largest
magnitude of the recorded table (1e-9: the project's standing GPU-float tolerance)."""
import numpy as np
import pytest

import em_util
from golden_util import model_args

pytestmark = pytest.mark.gpu

NAMES = [n for n in em_util.fixture_names() if "ret" in em_util.load(n)]
RAISING = [n for n in em_util.fixture_names() if "ret" not in em_util.load(n)]
FLOAT_TABLES = ("counts", "waitingTimes", "waitingTimesSites", "countsSites", "trackingNs", "errorCountSites")


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


@pytest.fixture(scope="module", params=NAMES)
def env(request):
    fx = em_util.load(request.param)
    dev = make_device(fx)
    dev.set_model(**model_args(fx["model"]))
    tree = host_tree(fx["tree"]).upload(dev)
    yield fx, dev, tree
    dev.close()


def check_raw(got, raw, model, label=""):
    assert got["numTips"] == raw["numTips"], label
    if model["usingErrorRate"]:
        assert got["observedTotNucsSites"] == raw["observedTotNucsSites"], label
    if model["errorRateSiteSpecific"]:
        assert np.array_equal(got["observedNucsSites"], np.asarray(raw["observedNucsSites"], dtype=np.float64)), label
    worst = {}
    for k in FLOAT_TABLES:
        if k in raw:
            worst[k] = em_util.table_close(got[k], raw[k])
    for k in ("errorCount", "totTreeLength"):
        if k in raw:
            worst[k] = em_util.table_close([got[k]], [raw[k]])
    print(label, "worst |a-b| / bound per table:", {k: f"{v:.3g}" for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (label, worst)


def check_rates(got, fx, label=""):
    ret, L = fx["ret"], fx["context"]["lRef"]
    Q, sr, er, se = got
    assert em_util.table_close(Q, ret["Q"]) <= 1.0, label
    for g, w, clamps in ((sr, ret["siteRates"], (0.001, 0.005 * L)), (se, ret["siteErrRates"], (1e-10,))):
        assert (g is None) == (w is None), label                         # None shapes are preserved
        if w is not None:
            assert em_util.table_close(g, w) <= 1.0, label
            g, w = np.asarray(g), np.asarray(w)
            for c in clamps:                                             # clamped values are hit exactly where the reference hits them
                assert np.array_equal(np.nonzero(g == c)[0], np.nonzero(w == c)[0]), (label, c)
    assert (er is None) == (ret["errorRate"] is None), label
    if er is not None:
        assert em_util.table_close([er], [ret["errorRate"]]) <= 1.0, label


def test_raw_statistics(env):
    fx, dev, tree = env
    arena = dev.stats()
    check_raw(dev.em_expectation(tree.n_minor), fx["raw"], fx["model"], fx["name"])
    assert dev.stats() == arena                                          # the call's temporaries are released


def test_rates(env):
    from maple_amd.ops import TreeOps
    from maple_amd.tree_host import estimate_rates
    fx, dev, tree = env
    model = fx["model"]["emModel"]
    check_rates(dev.em_rates(tree.n_minor, model), fx, fx["name"] + " em_rates")
    got = estimate_rates(dev, tree, model)
    assert isinstance(got[0], list) and len(got[0]) == 4 and all(isinstance(r, list) for r in got[0])
    check_rates(got, fx, fx["name"] + " estimate_rates")
    check_rates(TreeOps(dev, tree).expectationMaximizationCalculationRates(model), fx, fx["name"] + " adapter")


@pytest.mark.parametrize("name", [n for n in NAMES if "lkAfterOneRound" in em_util.load(n)])
def test_log_likelihood_after_one_round(name):
    from maple_amd.tree_host import estimate_rates, rebuild_genome_lists, tree_log_likelihood
    fx = em_util.load(name)
    dev = make_device(fx)
    try:
        dev.set_model(**model_args(fx["model"]))
        tree = host_tree(fx["tree"]).upload(dev)
        Q, sr, er, se = estimate_rates(dev, tree, fx["model"]["emModel"])
        assert er is None and se is None
        dev.set_model(Q, siteRates=sr)
        tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp = rebuild_genome_lists(dev, tree)
        lk = tree_log_likelihood(dev, tree)[0]
        want = fx["lkAfterOneRound"]
        print(name, "LK after one round of EM:", lk, "recorded", want)
        assert abs(lk - want) <= 1e-9 * abs(want)
    finally:
        dev.close()


def permuted(t, seed):
    """The tree snapshot with its node ids permuted at random."""
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
    return out


def test_node_ids_permuted():
    fx = em_util.load("cat_a_full")
    dev = make_device(fx)
    try:
        dev.set_model(**model_args(fx["model"]))
        t = permuted(fx["tree"], 7)
        assert t["root"] != fx["tree"]["root"] or t["up"] != fx["tree"]["up"]
        tree = host_tree(t).upload(dev)
        first = dev.em_expectation(tree.n_minor)
        check_raw(first, fx["raw"], fx["model"], "cat_a_full permuted")
        check_rates(dev.em_rates(tree.n_minor, "UNREST"), fx, "cat_a_full permuted")
        second = dev.em_expectation(tree.n_minor)
        for k in ("counts", "waitingTimes", "errorCount", "totTreeLength", "observedTotNucsSites", "numTips", "observedNucsSites"):
            assert np.array_equal(np.asarray(first[k]), np.asarray(second[k])), k     # bit-identical totals on the same upload
    finally:
        dev.close()


def walked_branches(fx):
    t, u = fx["tree"], fx["model"]["usingErrorRate"]
    return sum(1 for v in range(t["n"]) if t["up"][v] is not None and (t["dist"][v] or (u and not t["children"][v])))


def test_ragged_blocks_fixture_shape():
    """cat_b fills more than one block of 256 branches and leaves a partly filled last wavefront, in every mode (the statistics
    themselves are checked by test_raw_statistics)."""
    for mode in ("plain", "ratevar", "gerr", "full"):
        nb = walked_branches(em_util.load(f"cat_b_{mode}"))
        assert nb > 256 and nb % 64 != 0, (mode, nb)


def test_error_paths():
    from maple_amd.runtime import MapleError
    fx = em_util.load("cat_zero_plain")
    dev = make_device(fx, arena=64 << 20)
    try:
        with pytest.raises(MapleError) as e:                             # no tree (and no model)
            dev.em_expectation()
        assert e.value.code == MapleError.ERR_STATE
        dev.set_model(**model_args(fx["model"]))
        with pytest.raises(MapleError) as e:                             # a model, no tree
            dev.em_rates()
        assert e.value.code == MapleError.ERR_STATE
        tree = host_tree(fx["tree"]).upload(dev)
        with pytest.raises(MapleError) as e:                             # M:10877: neither UNREST nor GTR, no error model
            dev.em_rates(tree.n_minor, 2)
        assert e.value.code == MapleError.ERR_ARG
        with pytest.raises(MapleError) as e:
            dev.em_rates(tree.n_minor, "JC")
        assert e.value.code == MapleError.ERR_ARG
        a, b = dev.em_expectation(None), dev.em_expectation([0] * tree.n)    # nMinor = NULL is an all-zero array
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])) or k in ("waitingTimesSites", "countsSites", "trackingNs", "errorCountSites"), k
        assert a["numTips"] == sum(1 for c in fx["tree"]["children"] if not c)
    finally:
        dev.close()
    fx = em_util.load("cat_zero_gerr")                                   # with an error model any model value goes through
    dev = make_device(fx, arena=64 << 20)
    try:
        with pytest.raises(MapleError) as e:                             # a tree, no model
            host_tree(fx["tree"]).upload(dev)
            dev.em_expectation()
        assert e.value.code == MapleError.ERR_STATE
        dev.set_model(**model_args(fx["model"]))
        tree = host_tree(fx["tree"]).upload(dev)
        Q, sr, er, se = dev.em_rates(tree.n_minor, 2)
        assert sr is None and se is None and er is not None and np.all(np.isfinite(Q))
    finally:
        dev.close()


@pytest.mark.parametrize("name", RAISING)
def test_negative_probability_is_fatal(name):
    """Where the reference raises Exception("exit") on a negative probability (M:10293 and its kin): MAPLE_ERR_FATAL."""
    from maple_amd.runtime import MapleError
    fx = em_util.load(name)
    assert fx["raised"] and "exit" in fx["raised"]
    dev = make_device(fx)
    try:
        dev.set_model(**model_args(fx["model"]))
        tree = host_tree(fx["tree"]).upload(dev)
        with pytest.raises(MapleError) as e:
            dev.em_rates(tree.n_minor, "UNREST")
        assert e.value.code == MapleError.ERR_FATAL
    finally:
        dev.close()
