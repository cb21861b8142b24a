"""GPU checks at BASELINE-like sizes through properties that do not depend on the size (the reference cannot be run
at these sizes in minutes; the C oracle, itself pinned to the reference's golden calls, is the checker on samples):

* model modes of configs[2] and configs[3]: UNREST + per-site rates, + per-site error rates;
* the query-major kernel against the oracle on a seeded sample of (query, candidate) pairs of a 10 000-tip tree;
* tree log-likelihood of the whole GPU-built mirror against the oracle's post-order sum;
* passGenomeListThroughBranch up then down restores the list (after shorten);
* shorten is idempotent; a list is never "different" from itself; merging is symmetric in the likelihood it returns.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = [[-0.5524, 0.0602, 0.3655, 0.1267], [0.1666, -2.6077, 0.0405, 2.4006],
     [0.8421, 0.1305, -2.4012, 1.4286], [0.0688, 0.4849, 0.0502, -0.6039]]


def world_model_kwargs(mode, l_ref, seed=2):
    rng = np.random.default_rng(seed + 100)
    kw = dict(Q=Q)
    if mode != "unrest":
        kw["siteRates"] = np.clip(rng.gamma(0.5, 2.0, size=l_ref), 0.001, 0.005 * l_ref)
    if mode == "siteerr":
        er = np.exp(rng.uniform(math.log(1e-10), math.log(1e-3), size=l_ref))
        kw.update(usingErrorRate=True, errorRates=er, errorRateGlobal=float(er.mean()))
    return kw


def build(n_tips, mode, seed=2, **dev_kw):
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_mirror import TreeMirror
    from oracle.oracle_py import Oracle
    data = make_dataset(n_samples=n_tips, l_ref=29903, seed=seed, mean_diffs=30.0, rate_variation=(mode != "unrest"),
                        frac_with_n=0.05, frac_ambig=0.05)
    ref_idx, rf = reference_tables(data.ref)
    kw = world_model_kwargs(mode, len(ref_idx), seed)
    dev = Device(ref_idx, rf, **dict(dict(arena_bytes=3 << 30), **dev_kw))
    dev.set_model(**kw)
    orc = Oracle(ref_idx, rf)
    orc.set_model(**kw)
    tip_kw = dict(error_rates=kw["errorRates"]) if mode == "siteerr" else {}
    tips = {int(v): tip_genome_list(dl, ref_idx, **tip_kw) for v, dl in zip(data.tip_node, data.diffs)}
    mirror = TreeMirror(dev, data.parent, data.blen, tips).build()
    return data, dev, orc, mirror


@pytest.fixture(scope="module", params=["unrest", "ratevar", "siteerr"])
def world(request):
    n = 10000 if request.param == "unrest" else 3000
    data, dev, orc, mirror = build(n, request.param)
    yield request.param, data, dev, orc, mirror
    dev.close()


def rel(a, b):
    if a == b:
        return 0.0
    return abs(a - b) / max(1.0, abs(a), abs(b))


def test_query_major_kernel_vs_oracle_sample(world):
    import torch
    mode, data, dev, orc, mirror = world
    l_ref = dev.lRef
    cand = mirror.candidate_nodes(1.0 / (10 * l_ref))
    q_nodes = np.asarray(data.tip_node[:64])
    cu = torch.device("cuda", 0)
    t_q = torch.from_numpy(mirror.lower[q_nodes].astype(np.int32)).to(cu)
    t_c = torch.from_numpy(mirror.tot_up[cand].astype(np.int32)).to(cu)
    out = torch.empty(len(q_nodes) * len(cand), dtype=torch.float64, device=cu)
    torch.cuda.synchronize()
    dev.append_queries_dev(len(q_nodes), t_q.data_ptr(), len(cand), t_c.data_ptr(), True, 1.0 / l_ref, out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(q_nodes), len(cand))
    assert np.isfinite(got).mean() > 0.99
    rng = np.random.default_rng(5)
    qi = rng.integers(len(q_nodes), size=400)
    ci = rng.integers(len(cand), size=400)
    q_lists = dev.download(mirror.lower[q_nodes])
    keys = sorted(set(ci.tolist()))
    c_lists = dict(zip(keys, dev.download(mirror.tot_up[cand[keys]])))
    worst = 0.0
    for a, b in zip(qi, ci):
        want = orc.appendProbNode(c_lists[int(b)], q_lists[int(a)], True, 1.0 / l_ref)
        g = float(got[a, b])
        if math.isinf(want):
            assert math.isinf(g)
        else:
            worst = max(worst, rel(g, want))
    assert worst < 1e-12, worst
    # each query scored against its own branch must be (one of) its best placements: the tree was built from the truth
    own = np.asarray([np.nonzero(cand == v)[0][0] if (cand == v).any() else -1 for v in q_nodes])
    ok = own >= 0
    best = got.max(axis=1)
    assert (got[np.arange(len(q_nodes))[ok], own[ok]] >= best[ok] - 25.0).mean() > 0.9


def test_tree_log_likelihood_vs_oracle(world):
    mode, data, dev, orc, mirror = world
    n = mirror.n_nodes
    ch = mirror.children
    internal = [v for v in range(n) if ch[v, 0] >= 0]
    c0, c1 = ch[internal, 0], ch[internal, 1]
    out, lk = dev.merge_batch(mirror.lower[c0], mirror.dist[c0], mirror.is_tip[c0], mirror.lower[c1], mirror.dist[c1],
                              mirror.is_tip[c1], False, returnLK=True)
    assert (out >= 0).all()
    root_lk = float(dev.root_prob_batch([mirror.lower[mirror.root]])[0])
    total = float(lk.sum()) + root_lk
    # oracle on a seeded sample of internal nodes + the root
    rng = np.random.default_rng(9)
    pick = rng.choice(len(internal), size=150, replace=False)
    lists0 = dev.download(mirror.lower[c0[pick]])
    lists1 = dev.download(mirror.lower[c1[pick]])
    merged = dev.download(out[pick])
    for k, i in enumerate(pick):
        res, want = orc.mergeVectors(lists0[k], mirror.dist[c0[i]], bool(mirror.is_tip[c0[i]]), lists1[k],
                                     mirror.dist[c1[i]], bool(mirror.is_tip[c1[i]]), returnLK=True)
        assert rel(float(lk[i]), want) < 1e-12
        assert len(res) == len(merged[k]) and all(x[0] == y[0] and x[1] == y[1] for x, y in zip(res, merged[k]))
    want_root = orc.findProbRoot(dev.download([mirror.lower[mirror.root]])[0], [[]])
    assert rel(root_lk, want_root) < 1e-12
    assert math.isfinite(total) and total < 0
    # symmetry: swapping the two children gives the same likelihood contribution
    out2, lk2 = dev.merge_batch(mirror.lower[c1[pick]], mirror.dist[c1[pick]], mirror.is_tip[c1[pick]],
                                mirror.lower[c0[pick]], mirror.dist[c0[pick]], mirror.is_tip[c0[pick]], False, returnLK=True)
    assert np.allclose(lk2, lk[pick], rtol=1e-12, atol=0)


def test_structural_properties(world):
    mode, data, dev, orc, mirror = world
    rng = np.random.default_rng(3)
    ids = mirror.tot_up[mirror.candidate_nodes(0.0)][:2000]
    mark = dev.mark()
    # shorten is idempotent and a list never differs from itself or from its shortened form
    s1 = dev.shorten_batch(ids)
    s2 = dev.shorten_batch(s1)
    n1, _ = dev.sizes(s1)
    n2, _ = dev.sizes(s2)
    assert np.array_equal(n1, n2)
    assert not dev.differ_batch(ids, ids).any()
    assert not dev.differ_batch(ids, s1).any()
    # a change of reference frame and back restores the list
    muts = []
    nuc = {"a": 0, "c": 1, "g": 2, "t": 3}
    for _ in range(len(ids)):
        pos = sorted(rng.choice(dev.lRef, size=5, replace=False) + 1)
        ml = []
        for p in pos:
            r = nuc[data.ref[p - 1]]
            ml.append((int(p), r, int((r + 1 + rng.integers(3)) % 4)))
        muts.append(ml)
    mids = dev.upload_mutations(muts)
    down = dev.pass_branch_batch(ids, mids, False)
    back = dev.shorten_batch(dev.pass_branch_batch(down, mids, True))
    a = dev.download(s1[:300])
    b = dev.download(back[:300])
    assert a == b
    dev.release(mark)


def test_batched_placement_equals_single_query_search(world):
    """maple_placement_search_batch (device-side traversal, one lane per query) against the one-query-at-a-time
    PlacementSearcher (host replay) on new samples: same node, score, branch lengths, bestDiffs and the same number of
    reference-equivalent appendProbNode evaluations, in every model mode."""
    from maple_amd.host import tip_genome_list
    from maple_amd.search import PlacementParams, PlacementSearcher
    from maple_amd.synth import perturb_diffs
    from maple_amd.tree_host import HostTree
    mode, data, dev, orc, mirror = world
    l_ref = dev.lRef
    ll = math.log(l_ref)
    tree = HostTree.from_mirror(mirror, dev)
    ps = PlacementSearcher(dev, tree, PlacementParams(oneMutBLen=1.0 / l_ref, effectivelyNon0BLen=1.0 / (10 * l_ref),
                                                      thresholdLogLK=18.0 * ll, thresholdLogLKoptimization=ll,
                                                      thresholdLogLKconsecutivePlacement=1.0,
                                                      onlyFindIdentical=(mode == "siteerr")))
    rng = np.random.default_rng(21)
    from maple_amd.host import reference_tables
    ref_idx, _ = reference_tables(data.ref)
    queries = [tip_genome_list(perturb_diffs(dl, data.ref, rng, n_extra=k % 3), ref_idx)
               for k, dl in enumerate(data.diffs[:48])]                  # every third query is a copy of a tip
    batch = ps.find_best_parent_batch(queries)
    n_minor = 0
    for q, got in zip(queries, batch):
        want = ps.find_best_parent_host_replay(q)
        assert got[0] == want[0] and got[1] == want[1], (got[:2], want[:2])
        assert got[4]["minor"] == want[4]["minor"] and got[4]["n_append"] == want[4]["n_append"]
        if want[2] is None:
            assert got[2] is None
            n_minor += 1
        else:
            assert tuple(0.0 if b is False else b for b in want[2]) == got[2]
        assert got[3] == want[3]
    assert 0 < n_minor < len(queries)


def test_update_partials_on_a_tree_with_local_references(world):
    """maple_update_partials at size, in every model mode, on the tree with MAT local references (lists cross reference
    frames on their way up and down): 150 simultaneous branch-length changes repaired incrementally, then every list of
    the tree against a full rebuild -- "not different" by the reference's own thresholds (areVectorsDifferent, both ways:
    the repair stops where that function says so) -- and the tree log-likelihood of both."""
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree, rebuild_genome_lists, tree_log_likelihood, update_genome_lists
    _, data, dev, orc, mirror = world
    mark = dev.mark()
    tree = HostTree.from_mirror(mirror)
    assert add_local_references(dev, tree, 30) > 10
    rng = np.random.default_rng(17)
    cand = np.nonzero((mirror.parent >= 0) & (mirror.dist > 1e-5))[0]
    pick = rng.choice(cand, size=150, replace=False)
    for v in pick:
        tree.dist[v] = tree.dist[v] * 2.5
    replaced = update_genome_lists(dev, tree, pick.tolist())
    assert replaced > 300
    lk_upd, _ = tree_log_likelihood(dev, tree)
    lo, ur, ul, tu = rebuild_genome_lists(dev, tree)
    for a, b in ((tree.id_lower, lo), (tree.id_upRight, ur), (tree.id_upLeft, ul), (tree.id_totUp, tu)):
        assert np.array_equal(a >= 0, b >= 0)
        ok = a >= 0
        assert not (dev.differ_batch(a[ok], b[ok]) | dev.differ_batch(b[ok], a[ok])).any()
    tree.id_lower, tree.id_upRight, tree.id_upLeft, tree.id_totUp = lo, ur, ul, tu
    lk_full, _ = tree_log_likelihood(dev, tree)
    assert abs(lk_upd - lk_full) <= 1e-9 * abs(lk_full)
    dev.release(mark)


def test_rebuild_inside_the_library_equals_the_python_level_loop(world):
    """maple_tree_rebuild_lists (reCalculateAllGenomeLists, M:6013-6347: the level loop inside the library, one fused
    mergeVectors -> shorten launch per level) against the Python level loop of separate merge / shorten launches: every list of
    the tree entry for entry -- on the tree with MAT local references (lists passed through reference branches) and as
    TreeMirror.build()."""
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree, rebuild_genome_lists
    from maple_amd.tree_mirror import TreeMirror
    _, data, dev, orc, mirror = world
    mark = dev.mark()
    tree = HostTree.from_mirror(mirror)
    assert add_local_references(dev, tree, 30) > 10
    a = rebuild_genome_lists(dev, tree, native=True)
    b = rebuild_genome_lists(dev, tree, native=False)
    for x, y in zip(a, b):
        assert np.array_equal(x >= 0, y >= 0)
        ok = np.nonzero(x >= 0)[0][::3]
        for lx, ly in zip(dev.download(x[ok]), dev.download(y[ok])):
            assert lx == ly
    dev.release(mark)
    mark = dev.mark()
    tips = np.nonzero(mirror.is_tip)[0]
    m1 = TreeMirror(dev, mirror.parent, mirror.dist.copy(), {int(v): l for v, l in zip(tips, dev.download(mirror.lower[tips]))})
    m2 = TreeMirror(dev, mirror.parent, mirror.dist.copy(), {int(v): l for v, l in zip(tips, dev.download(mirror.lower[tips]))})
    m1.build(native=True)
    m2.build(native=False)
    assert np.array_equal(m1.dist, m2.dist)
    for x, y in ((m1.lower, m2.lower), (m1.up_right, m2.up_right), (m1.up_left, m2.up_left), (m1.tot_up, m2.tot_up)):
        assert np.array_equal(x >= 0, y >= 0)
        ok = np.nonzero(x >= 0)[0][::3]
        for lx, ly in zip(dev.download(x[ok]), dev.download(y[ok])):
            assert lx == ly
    dev.release(mark)


def test_wavefront_wide_evaluate_placement_is_the_one_lane_chain_bit_for_bit(world, monkeypatch):
    """k_evalplace_wave (one wavefront per item: the three branch-length solves, three merges and the append of
    evaluatePlacement, M:6790-6806, each cut along its merge path) against k_evalplace (one lane per item), in every model
    mode: 600 (branch, sample) pairs -- the sample's own neighbourhood and random branches -- must give the same four
    numbers, bit for bit; and single-query placement searches (which also fold the refinement's two comparison scores into
    that launch) the same results either way."""
    mode, data, dev, orc, mirror = world
    rng = np.random.default_rng(31)
    l_ref = dev.lRef
    nodes = rng.choice(np.nonzero(mirror.parent >= 0)[0], size=600, replace=False)
    par = mirror.parent[nodes]
    up_ids = np.where(mirror.children[par, 0] == nodes, mirror.up_right[par], mirror.up_left[par]).astype(np.int32)
    tips = np.asarray(data.tip_node)
    # half of the samples next to the branch (its own subtree's first tip), half anywhere
    q_nodes = rng.choice(tips, size=600)
    q_ids = mirror.lower[q_nodes].astype(np.int32)
    args = (mirror.tot_up[nodes], mirror.lower[nodes], up_ids, mirror.dist[nodes], q_ids, True, mirror.is_tip[nodes])
    ok = (mirror.tot_up[nodes] >= 0) & (up_ids >= 0)
    args = tuple(a[ok] if isinstance(a, np.ndarray) else a for a in args)
    wave = dev.evaluate_placement_batch(*args)
    dev.set_tuning(wave_per_item_max=-1)
    lane = dev.evaluate_placement_batch(*args)
    dev.set_tuning()
    assert wave.shape == lane.shape and len(wave) > 300
    assert np.array_equal(wave.view(np.uint64), lane.view(np.uint64)), np.nonzero((wave != lane).any(axis=1))[0][:5]
    assert np.isfinite(wave[:, 1:]).all() and (wave[:, 1:] >= 0).all()
    # the search around it
    ll = math.log(l_ref)
    pkw = dict(oneMutBLen=1.0 / l_ref, effectivelyNon0BLen=1.0 / (10 * l_ref), thresholdLogLK=18.0 * ll,
               thresholdLogLKoptimization=ll, thresholdLogLKconsecutivePlacement=1.0)
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.synth import perturb_diffs
    ref_idx, _ = reference_tables(data.ref)
    mark = dev.mark()
    dev.upload_tree(mirror.root, mirror.parent, mirror.children[:, 0], mirror.children[:, 1], mirror.dist, mirror.is_tip,
                    mirror.lower, mirror.up_right, mirror.up_left, mirror.tot_up, -np.ones(mirror.n_nodes, dtype=np.int32))
    dev.placement_prepare(**pkw)
    qs = dev.upload([tip_genome_list(perturb_diffs(data.diffs[i], data.ref, rng), ref_idx) for i in range(24)])
    res = {}
    for name in ("wave", "lane"):
        if name == "lane":
            dev.set_tuning(wave_per_item_max=-1)
        res[name] = [dev.placement_search_batch(np.asarray([q], dtype=np.int32), **pkw) for q in qs]
    dev.set_tuning()
    for a, b in zip(res["wave"], res["lane"]):
        for k in ("bestNode", "nAppend", "status"):
            assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a["bestScore"].view(np.uint64), b["bestScore"].view(np.uint64))
        assert np.array_equal(a["blen"].view(np.uint64), b["blen"].view(np.uint64))
    dev.release(mark)


def test_explicit_pair_operators_one_wavefront_per_pair_are_the_one_lane_kernels(world, monkeypatch):
    """maple_append_batch, maple_merge_batch (without the likelihood), maple_blen_batch and maple_differ_batch send batches of up to 1 024 pairs --
    a single reference call, a handful of calls -- through one wavefront per pair (k_wave_append, k_merge_wave, k_blen_wave, k_differ_wave);
    in every model mode the scores, lists and lengths must be those of the one-lane kernels, bit for bit."""
    mode, data, dev, orc, mirror = world
    rng = np.random.default_rng(41)
    nodes = rng.choice(np.nonzero(mirror.parent >= 0)[0], size=900, replace=False)
    par = mirror.parent[nodes]
    up_ids = np.where(mirror.children[par, 0] == nodes, mirror.up_right[par], mirror.up_left[par]).astype(np.int32)
    ok = (up_ids >= 0) & (mirror.tot_up[nodes] >= 0)
    nodes, up_ids = nodes[ok], up_ids[ok]
    low, tip, dist = mirror.lower[nodes], mirror.is_tip[nodes], mirror.dist[nodes]
    q = mirror.lower[rng.choice(np.asarray(data.tip_node), size=len(nodes))]
    mark = dev.mark()

    def run():
        return dict(app=dev.append_batch(mirror.tot_up[nodes], q, True, 1.0 / dev.lRef),
                    app2=dev.append_batch(up_ids, low, tip, dist),
                    low=dev.merge_batch(low, dist, tip, q, 1.0 / dev.lRef, True, False),
                    up=dev.merge_batch(up_ids, dist / 2, False, low, dist / 2, tip, True),
                    blen=dev.blen_batch(mirror.tot_up[nodes], q, True), blen2=dev.blen_batch(up_ids, low, tip),
                    dif=dev.differ_batch(low, np.roll(low, 1)), dif2=dev.differ_batch(mirror.tot_up[nodes], mirror.tot_up[nodes]))

    wave = run()
    dev.set_tuning(wave_per_item_max=-1)
    lane = run()
    dev.set_tuning()
    assert len(nodes) > 500
    for k in ("app", "app2"):
        assert np.array_equal(wave[k].view(np.uint64), lane[k].view(np.uint64)), k
    for k in ("blen", "blen2"):
        assert np.array_equal(wave[k][0].view(np.uint64), lane[k][0].view(np.uint64)) and np.array_equal(wave[k][1], lane[k][1]), k
    assert np.array_equal(wave["dif"], lane["dif"]) and wave["dif"].sum() > 400 and not wave["dif2"].any() and not lane["dif2"].any()
    for k in ("low", "up"):
        assert np.array_equal(wave[k] >= 0, lane[k] >= 0), k
        good = wave[k] >= 0
        assert good.sum() > 400 and dev.download(wave[k][good]) == dev.download(lane[k][good]), k
    dev.release(mark)


def exact_list(rng, ref, u, n):
    """A list of exactly n entries in the reference's tuple grammar (tests/list_edges.Builder): an isolated site is two entries
    (the reference run before it and the site), a site next to the one before is one, the run to lRef the last.  The sites are
    nucleotides, O vectors, single positions of N and single positions of the reference with a tail (what shorten() joins)."""
    import list_edges as le
    n_adj = int(rng.integers(20, 60)) * 2 + (n + 1) % 2                   # 2 * sites - adjacent + 1 == n
    n_sites = (n - 1 + n_adj) // 2
    adj = np.zeros(n_sites, dtype=bool)
    adj[rng.choice(np.arange(1, n_sites), size=n_adj, replace=False)] = True
    gap = np.where(adj, 0, 1)                                             # reference positions in front of each site
    free = len(ref) - 1 - n_sites - int(gap.sum())                        # (the last position stays the closing run's)
    iso = np.nonzero(~adj)[0]
    gap[iso] += rng.multinomial(free, np.ones(len(iso)) / len(iso))
    b, p = le.Builder(ref, u), 0
    for k in range(n_sites):
        p += int(gap[k]) + 1
        r, kind = int(ref[p - 1]), rng.random()
        d0 = float(rng.choice([0.0, 1e-5, 3e-4][0 if u else 1:])) if rng.random() < 0.4 else None
        d1 = float(rng.choice([1e-5, 2e-3])) if d0 is not None and rng.random() < 0.3 else None
        if adj[k] and kind < 0.5:
            b.run(4, p, p, d0=float(rng.choice([1e-4, 1e-4 + 1e-10, 2e-4])), flag=bool(rng.random() < 0.8))
        elif adj[k] and kind < 0.6:
            b.run(5, p, p)
        elif kind > 0.85:
            b.o(p, le.o_vec(rng, r, float(rng.uniform(0.01, 0.6))), d0=d0)
        else:
            b.nuc(p, le.other(rng, r), d0=d0, d1=d1, flag=bool(rng.random() < 0.5))
    out = b.done()
    assert len(out) == n
    le.check_grammar(out, len(ref), u)
    return out


def split_runs(gl, k):
    """gl with its last k reference runs without a tail cut in two: k entries more, and no list operator can tell."""
    out, pos, todo = [], [0], k
    for e in gl:
        pos.append(e[1] if e[0] in (4, 5) else pos[-1] + 1)
    for i in range(len(gl) - 1, -1, -1):
        e = gl[i]
        out.append(e)
        if todo and e[0] == 4 and len(e) == 2 and e[1] - pos[i] >= 2:
            out.append((4, e[1] - 1))
            todo -= 1
    assert todo == 0
    return out[::-1]


def change_nucs(rng, gl, k):
    """gl with another nucleotide at its last site and at k - 1 more of its sites that hold one."""
    import list_edges as le
    at = [i for i, e in enumerate(gl) if e[0] < 4]
    out = list(gl)
    for i in [at[-1]] + [int(x) for x in rng.choice(at[:-1], size=k - 1, replace=False)]:
        out[i] = (le.other(rng, gl[i][1], (gl[i][0],)),) + gl[i][1:]
    return out


@pytest.mark.parametrize("mode", ["unrest", "siteerr"])
def test_explicit_pair_wavefront_kernels_at_their_staging_limits(mode):
    """The explicit-pair wavefront kernels on lists of exactly one entry less than, as many as and one entry more than they stage:
    255 / 256 / 257 entries per list for k_merge_wave, k_wave_append and k_blen_wave (WaveUpdLdsStd::wuIn, WaveLdsStd::capW: the
    sizes of k_update_items_wave's inputs too), 511 / 512 / 513 for k_differ_wave and k_shorten_wave (WaveUpdLdsStd::cap).  All nine
    ordered size pairs, by wavefronts and by lanes (wave_per_item_max = -1): words and doubles bit for bit; the wavefront form
    against the oracle at the bars of test_hip_list_edges.py (appendProbNode 1e-12, the others 1e-9, structure exact); and the
    debug library's wavefront append on the same pairs.
    (What this can and cannot see: the oracle knows nothing of the kernels' routes, and a list beyond the limit is walked by
    lane 0 with the same result.  A limit that is off by one towards the one-lane walk therefore still passes; one that is off
    towards the staged walk overruns the staging and does not.)"""
    import list_edges as le
    from golden_util import close, lists_match
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref, kw = le.reference(), le.model(mode)
    u = bool(kw.get("usingErrorRate"))
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20)
    dbg = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20, debug=True)
    orc = Oracle(ref, le.ROOT_FREQS)
    for x in (dev, dbg, orc):
        x.set_model(**kw)
    rng = np.random.default_rng(61 + len(mode))
    # sets 0, 1: unrelated lists; sets 2, 3: the first list of set 0 and a list six nucleotides away from it (a branch length
    # to estimate, few factors to multiply), each cut to the three sizes
    small = [[exact_list(rng, ref, u, n) for n in (255, 256, 257)] for _ in range(2)]
    small += [[split_runs(g, k) for k in (0, 1, 2)] for g in (small[0][0], change_nucs(rng, small[0][0], 6))]
    base = exact_list(rng, ref, u, 511)
    big = [[split_runs(g, k) for k in (0, 1, 2)] for g in (base, change_nucs(rng, base, 1))]
    ids_s, ids_b = [dev.upload(x) for x in small], [dev.upload(x) for x in big]
    for ids, want in ((ids_s, [255, 256, 257]), (ids_b, [511, 512, 513])):
        for row in ids:
            assert dev.sizes(row)[0].tolist() == want
    ij = [(i, j) for i in range(3) for j in range(3)]
    # the 256 class: (list of set a, list of set a ^ 1), the child's as a tip's and as an internal node's
    pairs = [(a, i, a ^ 1, j, t) for a in range(4) for i, j in ij for t in (False, True)]
    P = np.asarray([ids_s[a][i] for a, i, b, j, t in pairs])
    Cl = np.asarray([ids_s[b][j] for a, i, b, j, t in pairs])
    lP, lC = [small[a][i] for a, i, b, j, t in pairs], [small[b][j] for a, i, b, j, t in pairs]
    tip = np.asarray([t for *_, t in pairs])
    bl = np.asarray([[1e-5, 1e-3, 0.0][k % 3] for k in range(len(pairs))])
    b2 = np.asarray([[2e-4, 1e-5][k % 2] for k in range(len(pairs))])
    ud = np.asarray([k % 4 == 1 for k in range(len(pairs))])
    # the 512 class: the same list cut differently (not different), and against the list with another last nucleotide
    dpairs = [(0, i, b, j) for b in (0, 1) for i, j in ij] + [(1, i, 0, j) for i, j in ij]
    D1, D2 = np.asarray([ids_b[a][i] for a, i, b, j in dpairs]), np.asarray([ids_b[b][j] for a, i, b, j in dpairs])
    S = np.concatenate(ids_b)
    assert len(pairs) * 3 + len(dpairs) + len(S) < 1024

    def run():
        mg = dev.merge_batch(P, bl + 1e-5, False, Cl, b2, tip, ud)
        sh = dev.shorten_batch(S)
        return dict(app=dev.append_batch(P, Cl, tip, bl), blen=dev.blen_batch(P, Cl, tip), dif=dev.differ_batch(D1, D2), mg=mg, sh=sh,
                    mg_pk=dev.download_packed(mg[mg >= 0]), sh_pk=dev.download_packed(sh))

    wave = run()
    dev.set_tuning(wave_per_item_max=-1)
    lane = run()
    dev.set_tuning()
    dwave, _ = dbg.debug_wave_append_batch(dbg.upload(lP), dbg.upload(lC), tip, bl)
    got_mg = dev.download(wave["mg"])
    got_sh = dev.download(wave["sh"])
    dev.close()
    dbg.close()
    # wavefronts against lanes: bit for bit
    assert np.array_equal(wave["app"].view(np.uint64), lane["app"].view(np.uint64))
    assert np.array_equal(wave["app"].view(np.uint64), dwave.view(np.uint64))
    assert np.array_equal(wave["blen"][0].view(np.uint64), lane["blen"][0].view(np.uint64)) and np.array_equal(wave["blen"][1], lane["blen"][1])
    assert np.array_equal(wave["dif"], lane["dif"])
    assert np.array_equal(wave["mg"] >= 0, lane["mg"] >= 0) and (wave["mg"] >= 0).sum() > len(pairs) // 2
    for k in ("mg_pk", "sh_pk"):
        for a in ("ent_off", "pos", "meta", "aux_off"):
            assert np.array_equal(getattr(wave[k], a), getattr(lane[k], a)), (k, a)
        assert np.array_equal(wave[k].aux.view(np.uint64), lane[k].aux.view(np.uint64)), k
    # wavefronts against the oracle
    for k, (a, i, b, j, t) in enumerate(pairs):
        want = orc.appendProbNode(lP[k], lC[k], bool(t), float(bl[k]))
        g = float(wave["app"][k])
        assert (g == want) if (math.isinf(want) or math.isinf(g)) else close(g, want, 1e-12), ("append", k, g, want)
        want = orc.estimateBranchLengthWithDerivative(lP[k], lC[k], bool(t))
        if want is False:
            assert wave["blen"][1][k], ("blen", k)
        else:
            assert not wave["blen"][1][k] and close(float(wave["blen"][0][k]), want, 1e-9), ("blen", k, wave["blen"][0][k], want)
        want = orc.mergeVectors(lP[k], float(bl[k]) + 1e-5, False, lC[k], float(b2[k]), bool(t), isUpDown=bool(ud[k]))
        assert lists_match(got_mg[k], want, 1e-9), ("merge", k)
    big_flat = [g for row in big for g in row]
    for k, (a, i, b, j) in enumerate(dpairs):
        assert bool(wave["dif"][k]) == bool(orc.areVectorsDifferent(big[a][i], big[b][j])) == (a != b), ("differ", k)
    n_shorter = 0
    for k, g in enumerate(big_flat):
        want = orc.shorten(g)
        assert lists_match(got_sh[k], want, 1e-9), ("shorten", k)
        n_shorter += len(want) < len(g)
    assert n_shorter >= 4                                                 # (at least the runs cut in two are joined again)


def test_wavefront_wide_update_items_leave_the_one_lane_lists(world, monkeypatch):
    """k_update_items_wave (one wavefront per item: mergeVectors, shorten and areVectorsDifferent cut along the merge path,
    wave_update.h) against k_update_items (one lane per item), in every model mode: the same 60 changes -- one at a time,
    the single-change chains the wavefront-wide kernel is for, then 40 at once -- repaired by both; every list either
    leaves must be the other's entry for entry, bit for bit."""
    from maple_amd.tree_host import HostTree, update_genome_lists
    _, data, dev, orc, mirror = world
    rng = np.random.default_rng(29)
    cand = np.nonzero((mirror.parent >= 0) & (mirror.dist > 1e-5))[0]
    pick = rng.choice(cand, size=60, replace=False)
    scale = rng.choice([0.3, 2.5, 40.0], size=60)

    def run():
        tree = HostTree.from_mirror(mirror)
        n = 0
        for v, f in zip(pick[:20], scale[:20]):
            tree.dist[v] = tree.dist[v] * f
            n += update_genome_lists(dev, tree, [int(v)])
        for v, f in zip(pick[20:], scale[20:]):
            tree.dist[v] = tree.dist[v] * f
        n += update_genome_lists(dev, tree, pick[20:].tolist())
        return tree, n

    mark = dev.mark()
    wave, n_wave = run()
    dev.set_tuning(wave_per_item_max=-1)
    lane, n_lane = run()
    dev.set_tuning()
    assert n_wave == n_lane and n_wave > 150
    assert np.array_equal(wave.dist, lane.dist)
    n_cmp = 0
    for attr in ("id_lower", "id_upRight", "id_upLeft", "id_totUp"):
        a, b = getattr(wave, attr), getattr(lane, attr)
        assert np.array_equal(a >= 0, b >= 0), attr
        moved = np.nonzero((a >= 0) & (a != getattr(HostTree.from_mirror(mirror), attr)))[0]
        if len(moved):
            assert dev.download(a[moved]) == dev.download(b[moved]), attr
            n_cmp += len(moved)
    assert n_cmp > 150
    dev.release(mark)


def test_wavefront_wide_kernels_around_their_list_length_limit(monkeypatch):
    """The wavefront-wide walks stage lists of up to 256 entries; longer ones go through the one-lane code on lane 0 of the
    same launch.  A 400-tip tree of divergent samples (~80 differences each: lists on both sides of the limit) takes both routes in the same launches: updatePartials and evaluatePlacement must still be the one-lane
    kernels', bit for bit."""
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_host import HostTree, update_genome_lists
    from maple_amd.tree_mirror import TreeMirror
    data = make_dataset(n_samples=400, l_ref=29903, seed=9, mean_diffs=80.0, frac_with_n=0.1, frac_ambig=0.05)
    ref_idx, rf = reference_tables(data.ref)
    dev = Device(ref_idx, rf, arena_bytes=1 << 30)
    dev.set_model(Q=Q)
    tips = {int(v): tip_genome_list(dl, ref_idx) for v, dl in zip(data.tip_node, data.diffs)}
    mirror = TreeMirror(dev, data.parent, data.blen, tips).build()
    n_ent = dev.sizes(mirror.tot_up[mirror.tot_up >= 0])[0]
    assert (n_ent > 256).sum() > 20 and (n_ent <= 200).sum() > 20, (n_ent.min(), int(np.median(n_ent)), n_ent.max())
    rng = np.random.default_rng(37)
    cand = np.nonzero((mirror.parent >= 0) & (mirror.dist > 1e-5))[0]
    pick = rng.choice(cand, size=40, replace=False)

    def run():
        tree = HostTree.from_mirror(mirror)
        n = 0
        for v in pick:
            tree.dist[v] = tree.dist[v] * 2.5
            n += update_genome_lists(dev, tree, [int(v)])
        return tree, n

    wave, n_wave = run()
    dev.set_tuning(wave_per_item_max=-1)
    lane, n_lane = run()
    dev.set_tuning()
    assert n_wave == n_lane and n_wave > 100
    base = HostTree.from_mirror(mirror)
    for attr in ("id_lower", "id_upRight", "id_upLeft", "id_totUp"):
        a, b = getattr(wave, attr), getattr(lane, attr)
        assert np.array_equal(a >= 0, b >= 0), attr
        moved = np.nonzero((a >= 0) & (a != getattr(base, attr)))[0]
        if len(moved):
            assert dev.download(a[moved]) == dev.download(b[moved]), attr
    nodes = np.nonzero(mirror.parent >= 0)[0]
    par = mirror.parent[nodes]
    up_ids = np.where(mirror.children[par, 0] == nodes, mirror.up_right[par], mirror.up_left[par]).astype(np.int32)
    ok = (mirror.tot_up[nodes] >= 0) & (up_ids >= 0)
    nodes, up_ids = nodes[ok], up_ids[ok]
    q_ids = mirror.lower[rng.choice(np.asarray(data.tip_node), size=len(nodes))].astype(np.int32)
    args = (mirror.tot_up[nodes], mirror.lower[nodes], up_ids, mirror.dist[nodes], q_ids, True, mirror.is_tip[nodes])
    wave4 = dev.evaluate_placement_batch(*args)
    dev.set_tuning(wave_per_item_max=-1)
    lane4 = dev.evaluate_placement_batch(*args)
    dev.set_tuning()
    assert len(wave4) > 500 and np.array_equal(wave4.view(np.uint64), lane4.view(np.uint64))
    # shorten() of single lists (k_shorten_wave for small batches): merged-but-unshortened lists are what it is for
    half = mirror.dist[nodes][:500] / 2
    merged = dev.merge_batch(up_ids[:500], half, False, mirror.lower[nodes][:500], half, mirror.is_tip[nodes][:500], True)
    merged = merged[merged >= 0]
    assert len(merged) > 300
    sw = dev.shorten_batch(merged)
    dev.set_tuning(wave_per_item_max=-1)
    sl = dev.shorten_batch(merged)
    dev.set_tuning()
    assert dev.download(sw) == dev.download(sl)
    assert (dev.sizes(sw)[0] < dev.sizes(merged)[0]).sum() > 50           # (it did shorten something)
    dev.close()


def test_serial_placement_through_tree_patch_on_a_tree_with_local_references(world):
    """The serial placement phase on a tree with MAT local references, in every model mode: 20 samples one after the other
    (single-query search, a new internal node + tip at the best branch, maple_update_partials, HostTree.sync =
    maple_tree_patch) must give, sample for sample, the same search results as the same sequence with a full
    maple_tree_upload after every sample -- the patched copy of the tree, its reference frames and its candidate / leaf
    columns are the rebuilt ones.  (The tree edit is a stand-in for placeSampleOnTree; the reference's own edits are
    replayed by test_online_sample_additions_through_tree_patch on trees without local references.)"""
    from maple_amd.host import tip_genome_list
    from maple_amd.mat import add_local_references
    from maple_amd.synth import perturb_diffs
    from maple_amd.tree_host import HostTree, update_genome_lists
    mode, data, dev, orc, mirror = world
    l_ref = dev.lRef
    ll = math.log(l_ref)
    pkw = dict(oneMutBLen=1.0 / l_ref, effectivelyNon0BLen=1.0 / (10 * l_ref), thresholdLogLK=18.0 * ll,
               thresholdLogLKoptimization=ll, thresholdLogLKconsecutivePlacement=1.0)
    prng = np.random.default_rng(23)
    from maple_amd.host import reference_tables
    ref_idx, _ = reference_tables(data.ref)
    new = [tip_genome_list(perturb_diffs(data.diffs[i], data.ref, prng), ref_idx) for i in range(20)]

    def run(patching):
        mark = dev.mark()
        tree = HostTree.from_mirror(mirror)
        assert add_local_references(dev, tree, 30) > 10
        tree.upload_topology(dev)
        results, patched = [], []
        for lst in new:
            patched.append(tree.sync(dev) if patching else (tree.upload_topology(dev), -1)[1])
            dev.placement_prepare(**pkw)
            qid = dev.upload([lst])
            out = dev.placement_search_batch(qid, **pkw)
            assert out["status"][0] >= 0
            results.append((int(out["status"][0]), int(out["bestNode"][0]), float(out["bestScore"][0]), tuple(out["blen"][0].tolist())))
            b = int(out["bestNode"][0])
            if out["status"][0] != 0 or tree.up[b] is None:
                continue
            top, bottom, app = (float(x) for x in out["blen"][0])
            n = tree.n
            g, p, s = tree.up[b], n, n + 1
            up = list(tree.up) + [g, p]
            children = [list(c) for c in tree.children] + [[b, s], []]
            children[g] = [p if c == b else c for c in children[g]]
            up[b] = p
            dist = list(tree.dist) + [top, app]
            dist[b] = bottom
            changed = tree.apply_topology(tree.root, up, children, dist, list(tree.n_minor) + [0, 0])
            tree.id_lower[s] = int(out["bestDiffs"][0])                  # the sample in the frame of its new place
            update_genome_lists(dev, tree, changed)
        dev.release(mark)
        return results, patched
    a, patched = run(True)
    b, _ = run(False)
    assert patched[0] == 0 and all(0 <= p < 64 for p in patched), patched
    assert len(a) == len(b) == 20
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[:2] == y[:2] and rel(x[2], y[2]) < 1e-12 and all(rel(u, v) < 1e-12 for u, v in zip(x[3], y[3])), (k, x, y)
    assert sum(r[0] == 0 for r in a) >= 10


def test_wavefront_wide_append_on_tree_lists(world):
    """wave_append on the lists of a real tree (probVectTotUp of 4 000 branches against tip lists, every model mode; lists
    near the root are longer than what the cooperative walk stages and take its one-lane fall-back): identical to
    maple_append_batch in every bit."""
    mode, data, dev, orc, mirror = world
    rng = np.random.default_rng(41)
    cand = np.nonzero(mirror.tot_up >= 0)[0]
    tips = np.nonzero(mirror.is_tip.astype(bool))[0]
    pl = mirror.tot_up[rng.choice(cand, size=4000)]
    cl = mirror.lower[rng.choice(tips, size=4000)]
    bl = np.where(rng.random(4000) < 0.2, 0.0, 1.0 / dev.lRef)          # some zero-length attachments: -inf results
    one = dev.append_batch(pl, cl, True, bl)
    # (the wavefront-wide kernel's entry point is a hook of libmaple_hip_debug.so: the same lists on a device of that library)
    from maple_amd.host import reference_tables
    from maple_amd.runtime import Device
    ref_idx, rf = reference_tables(data.ref)
    dbg = Device(ref_idx, rf, arena_bytes=1 << 30, debug=True)
    dbg.set_model(**world_model_kwargs(mode, len(ref_idx)))
    pl_d, cl_d = dbg.upload_packed(dev.download_packed(pl)), dbg.upload_packed(dev.download_packed(cl))
    assert np.array_equal(dbg.append_batch(pl_d, cl_d, True, bl), one)
    wave, ms = dbg.debug_wave_append_batch(pl_d, cl_d, True, bl)
    dbg.close()
    assert np.array_equal(one, wave), int((one != wave).sum())
    assert np.isfinite(one).any() and (mode == "siteerr" or np.isinf(one).any())   # (with an error model a zero-length mismatch is finite)
    print(f"{mode}: 4000 wavefront-wide appendProbNode in {ms:.3f} ms")


def test_batch_kernel_with_queries_longer_than_the_lds_stage():
    """k_append_queries keeps the tile's query words in LDS up to 192 entries and reads longer lists from memory: both
    paths against the oracle (samples with ~150 and ~400 differences give lists on either side of the limit)."""
    import torch
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from oracle.oracle_py import Oracle
    data = make_dataset(n_samples=96, l_ref=29903, seed=12, mean_diffs=30.0, frac_with_n=0.2, frac_ambig=0.2)
    long_a = make_dataset(n_samples=4, l_ref=29903, seed=13, mean_diffs=150.0)
    long_b = make_dataset(n_samples=4, l_ref=29903, seed=14, mean_diffs=400.0)
    ref_idx, rf = reference_tables(data.ref)
    dev = Device(ref_idx, rf, arena_bytes=256 << 20)
    dev.set_model(Q)
    orc = Oracle(ref_idx, rf)
    orc.set_model(Q)
    cands = [tip_genome_list(dl, ref_idx) for dl in data.diffs]
    # the long samples were drawn against their own random references: re-use only their positions / bases on this one
    queries = []
    for ds in (long_a, long_b):
        for dl in ds.diffs:
            fixed = [(("acgt".replace(data.ref[e[1] - 1], ""))[e[1] % 3], e[1]) for e in dl if e[0] in "acgt"]
            queries.append(tip_genome_list(sorted(set(fixed), key=lambda e: e[1]), ref_idx))
    n_ent = [len(q) for q in queries]
    assert min(n_ent) < 192 < max(n_ent), n_ent
    c_ids = dev.upload(cands)
    q_ids = dev.upload(queries)
    cu = torch.device("cuda", 0)
    t_q = torch.from_numpy(q_ids.astype(np.int32)).to(cu)
    t_c = torch.from_numpy(c_ids.astype(np.int32)).to(cu)
    out = torch.empty(len(queries) * len(cands), dtype=torch.float64, device=cu)
    torch.cuda.synchronize()
    dev.append_queries_dev(len(queries), t_q.data_ptr(), len(cands), t_c.data_ptr(), True, 1.0 / dev.lRef, out.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(len(queries), len(cands))
    for qi, q in enumerate(queries):
        for ci in range(0, len(cands), 7):
            want = orc.appendProbNode(cands[ci], q, True, 1.0 / dev.lRef)
            g = float(got[qi, ci])
            assert (math.isinf(want) and math.isinf(g)) or rel(g, want) < 1e-12, (qi, ci, g, want)
    dev.close()


def test_root_frame_candidate_copies_do_not_pile_up_in_the_arena():
    """A tree with local references: the whole-tree searches' rows are made in the ROOT's frame, from copies of every candidate list
    re-expressed there once per tree (ensure_cand_root, spr_batch.hip).  maple_tree_patch / maple_tree_upload drop the copies'
    validity; the next search makes new ones.  The stale ones must go when they are still the arena's last lists -- a loop of
    rounds and patches used to gain n_scored lists per turn -- and the rounds' results must not change."""
    import bench
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree
    data, dev, orc, m = build(3000, "unrest", seed=6)
    ht = HostTree.from_mirror(m)
    assert add_local_references(dev, ht, 50) > 20
    dist = np.asarray([float(x or 0.0) for x in ht.dist])
    cols = (m.parent, m.children[:, 0], m.children[:, 1], dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft, ht.id_totUp)
    dev.upload_tree(ht.root, *cols, ht.id_mut)
    kw = bench.search_kwargs(dev.lRef)
    nodes = bench.preorder_nodes(m)
    first, counts, mut_ids = None, [], []
    before = dev.stats()["n_lists"]
    touched = np.asarray(nodes[:8], dtype=np.int32)
    for turn in range(4):
        g = dev.spr_search_batch(nodes, **kw)
        if first is None:
            first = g
        for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
            assert np.array_equal(g[k], first[k]), (turn, k)
        counts.append(dev.stats()["n_lists"])
        # a MAT mutation list uploaded between the rounds (as a caller does for a new reference branch) must survive the release of
        # the stale copies: an arena mark also carries the count of mutation lists, ensure_cand_root must not release through it
        mut_ids.append(int(dev.upload_mutations([[(10 + turn, 0, 1), (500 + turn, 2, 3)]])[0]))
        # the same records again: nothing changes but the library's tables are stale
        dev.tree_patch(m.n_nodes, touched, *[np.asarray(c)[touched] for c in cols])
    # every mutation list uploaded on the way is still there and still its own (pass a list through each: position 10+turn A->C)
    lst = dev.upload([[(4, dev.lRef)]])
    for turn, mid in enumerate(mut_ids):
        assert mid == mut_ids[0] + turn, mut_ids
        out = dev.download(dev.pass_branch_batch(lst, [mid], False))[0]
        # R up to the first mutated site, the site as an explicit nucleotide, R up to the second, the site, R to the end
        assert [e[0] for e in out] == [4, 0, 4, 2, 4] and [e[1] for e in out[::2]] == [9 + turn, 499 + turn, dev.lRef], (turn, out)
    assert (first["status"] == 0).sum() > 1000
    assert counts[0] - before > 1000, (before, counts)               # (the copies were made: one per scored branch)
    assert counts[0] == counts[1] == counts[2] == counts[3], counts  # (... and replaced, not added to, after every patch)
    dev.close()


def test_bench_two_ranks_plumbing():
    """`bench.py --gpus 2` as the driver launches it (torch.distributed.run, one process per rank) on a box with ONE GPU:
    MAPLE_BENCH_BACKEND=gloo lets both ranks share it and sends the collectives through host memory.  Checks the N > 1
    path end to end: pre-order sharding of each step's batch, the all-gather of proposed moves, the max-over-ranks
    timing and the sum of the ranks' candidate placements."""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    common = ["--samples", "1500", "--model", "unrest", "--batch", "600", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
              "--no-extras"]
    env = dict(os.environ, MAPLE_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert two.returncode == 0, two.stderr[-2000:]
    line2 = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1])
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True,
                         timeout=900, env=env, cwd=root)
    assert one.returncode == 0, one.stderr[-2000:]
    line1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert line2["n_gpus"] == 2 and line1["n_gpus"] == 1 and line2["scaling"] == "strong"
    # the same searches, whoever ran them: the same total of candidate placements
    assert line2["config"]["searches_timed"] == line1["config"]["searches_timed"] == 2 * 600
    assert line2["config"]["candidate_placements_timed"] == line1["config"]["candidate_placements_timed"]
    assert line2["value"] > 0 and line2["roofline"]["frac"] >= 0


def test_bench_two_ranks_rccl():
    """The same two-rank run over RCCL (backend "nccl"), one GPU per rank -- only where two GPUs are visible (the boxes of this
    project's rounds have one: skipped there; the gloo form above is what runs).  Proposal records then stay in device memory
    through the all-gather (maple_amd.parallel.gather_proposals with a cuda device)."""
    import json
    import os
    import socket
    import subprocess
    import sys
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one GPU visible: the RCCL form of the two-rank run needs two")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    common = ["--samples", "1500", "--model", "unrest", "--batch", "600", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
              "--no-extras"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("MAPLE_BENCH_BACKEND", None)
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
                          "127.0.0.1", "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert two.returncode == 0, two.stderr[-2000:]
    line2 = json.loads([ln for ln in two.stdout.splitlines() if ln.startswith("{")][-1])
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + common, capture_output=True, text=True,
                         timeout=900, env=env, cwd=root)
    assert one.returncode == 0, one.stderr[-2000:]
    line1 = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    assert line2["n_gpus"] == 2 and line2["config"]["searches_timed"] == line1["config"]["searches_timed"]
    assert line2["config"]["candidate_placements_timed"] == line1["config"]["candidate_placements_timed"]


def test_bench_plain_run_dumps_its_outputs(tmp_path):
    """A plain `bench.py` run (no --full) on a small tree: the line has the contract's fields and nothing of what --full adds,
    --steps timed steps, and --dump-outputs writes the last timed step's arrays in float64 -- the same files from run to run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--gpus", "1", "--samples", "1500", "--model", "unrest", "--batch", "600", "--steps", "3", "--warmup", "1"]
    lines = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + common + ["--dump-outputs", str(tmp_path / run)],
                           capture_output=True, text=True, timeout=600, cwd=root)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    line = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["config"]["searches_timed"] == 3 * 600
    assert "cpu_baseline" not in line and "tree_log_lk" not in line and line["first_step_after_upload_ms"] is None
    files = sorted(os.listdir(tmp_path / "a"))
    assert "placement.npy" in files and "moves.npy" in files and files == sorted(os.listdir(tmp_path / "b"))
    nodes = np.load(tmp_path / "a" / "nodes.npy")
    assert nodes.dtype == np.float64 and len(nodes) == 600
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b, equal_nan=True), f


def test_apply_phase_batched_equals_sequential(world):
    """applySPRMovesParallel (M:9470-9484) in its two drivers (maple_amd/spr_apply.py): the proposed moves of a deep round on a
    tree with misplaced tips, re-searched one at a time on the current tree and applied -- against the same moves re-searched
    32 at a time, a speculative result kept only while nothing its search may have read was touched.  Same applied sequence,
    same topology, same branch lengths, and every genome list the same entry for entry."""
    import bench
    from maple_amd.spr_apply import SprApplier
    mode, data, dev, orc, mirror = world
    kw = bench.search_kwargs(dev.lRef)
    m = mirror
    # misplace 60 tips: swap the lower lists of pairs of tips far apart in the tree, then rebuild the lists
    from maple_amd.tree_mirror import TreeMirror
    rng = np.random.default_rng(17)
    tips = np.asarray(data.tip_node)
    pick = rng.choice(tips, size=120, replace=False)
    mark = dev.mark()
    tip_lists = {int(v): dev.download([m.lower[v]])[0] for v in tips}
    for a, b in zip(pick[:60], pick[60:]):
        tip_lists[int(a)], tip_lists[int(b)] = tip_lists[int(b)], tip_lists[int(a)]
    m2 = TreeMirror(dev, m.parent, m.dist.copy(), tip_lists).build()
    no_mut = -np.ones(m2.n_nodes, dtype=np.int32)
    dev.upload_tree(m2.root, m2.parent, m2.children[:, 0], m2.children[:, 1], m2.dist, m2.is_tip, m2.lower, m2.up_right, m2.up_left,
                    m2.tot_up, no_mut)
    order = bench.preorder_nodes(m2)
    r = dev.spr_search_batch(order, **kw)
    prop = np.nonzero(r["placement"] >= 0)[0]
    prop = prop[np.argsort(-r["improvement"][prop], kind="stable")]
    moves = order[prop][:80]
    assert len(moves) >= 40
    seq = SprApplier.from_mirror(dev, m2).apply_sequential(moves, kw)
    bat = SprApplier.from_mirror(dev, m2).apply_batched(moves, kw, batch=32)
    assert len(seq.applied) >= 20
    assert seq.applied == bat.applied
    # (searches from misplaced tips expand wide regions, so speculative results are often dropped here; on the bench tree the
    # searches are local and a batch of 32 is mostly kept -- bench.py's apply_phase block)
    assert len(bat.times["search"]) < len(seq.times["search"]) and max(k for _, k in bat.batches) >= 2
    for a in ("up", "c0", "c1", "dist"):
        assert np.array_equal(getattr(seq, a), getattr(bat, a)), a
    for a in ("lower", "up_right", "up_left", "tot_up"):
        ia, ib = getattr(seq, a), getattr(bat, a)
        assert np.array_equal(ia >= 0, ib >= 0), a
        have = np.nonzero(ia >= 0)[0]
        assert dev.download(ia[have]) == dev.download(ib[have]), a
    dev.release(mark)


def test_deep_round_with_error_model_at_20k_tips_frontier_tier_equals_lane_tier():
    """A deep SPR round with the error model on a 20 000-tip tree: a fifth of the searches is long, the frontier tier's pools run
    over on the first call (searches handed back, the level ranges end at the pools' capacity) and the long searches leave at
    the lane tiers' budget.  Status, node ids, candidate counts, scores and branch lengths equal those of the
    one-lane-per-search kernels, bit for bit -- on the first call and on the next one, whose pools are sized by what the
    first asked for."""
    import bench
    data, dev, orc, m = build(20000, "siteerr", seed=1)
    dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left,
                    m.tot_up, -np.ones(m.n_nodes, dtype=np.int32))
    kw = bench.search_kwargs(dev.lRef)
    nodes = bench.preorder_nodes(m)
    lane = dev.spr_search_batch(nodes, search_tier=1, **kw)
    # (wide_search_budget = 20 000 items per search: more than the pools of a first call hold -- they run over, then grow)
    for budget in (20000, 20000, 0, 0):
        g = dev.spr_search_batch(nodes, wide_search_budget=budget, **kw)
        for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
            assert np.array_equal(g[k], lane[k]), (budget, k)
    assert (g["status"] == 0).sum() > 30000 and g["nAppend"].sum() > 1e7
    # (from the second call on, the nodes whose search ran over the budget went to the dense tier at once -- the library remembers
    # them per tree: maple_tuning.noOverHint switches that off; a hint left by ANOTHER budget is only a hint)
    dev.set_tuning(no_over_hint=True)
    g = dev.spr_search_batch(nodes, **kw)
    dev.set_tuning()
    for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
        assert np.array_equal(g[k], lane[k]), ("no hints", k)
    g = dev.spr_search_batch(nodes[::3], wide_search_budget=300, **kw)
    for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
        assert np.array_equal(g[k], lane[k][::3]), ("hints of another budget", k)
    dev.close()


@pytest.mark.parametrize("mode", ["unrest", "ratevar", "siteerr"])
def test_frontier_tier_on_a_tree_with_local_references_equals_the_lane_tier(mode):
    """Trees as MAPLE makes them carry MAT local references (makeNodeReference, M:8296-8354; here setUpMAT's rule, 50 descendants per
    reference node): a search re-expresses the lists it carries at every reference branch it crosses (M:6844-6847, 7111-7118,
    7148-7155, 7359-7366, 7388-7395).  The frontier tier (items carry the removed list of their frame; a list that leaves a frame goes
    through passGenomeListThroughBranch) against the one-lane-per-search kernels on a 10 000-tip tree, every search of a deep
    round: status, node ids, moves, candidate counts, scores and branch lengths bit for bit -- with and without the hand-over of
    long searches to the dense tier."""
    import bench
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree
    data, dev, orc, m = build(10000, mode, seed=4)
    ht = HostTree.from_mirror(m)
    n_ref = add_local_references(dev, ht, 50)
    assert n_ref > 100
    dist = np.asarray([float(x or 0.0) for x in ht.dist])
    dev.upload_tree(ht.root, m.parent, m.children[:, 0], m.children[:, 1], dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft,
                    ht.id_totUp, ht.id_mut)
    kw = bench.search_kwargs(dev.lRef)
    nodes = bench.preorder_nodes(m)
    for budget in (-1, 0):
        lane = dev.spr_search_batch(nodes, search_tier=1, wide_search_budget=budget, **kw)
        for _ in range(2):                                              # (the second call: pools sized by the first)
            g = dev.spr_search_batch(nodes, wide_search_budget=budget, **kw)
            for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
                assert np.array_equal(g[k], lane[k]), (budget, k, int((g[k] != lane[k]).sum()))
    assert (g["status"] == 0).sum() > 15000 and g["nAppend"].sum() > 1e7
    if mode == "unrest":
        # bestRemovedPartials (M:7720: the removed list in the best branch's frame, as the reference's in-place shorten() left it):
        # the two tiers hand back the same list, entry for entry -- also where a list was shortened on the way and re-expressed
        # from its shortened form afterwards (k_fr_replay hands such a search to the one-lane kernel: the event item's own
        # children included since round 6)
        mark = dev.mark()
        a = dev.spr_search_batch(nodes, want_removed_partials=True, **kw)
        la = dev.download(a["removedPartials"][a["removedPartials"] >= 0])
        have_a = a["removedPartials"] >= 0
        dev.release(mark)
        b = dev.spr_search_batch(nodes, search_tier=1, want_removed_partials=True, **kw)
        assert np.array_equal(have_a, b["removedPartials"] >= 0) and have_a.sum() > 1000
        lb = dev.download(b["removedPartials"][b["removedPartials"] >= 0])
        assert la == lb
        dev.release(mark)
    dev.close()


@pytest.mark.parametrize("mode", ["ratevar", "siteerr"])
def test_frontier_levels_by_wavefronts_or_by_lanes_give_the_same_searches(mode):
    """maple_tuning.waveAllBelow only chooses HOW a level of the frontier tier is walked -- a wavefront per item that still updates
    genome lists (wave_update.h: the walks cut along their merge paths) or a lane per item: never, for the small levels only (the
    default), for every level.  Same searches bit for bit, on a plain tree and on the same tree with MAT local references."""
    import bench
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree
    data, dev, orc, m = build(3000, mode, seed=8)
    kw = bench.search_kwargs(dev.lRef)
    nodes = bench.preorder_nodes(m)
    no_mut = -np.ones(m.n_nodes, dtype=np.int32)
    ht = HostTree.from_mirror(m)
    for form in ("plain", "local references"):
        if form == "plain":
            dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left, m.tot_up, no_mut)
        else:
            assert add_local_references(dev, ht, 40) > 20
            dist = np.asarray([float(x or 0.0) for x in ht.dist])
            dev.upload_tree(ht.root, m.parent, m.children[:, 0], m.children[:, 1], dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft,
                            ht.id_totUp, ht.id_mut)
        res = []
        for wab in (-1, 0, 1 << 30):
            dev.set_tuning(wave_all_below=wab)
            res.append(dev.spr_search_batch(nodes, wide_search_budget=-1, **kw))
        dev.set_tuning()
        for r in res[1:]:
            for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
                assert np.array_equal(r[k], res[0][k]), (form, k)
        assert (res[0]["status"] == 0).sum() > 4000
    dev.close()


@pytest.mark.parametrize("mode", ["ratevar", "siteerr"])
def test_frontier_wavefront_size_classes_are_both_used_and_equal_the_lane_forms(mode):
    """The wavefront-wide items of a frontier level come in two size classes (frt::WaveSmall / frt::WaveBig, frontier_dev.h:
    k_fr_sort_level lists an item for the class whose staging its lists fit, k_fr_updating_wave_s / k_fr_updating_wave take
    them).  A 400-tip tree of divergent samples (60 differences on average: tip lists of 17 to 257 entries, most of them at
    most 128) with every level by wavefronts: BOTH classes get items, and the searches are those of a lane per item and of the
    one-lane-per-search kernels, bit for bit, on the plain tree and with MAT local references."""
    import bench
    from maple_amd.host import reference_tables, tip_genome_list
    from maple_amd.mat import add_local_references
    from maple_amd.runtime import Device
    from maple_amd.synth import make_dataset
    from maple_amd.tree_host import HostTree
    from maple_amd.tree_mirror import TreeMirror
    data = make_dataset(n_samples=400, l_ref=29903, seed=9, mean_diffs=60.0, frac_with_n=0.1, frac_ambig=0.05)
    ref_idx, rf = reference_tables(data.ref)
    mkw = world_model_kwargs(mode, len(ref_idx), 9)
    dev = Device(ref_idx, rf, arena_bytes=1 << 30, debug=True)
    dev.set_model(**mkw)
    tip_kw = dict(error_rates=mkw["errorRates"]) if mode == "siteerr" else {}
    tips = {int(v): tip_genome_list(dl, ref_idx, **tip_kw) for v, dl in zip(data.tip_node, data.diffs)}
    m = TreeMirror(dev, data.parent, data.blen, tips).build()
    kw = bench.search_kwargs(dev.lRef)
    nodes = bench.preorder_nodes(m)
    ht = HostTree.from_mirror(m)
    for form in ("plain", "local references"):
        if form == "plain":
            dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left, m.tot_up,
                            -np.ones(m.n_nodes, dtype=np.int32))
        else:
            assert add_local_references(dev, ht, 40) > 0
            dist = np.asarray([float(x or 0.0) for x in ht.dist])
            dev.upload_tree(ht.root, m.parent, m.children[:, 0], m.children[:, 1], dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft,
                            ht.id_totUp, ht.id_mut)
        res = []
        for wab in (-1, 1 << 30):
            dev.set_tuning(wave_all_below=wab)
            res.append(dev.spr_search_batch(nodes, wide_search_budget=-1, **kw))
        if form == "plain":
            dev.frontier_levels()
            n_small, n_big = (int(x.sum()) for x in dev.last_wave_items)
            print(f"wavefront-wide items, {mode}: {n_small} small class, {n_big} big class")
            assert n_small > 0 and n_big > 0, (n_small, n_big)
        dev.set_tuning()
        res.append(dev.spr_search_batch(nodes, search_tier=1, wide_search_budget=-1, **kw))
        for r in res[1:]:
            for k in ("status", "bestNode", "placement", "nAppend", "bestScore", "currentLK", "improvement", "blen"):
                assert np.array_equal(r[k], res[0][k]), (form, k)
        assert (res[0]["status"] == 0).any()
    dev.close()


def test_local_references_batched_equals_one_by_one():
    """maple_amd.mat.add_local_references (every step batched: what the 1 000 000-tip bench tree needs) against its first
    form, one reference node at a time: the same reference nodes, the same mutation lists, the same four genome lists of
    every node, entry for entry."""
    from maple_amd.mat import add_local_references, add_local_references_one_by_one
    from maple_amd.tree_host import HostTree
    data, dev, orc, m = build(3000, "ratevar", seed=11)
    trees = []
    for fn in (add_local_references_one_by_one, add_local_references):
        ht = HostTree.from_mirror(m)
        n_ref = fn(dev, ht, 40)
        trees.append((n_ref, ht))
    (n1, a), (n2, b) = trees
    assert n1 == n2 and n1 > 20
    assert a.mutations == b.mutations
    assert np.array_equal(np.asarray(a.id_mut) >= 0, np.asarray(b.id_mut) >= 0)
    for col in ("id_lower", "id_upRight", "id_upLeft", "id_totUp"):
        ia, ib = np.asarray(getattr(a, col)), np.asarray(getattr(b, col))
        assert np.array_equal(ia >= 0, ib >= 0), col
        have = np.nonzero(ia >= 0)[0]
        assert dev.download(ia[have]) == dev.download(ib[have]), col
    dev.close()


def test_oracle_tree_log_lk_from_the_tips_equals_the_library_on_plain_and_local_reference_trees(world):
    """bench.tree_log_lk_check, the bench line's `tree_log_lk`: calculateTreeLikelihood (M:9721-9779) by the library over the
    stored lower lists -- of the plain tree and of the same tree with MAT local references -- against the C oracle's value from
    the tips' lists alone (no list of the GPU's enters it)."""
    import bench
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree
    mode, data, dev, orc, mirror = world
    tips = np.nonzero(mirror.is_tip)[0]
    tip_ids = mirror.lower.copy()
    from maple_amd.host import reference_tables
    ref_idx, rf = reference_tables(data.ref)
    kw = world_model_kwargs(mode, len(ref_idx))
    plain = bench.tree_log_lk_check(dev, mirror, None, tip_ids, kw, ref_idx, rf)
    assert plain["rel_delta"] <= 1e-12, plain
    mark = dev.mark()
    ht = HostTree.from_mirror(mirror)
    assert add_local_references(dev, ht, 50) > 5
    mat = bench.tree_log_lk_check(dev, mirror, ht, tip_ids, kw, ref_idx, rf)
    # (the reference's whole-genome term, M:4487, uses the root's reference in every frame: the two forms of the tree differ in
    # about the fifth digit, each equal to the oracle's value for its own form)
    assert mat["rel_delta"] <= 1e-11 and 0 < abs(mat["oracle"] - plain["oracle"]) < 1e-3 * abs(plain["oracle"]), (mat, plain)
    dev.release(mark)
    assert len(tips) * 2 - 1 == mirror.n_nodes


@pytest.mark.parametrize("mode", ["ratevar", "siteerr"])
def test_serial_loop_with_rows_made_ahead_equals_the_plain_loop(mode):
    """maple_placement_ahead (include/maple_hip.h): the score rows of the next samples of the serial placement loop (M:11692-11752)
    made in ONE launch and kept current under maple_tree_patch.  The loop with the samples announced 64 at a time against the
    plain loop (one scoring launch per sample) on a 6 000-tip tree, 400 new samples -- among them copies of tips (minor sequences:
    skipped by the stand-in edit) and samples placed next to samples added before them: every search's status, node, score,
    branch lengths and candidate count bit for bit, the final trees identical (relatives, lengths), the lists of a sample of the
    final tree's nodes entry for entry; and the rows were really used (the library counts its refreshes)."""
    import bench
    from maple_amd.host import tip_genome_list
    from maple_amd.synth import perturb_diffs
    data, dev, orc, m = build(6000, mode, seed=9)
    l_ref = dev.lRef
    ll = math.log(l_ref)
    pkw = dict(oneMutBLen=1.0 / l_ref, effectivelyNon0BLen=1.0 / (10 * l_ref), thresholdLogLK=18.0 * ll,
               thresholdLogLKoptimization=1.0 * ll, thresholdLogLKconsecutivePlacement=1.0)
    kw = world_model_kwargs(mode, l_ref, 9)
    tip_kw = dict(error_rates=kw["errorRates"]) if mode == "siteerr" else {}
    prng = np.random.default_rng(3)
    src = prng.choice(len(data.diffs), size=400, replace=True)            # (with replacement: several samples next to one tip)
    new_lists = []
    for k, i in enumerate(src):
        dl = data.diffs[int(i)] if k % 25 == 0 else perturb_diffs(data.diffs[int(i)], data.ref, prng)
        new_lists.append(tip_genome_list(dl, dev.ref_idx, **tip_kw))
    runs, stats = [], []
    # plain loop; rows by expansion; every branch; expansion cut short; rows by expansion without the traversals made ahead
    for ahead, expansion, spec in ((0, 0, True), (64, 0, True), (64, 1, True), (64, 2, True), (64, 0, False)):
        mark = dev.mark()
        dev.set_tuning(no_ahead_expansion=expansion, no_ahead_speculation=not spec)
        before = dev.placement_ahead_stats()
        sp = bench.serial_phase(dev, m, new_lists, pkw, ahead=ahead)
        after = dev.placement_ahead_stats()
        stats.append({k: after[k] - before[k] for k in after})
        c = sp["cols"]
        n = c["n"]
        probe = np.arange(0, n, 97)
        lists = {name: dev.download(c[name][probe][c[name][probe] >= 0]) for name in ("lower", "tot_up", "up_right")}
        runs.append((sp, lists))
        dev.release(mark)
    dev.set_tuning()
    (a, la) = runs[0]
    assert a["placed"] > 300 and len(a["times"]["ahead"]) == 0 and stats[0]["searches"] == 0
    for (b, lb), st in zip(runs[1:], stats[1:]):
        assert a["placed"] == b["placed"]
        assert a["results"] == b["results"]
        ca, cb = a["cols"], b["cols"]
        assert ca["n"] == cb["n"]
        for name in ("up", "c0", "c1", "dist", "tip"):
            assert np.array_equal(ca[name][: ca["n"]], cb[name][: cb["n"]]), name
        for name in la:
            assert la[name] == lb[name], name
        assert len(b["times"]["ahead"]) >= 6 and st["searches"] == len(new_lists), st
    # rows by expansion: items were expanded, far fewer than samples x branches, and few rows had to be scored in full after all
    assert stats[1]["expanded_items"] > 0 and stats[2]["expanded_items"] == 0
    assert stats[1]["expanded_items"] < 0.5 * len(new_lists) * m.n_nodes
    assert stats[1]["fallbacks"] <= 0.2 * len(new_lists), stats[1]
    assert stats[2]["fallbacks"] == 0
    # ... and with the expansion cut short after six levels nearly every search has its row scored in full after all: same results
    assert stats[3]["fallbacks"] > 0.5 * len(new_lists), stats[3]
    # the traversal of the next sample made by a host thread during the placement before it: used where the placement touched
    # nothing it had visited, dropped (and made again) where it did -- and never made when switched off
    assert stats[1]["traversals_ahead_used"] > 0.3 * len(new_lists), stats[1]
    assert stats[1]["traversals_ahead_used"] + stats[1]["traversals_ahead_dropped"] <= len(new_lists)
    assert stats[4]["traversals_ahead_used"] == 0 and stats[4]["traversals_ahead_dropped"] == 0
    print("rows made ahead:", stats)
    dev.close()


# ---- the announced serial loop at its edges ------------------------------------------------------------------------------
# Each test below runs the serial placement loop (bench.serial_phase's stand-in tree edit) with its samples announced
# (maple_placement_ahead) and without, on the same inputs and with the same interleaved calls, and requires the same result of
# every search bit for bit; on a sample of the searches it also requires the C oracle's findBestParentForNewSample on the tree
# as it is then (an OracleTree downloaded once and brought up to date in place with the nodes touched since the last check).

def small_pkw(l_ref):
    ll = math.log(l_ref)
    return dict(oneMutBLen=1.0 / l_ref, effectivelyNon0BLen=1.0 / (10 * l_ref), thresholdLogLK=18.0 * ll,
                thresholdLogLKoptimization=1.0 * ll, thresholdLogLKconsecutivePlacement=1.0)


def serial_loop(dev, m, new_lists, pkw, ahead=0, hook=None, orc=None, oracle_every=0, stop=None):
    """The serial placement loop on TreeMirror ``m`` (the edit of bench.serial_phase) with a hook before every search:
    hook(k, st) may call the library between two searches and edit st["waiting"] (the announced samples not yet searched, in
    order) -- it is called in the plain loop too.  Announced loops take ``ahead`` samples at a time; their lists are uploaded
    before any per-search mark.  Returns the per-search results (status, node, score, lengths, nAppend), the steps at which the
    root's lower list got a new id, and the oracle checks (k, oracle's answer, result).  ``stop``: search only that many."""
    import bench
    n_add = len(new_lists)
    n0, cap = m.n_nodes, m.n_nodes + 2 * n_add

    def grown(a, fill, dtype):
        out = np.full(cap, fill, dtype=dtype)
        out[:n0] = a
        return out
    up = grown(m.parent, -1, np.int32)
    c0, c1 = grown(m.children[:, 0], -1, np.int32), grown(m.children[:, 1], -1, np.int32)
    tip = grown(m.is_tip, 0, np.uint8)
    dist = grown(m.dist, 0.0, np.float64)
    mut = np.full(cap, -1, dtype=np.int32)
    lower, up_right = grown(m.lower, -1, np.int32), grown(m.up_right, -1, np.int32)
    up_left, tot_up = grown(m.up_left, -1, np.int32), grown(m.tot_up, -1, np.int32)
    depth, dstep = bench.tree_depths(m.root, c0, c1, n0, cap)
    n = n0
    dev.upload_tree(m.root, up[:n], c0[:n], c1[:n], dist[:n], tip[:n], lower[:n], up_right[:n], up_left[:n], tot_up[:n], mut[:n])
    st = dict(dev=dev, pkw=pkw, ahead=ahead, waiting=[], rest=[], new_lists=new_lists,
              cols=dict(up=up, c0=c0, c1=c1, dist=dist, tip=tip, lower=lower, up_right=up_right, up_left=up_left, tot_up=tot_up),
              extra_touched=[], n=n)
    results, root_changes, checks = [], [], []
    otree, since = None, []
    if orc is not None:
        from oracle.oracle_py import OracleTree
        lists4 = []
        for ids in (lower[:n], up_right[:n], up_left[:n], tot_up[:n]):
            have = np.nonzero(ids >= 0)[0]
            lists4.append((have, dev.download_packed(ids[have])))
        otree = OracleTree(orc, int(m.root), up[:n].copy(), np.stack([c0[:n], c1[:n]], axis=1), dist[:n].copy(), None,
                           np.zeros(n, dtype=np.int32), lists4)
    for k in range(n_add if stop is None else stop):
        st["k"], st["n"] = k, n
        dev.placement_prepare(**pkw)
        if ahead > 0 and not st["waiting"]:
            if not st["rest"]:
                st["rest"] = [int(x) for x in dev.upload(new_lists[k: k + ahead])]
            got = dev.placement_ahead(np.asarray(st["rest"], dtype=np.int32), **pkw)
            got = got if got > 0 else len(st["rest"])
            st["waiting"], st["rest"] = st["rest"][:got], st["rest"][got:]
        if hook is not None:
            hook(k, st)
        if ahead > 0:
            qid = st["waiting"].pop(0)
        else:
            qid = int(dev.upload([new_lists[k]])[0])
        mark = dev.mark()
        out = dev.placement_search_batch(np.asarray([qid], dtype=np.int32), **pkw)
        dev.release(mark)
        b = int(out["bestNode"][0])
        res = (int(out["status"][0]), b, float(out["bestScore"][0]), tuple(float(x) for x in out["blen"][0]), int(out["nAppend"][0]))
        results.append(res)
        if otree is not None and k % oracle_every == 0:
            touched = np.unique(np.concatenate([np.asarray(x, dtype=np.int64) for x in since + st["extra_touched"]] or [np.zeros(0, np.int64)]))
            st["extra_touched"] = []
            since = []
            lists4 = []
            for col in (lower, up_right, up_left, tot_up):
                ids = col[touched]
                have = touched[ids >= 0]
                lists4.append((have, dev.download_packed(col[have])))
            otree.update(orc, int(m.root), up[:n].copy(), np.stack([c0[:n], c1[:n]], axis=1), dist[:n].copy(), np.zeros(n, dtype=np.int32), lists4)
            o = orc.find_best_parent_for_new_sample(otree, new_lists[k], allowedFails=5, strictStopRules=True, **pkw)
            checks.append((k, o, res))
        if res[0] != 0 or up[b] < 0:
            continue
        top, bottom, app = res[3]
        g, p, s = int(up[b]), n, n + 1
        depth, dstep = bench.place_depths(depth, dstep, g, p, b, s, m.root, c0, c1, n)
        if c0[g] == b:
            c0[g] = p
        else:
            c1[g] = p
        up[p], c0[p], c1[p], dist[p], tip[p] = g, b, s, top, 0
        up[b], dist[b] = p, bottom
        up[s], dist[s], tip[s], lower[s] = p, app, 1, qid
        n += 2
        root_lower = int(lower[m.root])
        dev.update_partials(m.root, up[:n], c0[:n], c1[:n], tip[:n], mut[:n], depth[:n], dist[:n], lower[:n], up_right[:n],
                            up_left[:n], tot_up[:n], [b, s, p])
        if int(lower[m.root]) != root_lower:
            root_changes.append(k)
        touched = np.unique(np.concatenate([dev.update_partials_touched(), [g, b, p, s]])).astype(np.int32)
        dev.tree_patch(n, touched, up[touched], c0[touched], c1[touched], dist[touched], tip[touched], lower[touched],
                       up_right[touched], up_left[touched], tot_up[touched])
        since.append(touched)
    st["n"] = n
    return dict(results=results, root_changes=root_changes, checks=checks, st=st)


def check_against_oracle(checks, min_checks):
    """The oracle's answer on the sampled searches: status, node and nAppend exact, score 1e-9 relative, lengths 1e-8; a different
    node only as a tie (both scores within 1e-11 relative), at most one in a hundred checks."""
    ties = 0
    for k, (ost, onode, oscore, oblen, _, onapp), (gst, gnode, gscore, gblen, gnapp) in checks:
        assert ost == gst, (k, ost, gst)
        if onode != gnode:
            assert abs(oscore - gscore) <= 1e-11 * max(1.0, abs(oscore)), (k, onode, gnode, oscore, gscore)
            ties += 1
            continue
        assert onapp == gnapp, (k, onapp, gnapp)
        assert abs(oscore - gscore) <= 1e-9 * max(1.0, abs(oscore)), (k, oscore, gscore)
        if ost == 0:
            assert np.allclose(oblen, gblen, rtol=1e-8, atol=1e-15), (k, oblen, gblen)
    assert len(checks) >= min_checks and ties <= len(checks) // 100, (len(checks), ties)
    return ties


def small_world(mode, n_tips, seed, n_add, near_root=0, **dev_kw):
    """A small tree (n_tips tips) and n_add new samples: perturbed copies of random tips, every 25th an exact copy (a minor
    sequence), and -- near_root > 0 -- copies of the near_root tips closest to the root.  dev_kw: for the Device."""
    from maple_amd.host import tip_genome_list
    from maple_amd.synth import perturb_diffs
    data, dev, orc, m = build(n_tips, mode, seed=seed, **dev_kw)
    kw = world_model_kwargs(mode, dev.lRef, seed)
    tip_kw = dict(error_rates=kw["errorRates"]) if mode == "siteerr" else {}
    prng = np.random.default_rng(seed + 7)
    src = list(prng.choice(len(data.diffs), size=n_add, replace=True))
    if near_root:
        node_of = {int(v): i for i, v in enumerate(data.tip_node)}
        d = np.full(m.n_nodes, -1)
        d[m.root] = 0
        order = [m.root]
        for v in order:
            for c in m.children[v]:
                if c >= 0:
                    d[c] = d[v] + 1
                    order.append(int(c))
        shallow = sorted((int(d[v]), v) for v in node_of)[:near_root]
        for j, (_, v) in enumerate(shallow):
            src[(3 * j + 1) % n_add] = node_of[v]
    new_lists = []
    for k, i in enumerate(src):
        dl = data.diffs[int(i)] if k % 25 == 0 else perturb_diffs(data.diffs[int(i)], data.ref, prng)
        new_lists.append(tip_genome_list(dl, dev.ref_idx, **tip_kw))
    return data, dev, orc, m, new_lists


def test_announced_loop_root_column_under_full_row_fallback():
    """Finding 1: when the traversal asks for a branch the expansion did not reach, the sample's row is scored in full once more --
    and the root's column of that row must stay the CURRENT root vector's score.  A 300-tip tree, the expansion cut short
    (no_ahead_expansion=2: most searches fall back), copies of the tips closest to the root among the samples.  The placements
    of the stand-in edit do not give the root a new lower list on this tree (updatePartials stops below it), so the root's list
    is rewritten in place every 5th step with the list of the sample searched next, which then goes to the root: a stale root
    column gives another result."""
    data, dev, orc, m, new_lists = small_world("ratevar", 300, 31, 120, near_root=8)
    pkw = small_pkw(dev.lRef)
    saved = []

    def new_root_list(k, st):
        # (the placements do not give the root a new lower list on this tree: every 5th step it is rewritten in place --
        # maple_lists_update, then maple_tree_patch of the root -- with the list of the sample searched next, which then scores
        # best at the root; a stale root column gives another result)
        if k % 5:
            return
        cols, d = st["cols"], st["dev"]
        rid = int(cols["lower"][m.root])
        saved.append((rid, d.download([rid])[0]))
        d.update_lists([rid], [st["new_lists"][k]])
        v = np.asarray([m.root], dtype=np.int32)
        d.tree_patch(st["n"], v, *(cols[c][v] for c in ("up", "c0", "c1", "dist", "tip", "lower", "up_right", "up_left", "tot_up")))
        st["extra_touched"].append(v)
        st.setdefault("root_rewrites", []).append(k)

    runs, stats = [], []
    for ahead, expansion in ((0, 0), (40, 2)):
        mark = dev.mark()
        dev.set_tuning(no_ahead_expansion=expansion)
        before = dev.placement_ahead_stats()
        runs.append(serial_loop(dev, m, new_lists, pkw, ahead=ahead, hook=new_root_list, orc=orc if ahead else None, oracle_every=6))
        after = dev.placement_ahead_stats()
        stats.append({k: after[k] - before[k] for k in after})
        for rid, lst in reversed(saved):                                   # (the tree's own lists back for the next loop)
            dev.update_lists([rid], [lst])
        saved.clear()
        dev.release(mark)
    dev.set_tuning()
    plain, ahead = runs
    assert plain["results"] == ahead["results"]
    assert plain["root_changes"] == ahead["root_changes"]
    rewrites = ahead["st"]["root_rewrites"]
    assert len(rewrites) >= 20, rewrites
    assert sum(ahead["results"][k][1] == m.root for k in rewrites) >= 10       # (the rewritten root list did change the results)
    assert stats[1]["searches"] == len(new_lists) and stats[1]["fallbacks"] > 0.5 * len(new_lists), stats[1]
    check_against_oracle(ahead["checks"], 15)
    next_to_root = sum(1 for r in ahead["results"] if r[0] == 0 and r[1] in (int(m.children[m.root][0]), int(m.children[m.root][1])))
    print(f"root lower list renewed at {len(ahead['root_changes'])} of {len(new_lists)} steps by the placements, rewritten at "
          f"{len(rewrites)}; {next_to_root} placed on a child "
          f"branch of the root; {stats[1]}")
    dev.close()


def test_announced_loop_sees_a_list_rewritten_in_place():
    """Finding 2: maple_lists_update keeps a list's id; the node is then passed to maple_tree_patch with unchanged ids.  Between
    two announced searches, the mid-branch (tot_up) list of the branch the next sample goes to (found by a plain loop without
    the rewrite) gets the contents of a far branch's mid-branch list: a tip's in the other subtree of the root.  The branch then
    scores far worse for that sample and the search returns another node; a row left stale keeps the old winner.  The rewrite
    comes right after the second batch is announced (no column of that batch is dirty yet), and the rows hold every branch
    (no_ahead_expansion=1: no search falls back to scoring its row in full, which would hide a stale column).  The plain loop
    gets the same rewrite; every search must equal it, and the oracle on the rewritten tree."""
    data, dev, orc, m, new_lists = small_world("unrest", 300, 37, 40)
    pkw = small_pkw(dev.lRef)
    at = 16                                                              # (the first sample of the second batch of 16)
    done, winner = [], []

    def rewrite(k, st):
        if k != at:
            return
        cols, d = st["cols"], st["dev"]
        w = winner[0]
        assert w != m.root
        side = w
        while cols["up"][side] != m.root:                                  # (the child of the root above the winner)
            side = int(cols["up"][side])
        other = int(cols["c1"][m.root] if cols["c0"][m.root] == side else cols["c0"][m.root])
        far, stack = [], [other]                                           # (tips below the other child with a mid-branch list)
        while stack:
            v = stack.pop()
            if cols["c0"][v] >= 0:
                stack += [int(cols["c0"][v]), int(cols["c1"][v])]
            elif cols["dist"][v] > pkw["effectivelyNon0BLen"] and cols["tot_up"][v] >= 0:
                far.append(v)
        assert far
        tid = int(cols["tot_up"][w])
        done.append((w, tid, d.download([tid])[0]))
        d.update_lists([tid], d.download([int(cols["tot_up"][far[0]])]))
        v = np.asarray([w], dtype=np.int32)
        d.tree_patch(st["n"], v, *(cols[c][v] for c in ("up", "c0", "c1", "dist", "tip", "lower", "up_right", "up_left", "tot_up")))
        st["extra_touched"].append(v)

    mark = dev.mark()
    untouched = serial_loop(dev, m, new_lists, pkw)                      # (the plain loop without the rewrite)
    dev.release(mark)
    assert untouched["results"][at][0] == 0
    winner.append(untouched["results"][at][1])
    runs, stats = [], []
    for ahead in (0, 16):
        mark = dev.mark()
        dev.set_tuning(no_ahead_expansion=1)
        before = dev.placement_ahead_stats()
        runs.append(serial_loop(dev, m, new_lists, pkw, ahead=ahead, hook=rewrite, orc=orc if ahead else None, oracle_every=1))
        after = dev.placement_ahead_stats()
        dev.set_tuning()
        stats.append({k: after[k] - before[k] for k in after})
        _, tid, original = done[-1]
        dev.update_lists([tid], [original])                              # (the list as it was, in case it is the tree's own)
        dev.release(mark)
    plain, ahead = runs
    print(f"winner {winner[0]} rewritten: the search after it {untouched['results'][at]} -> {plain['results'][at]}")
    assert plain["results"][at][1] != untouched["results"][at][1]      # (the rewrite moves the decision: a stale row would not)
    assert plain["results"] == ahead["results"]
    assert stats[1]["searches"] == len(new_lists) and stats[1]["fallbacks"] == 0, stats[1]
    check_against_oracle(ahead["checks"], 30)
    dev.close()


def test_announced_loop_interleaved_calls_mid_batch():
    """Calls between two announced searches, each followed by the rest of the announced samples: a search of a sample that was
    not announced; placement_prepare with another effectivelyNon0BLen and back; a release of a mark below announced samples'
    lists (they are uploaded and announced again); set_model with the same model.  maple_hip.h says which of these drop the
    rows; the results must be those of the plain loop with the same calls in between."""
    mode = "ratevar"
    data, dev, orc, m, new_lists = small_world(mode, 400, 41, 72)
    pkw = small_pkw(dev.lRef)
    kw = world_model_kwargs(mode, dev.lRef, 41)
    stranger = new_lists[5]
    seen = {}

    def interleave(k, st):
        d = st["dev"]
        if k == 3:                                                          # a search of a sample nobody announced
            mk = d.mark()
            qid = d.upload([stranger])
            seen.setdefault(st["ahead"], []).append(d.placement_search_batch(qid, **st["pkw"]))
            d.release(mk)
        elif k == 9:                                                        # other parameters of the tables, then these again
            d.placement_prepare(**dict(st["pkw"], effectivelyNon0BLen=st["pkw"]["effectivelyNon0BLen"] * 50))
            d.placement_prepare(**st["pkw"])
        elif k == 20:                                                       # the waiting samples' lists released, then again
            if st["ahead"]:
                mk = d.mark()
                ids = [int(x) for x in d.upload([st["new_lists"][k + j] for j in range(len(st["waiting"]))])]
                assert d.placement_ahead(np.asarray(ids, dtype=np.int32), **st["pkw"]) > 0
                d.release(mk)
                ids = [int(x) for x in d.upload([st["new_lists"][k + j] for j in range(len(ids))])]
                got = d.placement_ahead(np.asarray(ids, dtype=np.int32), **st["pkw"])
                st["waiting"] = ids[:got] if got > 0 else ids
        elif k == 30:                                                       # the same model again
            d.set_model(**kw)

    runs, stats = [], []
    for ahead in (0, 24):
        mark = dev.mark()
        before = dev.placement_ahead_stats()
        runs.append(serial_loop(dev, m, new_lists, pkw, ahead=ahead, hook=interleave, orc=orc if ahead else None, oracle_every=4))
        after = dev.placement_ahead_stats()
        stats.append({k: after[k] - before[k] for k in after})
        dev.release(mark)
    plain, ahead = runs
    assert plain["results"] == ahead["results"]
    for k in ("status", "bestNode", "bestScore", "blen", "nAppend"):
        assert np.array_equal(seen[0][0][k], seen[24][0][k]), k
    assert stats[1]["searches"] >= len(new_lists) // 2, stats[1]
    check_against_oracle(ahead["checks"], 15)
    print("interleaved:", stats[1])
    dev.close()


def test_announced_loop_closed_mid_batch_then_a_fresh_context():
    """A context closed halfway through an announced batch, with the traversal of the next sample made ahead on (its thread is
    joined before anything is freed); a fresh context then runs the whole loop: the plain loop's results.  The context closed
    mid-batch leaves no GPU resource behind (live_resources)."""
    before = live_resources()
    data, dev, orc, m, new_lists = small_world("ratevar", 300, 43, 48, debug=True)
    pkw = small_pkw(dev.lRef)
    mark = dev.mark()
    plain = serial_loop(dev, m, new_lists, pkw, ahead=0)
    dev.release(mark)
    half = serial_loop(dev, m, new_lists, pkw, ahead=48, stop=24)        # (48 announced, 24 searched)
    assert half["results"] == plain["results"][:24]
    assert dev.placement_ahead_stats()["traversals_ahead_used"] > 0
    dev.close()
    assert np.array_equal(live_resources(), before), (live_resources(), before)
    data2, dev2, orc2, m2, lists2 = small_world("ratevar", 300, 43, 48)
    assert all(a == b for a, b in zip(lists2, new_lists))
    whole = serial_loop(dev2, m2, lists2, pkw, ahead=48)
    assert whole["results"] == plain["results"]
    assert dev2.placement_ahead_stats()["searches"] == len(new_lists)
    dev2.close()


# ---- a closed context leaves nothing behind ------------------------------------------------------------------------------
# Every GPU resource of a context -- device and page-locked memory, streams, events -- belongs to an owning member that counts
# itself into a process-wide ledger (maple_debug_live_resources: allocations, bytes, handles).  Each test reads the ledger before
# its context is created and after close() and requires the three differences to be zero (differences: the counters are shared
# by every context of the process).

def live_resources():
    from maple_amd.runtime import debug_live_resources
    return np.asarray(debug_live_resources(), dtype=np.int64)


def tiny_context(**kw):
    from maple_amd.runtime import Device
    ref_idx = np.arange(2000, dtype=np.uint8) % 4
    return Device(ref_idx, [0.25, 0.25, 0.25, 0.25], debug=True, **kw)


def test_live_resources_bare_context():
    before = live_resources()
    dev = tiny_context(arena_bytes=64 << 20)
    dev.close()
    assert np.array_equal(live_resources(), before), (live_resources(), before)


def test_live_resources_move_with_a_context():
    """The ledger is wired to the owners: a context alone holds its arena, its tables and its stream."""
    before = live_resources()
    dev = tiny_context(arena_bytes=64 << 20)
    held = live_resources() - before
    dev.close()
    assert held[0] >= 12 and held[1] >= 64 << 20 and held[2] >= 1, held
    assert np.array_equal(live_resources(), before), (live_resources(), before)


def test_live_resources_two_contexts_closed_in_reverse_order():
    before = live_resources()
    a = tiny_context(arena_bytes=64 << 20)
    b = tiny_context(arena_bytes=32 << 20)
    a.set_model(Q)
    b.set_model(Q, siteRates=np.ones(2000))
    b.close()
    a.close()
    assert np.array_equal(live_resources(), before), (live_resources(), before)


def test_live_resources_failed_creation():
    """maple_create refused for lack of memory (an arena of twice the card's memory: one allocation request the runtime turns
    down) frees what it had got by then."""
    import torch
    from maple_amd.runtime import MapleError
    total = int(torch.cuda.mem_get_info(0)[1])
    before = live_resources()
    with pytest.raises(MapleError):
        tiny_context(arena_bytes=2 * total)
    assert np.array_equal(live_resources(), before), (live_resources(), before)


def deep_round(dev, m, upload):
    """One deep SPR round over every node of the tree, frontier tier; the tree uploaded through ``upload``."""
    import bench
    upload()
    return dev.spr_search_batch(bench.preorder_nodes(m), **bench.search_kwargs(dev.lRef))


def test_live_resources_after_every_kind_of_call():
    """A 300-tip world with site-specific error rates (the error-rate tables exist) that has been through pair batches, an
    announced placement loop with updatePartials and tree patches, a traced search, a deep SPR round and a candidate set it
    never destroyed."""
    import bench
    before = live_resources()
    data, dev, orc, m, new_lists = small_world("siteerr", 300, 47, 8, debug=True, arena_bytes=1 << 30)
    assert (live_resources() - before > 0).all()

    def upload():
        dev.upload_tree(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.dist, m.is_tip, m.lower, m.up_right, m.up_left,
                        m.tot_up, -np.ones(m.n_nodes, dtype=np.int32))
    tips = np.nonzero(m.is_tip)[0][:64]
    a, b = m.lower[tips], m.lower[tips[::-1]]
    merged = dev.merge_batch(a, 1e-4, True, b, 2e-4, True, False)
    ok = merged >= 0
    assert ok.any()
    assert np.isfinite(dev.append_batch(merged[ok], a[ok], True, 1.0 / dev.lRef)).any()
    dev.blen_batch(merged[ok], a[ok], True)
    nodes = bench.preorder_nodes(m)
    upload()
    dev.debug_trace_query(0)
    dev.spr_search_batch(nodes[:32], **bench.search_kwargs(dev.lRef))
    assert len(dev.debug_trace_read()[0]) > 0
    dev.debug_trace_query(-1)
    g = deep_round(dev, m, upload)
    assert (g["status"] == 0).sum() > 100
    dev.candset_create(m.tot_up[m.candidate_nodes(0.0)], np.zeros(len(m.candidate_nodes(0.0)), dtype=np.int32), 1)
    loop = serial_loop(dev, m, new_lists, small_pkw(dev.lRef), ahead=8)   # (placement, rows made ahead, update_partials, tree_patch)
    assert sum(r[0] == 0 for r in loop["results"]) > 0 and len(dev.update_partials_touched()) > 0
    dev.close()
    assert np.array_equal(live_resources(), before), (live_resources(), before)


def test_live_resources_after_whole_tree_searches_on_a_tree_with_local_references():
    """The same on a 300-tip tree with rate variation that carries MAT local references: a search from a zero-length branch
    runs over its budget and becomes a whole-tree search, whose removed list goes into every reference frame on the device
    (fan_out_level) before the dense kernel scores it -- scratch of its own, and dense launches in the timing records."""
    import bench
    from maple_amd.mat import add_local_references
    from maple_amd.tree_host import HostTree
    before = live_resources()
    data, dev, orc, m = build(300, "ratevar", seed=4, debug=True, arena_bytes=1 << 30)
    ht = HostTree.from_mirror(m)
    assert add_local_references(dev, ht, 50) > 0
    dist = np.asarray([float(x or 0.0) for x in ht.dist])
    nodes = bench.preorder_nodes(m)
    assert (dist[nodes] == 0.0).any()

    def upload():
        dev.upload_tree(ht.root, m.parent, m.children[:, 0], m.children[:, 1], dist, m.is_tip, ht.id_lower, ht.id_upRight, ht.id_upLeft,
                        ht.id_totUp, ht.id_mut)
    dev.timing_reset()
    g = deep_round(dev, m, upload)
    assert (g["status"] == 0).sum() > 100
    dense = dev.timing_read_kind(dev.KIND_SPR_SCORE)
    assert dense[0] > 0 and dense[2] > 0, dense                             # (whole-tree searches were scored: launches, searches)
    dev.debug_trace_query(0)
    dev.spr_search_batch(nodes[:32], **bench.search_kwargs(dev.lRef))
    dev.debug_trace_query(-1)
    dev.close()
    assert np.array_equal(live_resources(), before), (live_resources(), before)
