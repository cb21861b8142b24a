"""GPU differential tests of the structural list operators on the corpus of tests/list_edges.py (struct_corpus): every
exported device form of passGenomeListThroughBranch, shorten, areVectorsDifferent, rootVector, findProbRoot and
isMinorSequence against the C oracle on the same inputs, in the five standard model modes
(tests/test_list_edges_coverage.py gates that the corpus reaches each rarely taken branch of the six), and the stop rule of
maple_update_partials, which is where areVectorsDifferent decides how far a change travels.

Bars (those of the rest of the suite): integer structure, booleans, 0 / 1 / 2 and -inf exact; lists out of pass and shorten
at tolerance 0.0 (test_hip_parity.test_structural_functions); O vectors and log-likelihoods within 1e-9 relative
(test_hip_parity.REL); kernel forms bit for bit against each other, words and doubles.

The check_* bodies take any binding with the operator ABI: tests/test_cpu_twin.py runs them (forms=False: as uploaded, no
tuning switch) on the CPU twin.
"""
import math

import numpy as np
import pytest

import list_edges as le
from golden_util import close, lists_match

pytestmark = pytest.mark.gpu
REL = 1e-9
STD_MODES = le.MODES[:5]
TILE_OVER = 1024                                                   # batches above this many items go one lane per item


@pytest.fixture(scope="module")
def ctx():
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref = le.reference()
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20)
    o = Oracle(ref, le.ROOT_FREQS)
    corp = {m: le.struct_corpus(m) for m in STD_MODES}
    yield dev, o, corp
    dev.close()


def use(ctx, mode):
    dev, o, corp = ctx
    for x in (dev, o):
        x.set_model(**le.model(mode))
    dev.set_tuning()
    return dev, o, corp[mode]


def same_packed(dev, ids_a, ids_b):
    """Two sets of device lists are the same words and the same doubles, bit for bit."""
    a, b = dev.download_packed(ids_a), dev.download_packed(ids_b)
    return (all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("ent_off", "pos", "meta", "aux_off"))
            and np.array_equal(a.aux.view(np.uint64), b.aux.view(np.uint64)))


def tiled(n):
    """Indices that repeat 0..n-1 until there are more than TILE_OVER items."""
    reps = TILE_OVER // n + 1
    return np.tile(np.arange(n), reps), reps


def every_form(dev, forms, call, n):
    """call(index array) -> list ids or values.  As uploaded; with forms also one lane per item below the threshold
    (wave_per_item_max=-1) and tiled above it.  Returns (as uploaded, [the other forms cut back to n items])."""
    first = call(np.arange(n))
    if not forms:
        return first, []
    dev.set_tuning(wave_per_item_max=-1)
    lane = call(np.arange(n))
    dev.set_tuning()
    idx, reps = tiled(n)
    big = np.asarray(call(idx))
    assert len(big) > TILE_OVER
    return first, [lane, big[:n], big[(reps - 1) * n:]]


def check_pass(dev, o, fam, forms=True):
    """k_pass on the pass families: lists equal to the oracle's at tolerance 0.0."""
    cases = fam["pass_edges"] + fam["pass_random"]
    n = len(cases)
    assert max(len(c["pv"]) for c in cases) > 64 and {len(c["mutations"]) for c in cases} >= {1, 2, 40, 70}
    want = [o.passGenomeListThroughBranch(c["pv"], c["mutations"], c["dirIsUp"]) for c in cases]
    mark = dev.mark()
    ids = dev.upload([c["pv"] for c in cases])
    mids = dev.upload_mutations([c["mutations"] for c in cases])
    ups = np.asarray([c["dirIsUp"] for c in cases])
    out, others = every_form(dev, forms, lambda i: dev.pass_branch_batch(ids[i], mids[i], ups[i]), n)
    got = dev.download(out)
    same = [same_packed(dev, out, x) for x in others]
    dev.release(mark)
    for k, c in enumerate(cases):
        assert lists_match(got[k], want[k], 0.0), (c["name"], got[k], want[k])
    assert all(same), same
    assert any(len(w) > len(c["pv"]) for w, c in zip(want, cases)) and any(len(w) < len(c["pv"]) + 2 * len(c["mutations"]) for w, c in zip(want, cases))


def check_shorten(dev, o, fam, forms=True):
    """k_shorten_wave / k_shorten on the shorten families (and on what pass makes of the pass families)."""
    vecs = [c["vec"] for c in fam["shorten_runs"]]
    vecs += [o.passGenomeListThroughBranch(c["pv"], c["mutations"], c["dirIsUp"]) for c in fam["pass_edges"]]
    n = len(vecs)
    assert max(len(v) for v in vecs) > 512
    want = [o.shorten(v) for v in vecs]
    mark = dev.mark()
    ids = dev.upload(vecs)
    out, others = every_form(dev, forms, lambda i: dev.shorten_batch(ids[i]), n)
    got = dev.download(out)
    same = [same_packed(dev, out, x) for x in others]
    dev.release(mark)
    for k in range(n):
        assert lists_match(got[k], want[k], 0.0), (k, got[k], want[k])
    assert all(same), same
    changed = [w != v for w, v in zip(want, vecs)]
    assert any(changed) and not all(changed)


def check_differ(dev, o, fam, forms=True):
    """k_differ_wave / k_differ, both ways round."""
    cases = fam["differ_edges"]
    n = len(cases)
    want = np.asarray([o.areVectorsDifferent(c["pv1"], c["pv2"]) for c in cases] + [o.areVectorsDifferent(c["pv2"], c["pv1"]) for c in cases])
    mark = dev.mark()
    ids = dev.upload([c["pv1"] for c in cases] + [c["pv2"] for c in cases])
    a, b = np.concatenate([ids[:n], ids[n:]]), np.concatenate([ids[n:], ids[:n]])
    got, others = every_form(dev, forms, lambda i: dev.differ_batch(a[i], b[i]), 2 * n)
    dev.release(mark)
    assert np.array_equal(got, want), [(c["name"], g, w) for c, g, w in zip(cases + cases, got, want) if g != w][:5]
    for k, c in enumerate(cases):
        assert c["expect"] is None or got[k] == c["expect"], c["name"]
    assert all(np.array_equal(got, x) for x in others)
    assert want.any() and not want.all()


def check_rootvec(dev, o, fam):
    """k_root_vector: passes up, root_walk, passes down, shorten_walk."""
    cases = fam["rootvec"]
    assert {len([m for m in c["path"] if m]) for c in cases} >= {0, 1, 3}
    assert {(c["bLen"] > 0, c["isFromTip"]) for c in cases} == {(False, False), (False, True), (True, False), (True, True)}
    want = [o.rootVector(c["pv"], c["bLen"], c["isFromTip"], c["path"]) for c in cases]
    mark = dev.mark()
    ids = dev.upload([c["pv"] for c in cases])
    paths = [dev.upload_mutations(c["path"]) if c["path"] else [] for c in cases]
    got = dev.download(dev.root_vector_batch(ids, [c["bLen"] for c in cases], [c["isFromTip"] for c in cases], paths))
    dev.release(mark)
    for k, c in enumerate(cases):
        assert lists_match(got[k], want[k], REL), (c["name"], got[k], want[k])


def check_rootprob(dev, o, fam):
    """k_root_prob on root-frame lists."""
    cases = fam["rootprob"]
    want = [o.findProbRoot(c["pv"], []) for c in cases]
    mark = dev.mark()
    got = dev.root_prob_batch(dev.upload([c["pv"] for c in cases]))
    dev.release(mark)
    for k, c in enumerate(cases):
        assert math.isfinite(want[k]) and close(float(got[k]), want[k], REL), (c["name"], got[k], want[k])


def check_minor(dev, o, fam, candset=True):
    """k_minor in both modes, both ways round; k_minor_candset (one frame) for a few queries against every first list."""
    cases = fam["minor"]
    n = len(cases)
    mark = dev.mark()
    ids = dev.upload([c["pv1"] for c in cases] + [c["pv2"] for c in cases])
    seen = set()
    for ident in (False, True):
        want = [o.isMinorSequence(c["pv1"], c["pv2"], ident) for c in cases] + [o.isMinorSequence(c["pv2"], c["pv1"], ident) for c in cases]
        got = dev.minor_batch(np.concatenate([ids[:n], ids[n:]]), np.concatenate([ids[n:], ids[:n]]), ident)
        assert [int(g) for g in got] == want, [(c["name"], g, w) for c, g, w in zip(cases + cases, got, want) if g != w][:5]
        seen |= {(ident, w) for w in want}
        if candset:
            cs = dev.candset_create(ids[:n], np.zeros(n, np.int32), 1)
            for q in range(n, 2 * n, max(1, n // 6)):
                got = dev.minor_candset(cs, [ids[q]], ident)
                want = [o.isMinorSequence(c["pv1"], cases[q - n]["pv2"], ident) for c in cases]
                assert [int(g) for g in got] == want, (q, ident)
            dev.candset_destroy(cs)
    dev.release(mark)
    assert seen == {(False, 0), (False, 1), (False, 2), (True, 0), (True, 1)}


@pytest.mark.parametrize("mode", STD_MODES)
def test_passGenomeListThroughBranch_every_form(ctx, mode):
    dev, o, fam = use(ctx, mode)
    check_pass(dev, o, fam)


@pytest.mark.parametrize("mode", STD_MODES)
def test_shorten_every_form(ctx, mode):
    dev, o, fam = use(ctx, mode)
    check_shorten(dev, o, fam)


@pytest.mark.parametrize("mode", STD_MODES)
def test_areVectorsDifferent_every_form(ctx, mode):
    dev, o, fam = use(ctx, mode)
    check_differ(dev, o, fam)


@pytest.mark.parametrize("mode", STD_MODES)
def test_rootVector(ctx, mode):
    dev, o, fam = use(ctx, mode)
    check_rootvec(dev, o, fam)


@pytest.mark.parametrize("mode", STD_MODES)
def test_findProbRoot(ctx, mode):
    dev, o, fam = use(ctx, mode)
    check_rootprob(dev, o, fam)


@pytest.mark.parametrize("mode", STD_MODES)
def test_isMinorSequence(ctx, mode):
    dev, o, fam = use(ctx, mode)
    check_minor(dev, o, fam)


# ---- the frontier tier's own pass and grading -----------------------------------------------------------------------------
def shorten_grade(vec):
    """What shorten (M:3721-3745) makes of a list, and how the frontier tier grades that list: 0 shorten leaves it as it is,
    1 every entry that goes away has the doubles and flag of its run's first entry, 2 otherwise."""
    out, head, last, absorbed, exact = [], vec[0], vec[0], False, True
    for nw in vec[1:]:
        absorb = nw[0] == 4 and head[0] == 4 and len(nw) == len(head)
        for a, b in zip(nw[2:], head[2:]):
            absorb = absorb and (a == b if isinstance(a, bool) else abs(a - b) <= le.THR)
        if absorb:
            absorbed = True
            exact = exact and nw[2:] == head[2:]
        else:
            out.append(last)
            head = nw
        last = nw
    out.append(last)
    return out, (0 if not absorbed else (1 if exact else 2))


@pytest.mark.parametrize("mode", STD_MODES)
def test_frontier_pass_and_grading(ctx, mode):
    """passGenomeListThroughBranch of a removed list as the frontier tier of the SPR search runs it -- one lane per item
    (fpass_removed: fpass_store + shorten_would_merge) and one wavefront per item (wave_pass, which re-implements the walk: a
    lane per entry, a binary search of the mutation list, a prefix sum) -- on the pass families and on the shorten families
    with one mutation elsewhere (at lRef): lists equal to the oracle's at tolerance 0.0, the two forms bit for bit, and the
    grade 0 / 1 / 2 of what shorten() would do to the new list (a wrong 0 keeps a search in the tier where the reference edits
    the removed list in place, M:7087).  In the product these functions are reached only from inside a search on a tree with
    MAT local references; the hook (maple_debug_frontier_pass_batch) compiles them into kernels of its own, so this checks the
    source the search is built from, not the search's own object code."""
    from maple_amd.runtime import Device
    dev, o, fam = use(ctx, mode)
    ref = le.reference()
    L = le.L_REF
    at_end = [le.mutation(ref, L, False, (int(ref[L - 1]) + 1) % 4)]
    cases = [(c["pv"], c["mutations"], c["dirIsUp"]) for c in fam["pass_edges"] + fam["pass_random"]]
    cases += [(c["vec"], at_end, False) for c in fam["shorten_runs"]]
    cases += [(c["vec"], [], bool(k % 2)) for k, c in enumerate(fam["shorten_runs"][:4])]         # a branch without mutations
    n = len(cases)
    want = [o.passGenomeListThroughBranch(pv, ms, up) if ms else pv for pv, ms, up in cases]
    grades = []
    for w in want:
        short, g = shorten_grade(w)
        assert short == o.shorten(w) and (g == 0) == (short == w)
        grades.append(g)
    dbg = Device(ref, le.ROOT_FREQS, arena_bytes=64 << 20, debug=True)
    try:
        dbg.set_model(**le.model(mode))
        ids = dbg.upload([pv for pv, _, _ in cases])
        mids = dbg.upload_mutations([ms for _, ms, _ in cases])
        mids[-1] = -1                                                   # (and no branch at all)
        ups = [up for _, _, up in cases]
        res = []
        for wave in (False, True):
            out, grade, same = dbg.debug_frontier_pass_batch(ids, mids, ups, wave_form=wave)
            assert [bool(x) for x in same] == [not ms for _, ms, _ in cases]
            assert all(out[k] == ids[k] for k in range(n) if same[k]) and all(out[k] != ids[k] for k in range(n) if not same[k])
            got = dbg.download(out)
            for k in range(n):
                assert lists_match(got[k], want[k], 0.0), (wave, k, got[k], want[k])
            new = [k for k in range(n) if not same[k]]
            assert [int(grade[k]) for k in new] == [grades[k] for k in new], [(k, int(grade[k]), grades[k]) for k in new if grade[k] != grades[k]][:5]
            res.append(out[new])
        assert same_packed(dbg, res[0], res[1])
        assert {grades[k] for k in new} == {0, 1, 2}
    finally:
        dbg.close()


# ---- the stop rule inside maple_update_partials ----------------------------------------------------------------------------
def stop_rule_lists(rng, ref, u):
    """Tips A, B, C of the tree root -> (inner, C), inner -> (A, B): A and B differ at some sites (O vectors in their parent's
    lower list) and A has an N run over sites where B has entries (entries with a length there)."""
    r = lambda p: int(ref[p - 1])                              # noqa: E731
    a, b, c = le.Builder(ref, u), le.Builder(ref, u), le.Builder(ref, u)
    for p in (100, 300, 500):
        x = le.other(rng, r(p))
        a.nuc(p, x)
        b.nuc(p, le.other(rng, r(p), (x,)))
    a.nuc(650, le.other(rng, r(650)))
    b.nuc(700, le.other(rng, r(700)))
    a.run(5, 800, 840)
    b.nuc(820, le.other(rng, r(820)))
    c.nuc(300, le.other(rng, r(300))).nuc(1200, le.other(rng, r(1200)))
    return a.done(), b.done(), c.done()


def moved_copies(new, u):
    """[(name, copy of `new` changed in one place)]: one O component moved as in each window case of le.WINDOW (scaled by y / x,
    or set to 0), the other three renormalised; one tail moved by 0.5 and by 2 thresholdProb."""
    out = []
    o_at = [k for k, e in enumerate(new) if e[0] == 6]
    t_at = [k for k, e in enumerate(new) if e[0] < 5 and len(e) > 2]
    assert o_at and t_at
    for k in o_at[:2]:
        vec = new[k][-1]
        for i in (int(np.argmin(vec)), int(np.argmax(vec))):
            for (x, y, _) in le.WINDOW:
                moved = vec[i] * (y / x) if x > 0.0 else 0.0
                if moved == vec[i] or moved >= 1.0:
                    continue
                scale = (1.0 - moved) / (1.0 - vec[i])
                v = [moved if j == i else vec[j] * scale for j in range(4)]
                out.append((("O", k, i, x, y), le.replace_entry(new, k, new[k][:-1] + (v,))))
    for k in t_at[:2]:
        e = new[k]
        for f in (0.5, 2.0):
            out.append((("tail", k, f), le.replace_entry(new, k, e[:2] + (e[2] + f * le.THR,) + e[3:])))
    return out


@pytest.mark.parametrize("mode", STD_MODES)
def test_update_partials_stops_where_areVectorsDifferent_says(ctx, mode):
    """maple_update_partials on the five-node tree root -> (inner, tip C), inner -> (tip A, tip B), A marked changed, inner's
    old lower list a copy of the right one moved in one place: inner's lower list is always replaced; root's exactly when the
    oracle's areVectorsDifferent(new, old) says so (M:5793), in both kernel forms of the level (one wavefront per item, one
    lane per item), which leave the same ids and lists.  Lists replaced: inner's lower list and A's probVectTotUp, plus root's
    lower list and inner's probVectTotUp when the change travels on; the upper lists come out as they were, so none of them is
    replaced."""
    dev, o, _ = use(ctx, mode)
    ref = le.reference()
    u = bool(le.model(mode).get("usingErrorRate"))
    A, B, Cl = stop_rule_lists(np.random.default_rng(7), ref, u)
    bl = 1e-5
    new = o.shorten(o.mergeVectors(A, bl, True, B, bl, True))
    ROOT, INNER, TC, TA, TB = 0, 1, 2, 3, 4
    up = np.asarray([-1, 0, 0, 1, 1], np.int32)
    c0 = np.asarray([1, 3, -1, -1, -1], np.int32)
    c1 = np.asarray([2, 4, -1, -1, -1], np.int32)
    tip = np.asarray([0, 0, 1, 1, 1], np.uint8)
    mut = np.full(5, -1, np.int32)
    depth = np.asarray([0, 1, 1, 2, 2], np.int32)
    copies = moved_copies(new, u)
    want = [o.areVectorsDifferent(new, old) for _, old in copies]
    assert any(want) and not all(want)
    mark = dev.mark()
    tips = dev.upload([Cl, A, B])
    dist0 = np.asarray([0.0, bl, bl, bl, bl])
    lower0 = np.asarray([-1, -1, tips[0], tips[1], tips[2]], np.int32)
    lo, ur, ul, tu, bad = dev.tree_rebuild_lists(ROOT, up, c0, c1, tip, None, dist0.copy(), lower0)
    assert len(bad) == 0 and lists_match(dev.download([lo[INNER]])[0], new, REL)
    olds = dev.upload([old for _, old in copies])
    for k, (name, old) in enumerate(copies):
        res = []
        for wave in (0, -1):
            dev.set_tuning(wave_per_item_max=wave)
            inner_mark = dev.mark()                                 # (both forms allocate from the same place: their ids can be compared)
            cols = [x.copy() for x in (lo, ur, ul, tu)]
            cols[0][INNER] = olds[k]
            dist = dist0.copy()
            n_rep = dev.update_partials(ROOT, up, c0, c1, tip, mut, depth, dist, *cols, [TA])
            touched = set(int(v) for v in dev.update_partials_touched())
            assert cols[0][INNER] != olds[k] and (cols[0][ROOT] != lo[ROOT]) == want[k], (name, want[k])
            assert touched == ({TA, INNER, ROOT} if want[k] else {TA, INNER}), (name, touched)
            assert n_rep == (4 if want[k] else 2), (name, n_rep)
            assert np.array_equal(dist, dist0) and all(np.array_equal(c[[TC, TB]], x[[TC, TB]]) for c, x in zip(cols, (lo, ur, ul, tu)))
            new_ids = [int(c[v]) for c in cols for v in range(5) if c[v] >= 0]
            res.append(([c.tolist() for c in cols], dev.download_packed(new_ids)))
            assert lists_match(dev.download([cols[0][INNER]])[0], new, REL)
            dev.release(inner_mark)
        dev.set_tuning()
        (ids_w, pk_w), (ids_l, pk_l) = res
        assert ids_w == ids_l
        assert all(np.array_equal(getattr(pk_w, a), getattr(pk_l, a)) for a in ("ent_off", "pos", "meta", "aux_off"))
        assert np.array_equal(pk_w.aux.view(np.uint64), pk_l.aux.view(np.uint64))
    dev.release(mark)
