"""GPU differential tests on the adversarial corpus of tests/list_edges.py: every device form of appendProbNode,
mergeVectors, estimateBranchLengthWithDerivative and evaluatePlacement against the C oracle on the same inputs, in every
model mode that reaches the family (tests/test_list_edges_coverage.py gates that the corpus reaches each branch).

Bars (those of the rest of the suite): integer structure exact, including None, False, fatal and -inf outcomes;
appendProbNode within 1e-12 relative of the oracle (test_hip_scale.py), the other operators within 1e-9
(test_hip_parity.py); kernel forms bit for bit against each other.
"""
import math
import os
import re

import numpy as np
import pytest

import list_edges as le
from golden_util import close, lists_match

pytestmark = pytest.mark.gpu
REL_APPEND = 1e-12
REL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STD_MODES = le.MODES[:5]


def kernel_constant(name):
    """A #define of maple_amd/csrc/append_queries.hip: the routes of the dense kernel follow the constants the library is built with."""
    with open(os.path.join(ROOT, "maple_amd", "csrc", "append_queries.hip")) as fh:
        return int(re.search(rf"#define {name} (\d+)", fh.read()).group(1))


@pytest.fixture(scope="module")
def ctx():
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref = le.reference()
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20)
    dbg = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20, debug=True)
    o = Oracle(ref, le.ROOT_FREQS)
    corp = {m: le.corpus(m) for m in le.MODES}
    yield dev, dbg, o, corp
    dev.close()
    dbg.close()


def use(ctx, mode):
    dev, dbg, o, corp = ctx
    for x in (dev, dbg, o):
        x.set_model(**le.model(mode))
    dev.set_tuning()
    return dev, dbg, o, corp[mode]


def same_value(a, b, rel):
    a, b = float(a), float(b)
    if math.isinf(b) or math.isinf(a):
        return a == b
    return close(a, b, rel)


APPEND_FAMS = ("append_d1_O", "append_carry", "skip_edges", "long")


@pytest.mark.parametrize("mode", STD_MODES)
def test_appendProbNode_every_form(ctx, mode):
    """k_append (> 1024 pairs, and again with the wavefront forms switched off), k_wave_append (<= 1024 pairs) and the
    wavefront walk of the debug library on the families of appendProbNode."""
    dev, dbg, o, fam = use(ctx, mode)
    cases = [c for f in APPEND_FAMS for c in fam[f]]
    n = len(cases)
    assert n <= 1024
    want = np.array([o.appendProbNode(c["P"], c["C"], c["isTipC"], c["bLen"]) for c in cases])
    lists = [c["P"] for c in cases] + [c["C"] for c in cases]
    tips, bls = [c["isTipC"] for c in cases], [c["bLen"] for c in cases]
    mark, mark_d = dev.mark(), dbg.mark()
    ids, ids_d = dev.upload(lists), dbg.upload(lists)
    wave = dev.append_batch(ids[:n], ids[n:], tips, bls)                              # k_wave_append
    reps = 1024 // n + 1
    lane = dev.append_batch(np.tile(ids[:n], reps), np.tile(ids[n:], reps), np.tile(tips, reps), np.tile(bls, reps))
    assert len(lane) > 1024                                                           # k_append, one lane per pair
    dev.set_tuning(wave_per_item_max=-1)
    lane_small = dev.append_batch(ids[:n], ids[n:], tips, bls)                        # k_append below 1024 pairs
    dev.set_tuning()
    dwave, _ = dbg.debug_wave_append_batch(ids_d[:n], ids_d[n:], tips, bls)
    dev.release(mark)
    dbg.release(mark_d)
    for k, c in enumerate(cases):
        assert same_value(wave[k], want[k], REL_APPEND), (k, c.get("name"), wave[k], want[k])
    assert np.array_equal(wave, lane[:n]) and np.array_equal(lane.reshape(reps, n), np.tile(lane[:n], (reps, 1)))
    assert np.array_equal(wave, lane_small)
    assert np.array_equal(wave, dwave)
    assert np.isneginf(want).any() and np.isfinite(want).sum() > n // 2


MERGE_FAMS = ("merge_carry", "merge_underflow", "merge_updown")


def oracle_merge(o, c, returnLK):
    try:
        return o.mergeVectors(c["pv1"], c["b1"], c["tip1"], c["pv2"], c["b2"], c["tip2"], returnLK=returnLK,
                              isUpDown=c["isUpDown"])
    except RuntimeError:
        return "fatal"


@pytest.mark.parametrize("mode", STD_MODES)
def test_mergeVectors_every_form(ctx, mode):
    """mergeVectors with the likelihood (k_merge: carry-overs and the underflow, which the reference raises on and the library
    reports as a fatal item) and without it (k_merge_wave and the one-lane k_merge, bit for bit)."""
    dev, dbg, o, fam = use(ctx, mode)
    cases = [c for f in MERGE_FAMS for c in fam[f]]
    n = len(cases)
    args = lambda ids: (ids[:n], [c["b1"] for c in cases], [c["tip1"] for c in cases], ids[n:],          # noqa: E731
                        [c["b2"] for c in cases], [c["tip2"] for c in cases], [c["isUpDown"] for c in cases])
    mark = dev.mark()
    ids = dev.upload([c["pv1"] for c in cases] + [c["pv2"] for c in cases])
    dev.set_fatal_policy(True)
    try:
        out, lk = dev.merge_batch(*args(ids), returnLK=True)
    finally:
        dev.set_fatal_policy(False)
    got_lk = [None if i < 0 else g for i, g in zip(out, dev.download([i if i >= 0 else -1 for i in out]))]
    nw = dev.merge_batch(*args(ids))                                                  # k_merge_wave
    dev.set_tuning(wave_per_item_max=-1)
    nl = dev.merge_batch(*args(ids))                                                  # k_merge, one lane
    dev.set_tuning()
    got_w, got_l = dev.download(nw), dev.download(nl)
    pk_w = dev.download_packed([i for i in nw if i >= 0])
    pk_l = dev.download_packed([i for i in nl if i >= 0])
    dev.release(mark)
    n_fatal = n_carry = 0
    for k, c in enumerate(cases):
        want = oracle_merge(o, c, True)
        if want == "fatal":
            assert out[k] == -2, (k, out[k])
            n_fatal += 1
        elif want is None:
            assert out[k] == -1 and got_lk[k] is None
        else:
            assert lists_match(got_lk[k], want[0], REL), (k, got_lk[k], want[0])
            assert close(float(lk[k]), want[1], REL), (k, lk[k], want[1])
            n_carry += c in fam["merge_carry"]
        want = oracle_merge(o, c, False)
        assert want != "fatal"
        assert lists_match(got_w[k], want, REL), (k, got_w[k], want)
    assert [i < 0 for i in nw] == [i < 0 for i in nl] and got_w == got_l
    for a in ("ent_off", "pos", "meta", "aux_off"):
        assert np.array_equal(getattr(pk_w, a), getattr(pk_l, a))
    assert np.array_equal(pk_w.aux.view(np.uint64), pk_l.aux.view(np.uint64))
    assert n_fatal == len(fam["merge_underflow"]) and n_carry == len(fam["merge_carry"])


def blen_cases(fam):
    out = list(fam.get("blen_tenth", [])) + list(fam.get("blen_none", []))
    out += [dict(P=c["P"], C=c["C"], fromTipC=c["isTipC"]) for c in fam.get("append_d1_O", [])]
    return out


@pytest.mark.parametrize("mode", le.MODES)
def test_estimateBranchLength_every_form(ctx, mode):
    """k_blen_wave and the one-lane k_blen: the early 0.1, the None exits over zero rates of Q, False results."""
    dev, dbg, o, fam = use(ctx, mode)
    cases = blen_cases(fam)
    n = len(cases)
    mark = dev.mark()
    ids = dev.upload([c["P"] for c in cases] + [c["C"] for c in cases])
    tips = [c["fromTipC"] for c in cases]
    tw, fw = dev.blen_batch(ids[:n], ids[n:], tips)
    dev.set_tuning(wave_per_item_max=-1)
    tl, fl = dev.blen_batch(ids[:n], ids[n:], tips)
    dev.set_tuning()
    dev.release(mark)
    n_tenth = 0
    for k, c in enumerate(cases):
        want = o.estimateBranchLengthWithDerivative(c["P"], c["C"], c["fromTipC"])
        if want is False:
            assert fw[k], (k, tw[k])
        else:
            assert not fw[k] and close(float(tw[k]), want, REL), (k, tw[k], want)
        n_tenth += c in fam.get("blen_tenth", []) and want == 0.1
    assert np.array_equal(fw, fl) and np.array_equal(tw, tl)
    assert n_tenth == len(fam.get("blen_tenth", []))


@pytest.mark.parametrize("mode", STD_MODES)
def test_evaluatePlacement_every_form(ctx, mode):
    """k_evalplace_wave and k_evalplace on placements whose top merge is None (the retry with defaultBLen * 0.1)."""
    dev, dbg, o, fam = use(ctx, mode)
    cases = fam["evalplace_fallback"]
    n = len(cases)
    keys = ("midTot", "down", "up", "rem")
    mark = dev.mark()
    ids = dev.upload([c[k] for k in keys for c in cases])
    args = (ids[:n], ids[n:2 * n], ids[2 * n:3 * n], [c["distance"] for c in cases], ids[3 * n:],
            [c["isRemovedTip"] for c in cases], [c["fromTip1"] for c in cases])
    ow = dev.evaluate_placement_batch(*args)
    dev.set_tuning(wave_per_item_max=-1)
    ol = dev.evaluate_placement_batch(*args)
    dev.set_tuning()
    dev.release(mark)
    for k, c in enumerate(cases):
        want = o.evaluatePlacement(c["midTot"], c["down"], c["up"], c["distance"], c["rem"], c["isRemovedTip"], c["fromTip1"])
        assert want[2] == o.defaultBLen * 0.1                                          # bestTop: the fallback
        assert all(same_value(g, w, REL) for g, w in zip(ow[k], want)), (k, ow[k], want)
    assert np.array_equal(ow, ol)


def dense_routes(dev, q_ids, c_ids):
    """Which route of k_append_queries_lds each chunk and query takes (append_queries.hip: a chunk of 64 candidates is staged in
    LDS if its words fit MAPLE_LDS_CAPW and its aux doubles MAPLE_LDS_CAPA; a query if it has <= MAPLE_QLDS entries)."""
    capw, capa, qlds, qb = (kernel_constant(x) for x in ("MAPLE_LDS_CAPW", "MAPLE_LDS_CAPA", "MAPLE_QLDS", "MAPLE_LDS_QB"))
    ne_c, na_c = dev.sizes(c_ids)
    ne_q, _ = dev.sizes(q_ids)
    staged = [int(ne_c[i:i + 64].sum()) <= capw and int(na_c[i:i + 64].sum()) <= capa for i in range(0, len(c_ids), 64)]
    return dict(staged_chunk=any(staged), unstaged_chunk=not all(staged), staged_query=bool((ne_q <= qlds).any()),
                unstaged_query=bool((ne_q > qlds).any()), partial_chunk=len(c_ids) % 64 != 0, query_blocks=len(q_ids) > qb)


@pytest.mark.parametrize("mode", STD_MODES)
def test_dense_kernel_routes_against_the_oracle(ctx, mode):
    """k_append_queries_lds (skipping form) on queries x candidates that take every route: staged and unstaged chunks and
    queries, a partial last chunk, more than one query block -- against the oracle and bit for bit against k_append."""
    import torch
    dev, dbg, o, fam = use(ctx, mode)
    queries, cands = le.dense_lists(mode)
    qb = kernel_constant("MAPLE_LDS_QB")
    reps = qb // len(queries) + 1
    mark = dev.mark()
    q_ids = np.tile(dev.upload(queries), reps)
    c_ids = dev.upload(cands)
    routes = dense_routes(dev, q_ids, c_ids)
    assert all(routes.values()), routes
    nQ, nC = len(q_ids), len(c_ids)
    cu = torch.device("cuda", 0)
    t_q = torch.from_numpy(q_ids.astype(np.int32)).to(cu)
    t_c = torch.from_numpy(c_ids.astype(np.int32)).to(cu)
    out = torch.empty(nQ * nC, dtype=torch.float64, device=cu)
    packed = o.pack_many(cands + queries)
    nq = len(queries)
    for isTip, bl in ((True, 1e-4), (False, 0.0)):
        torch.cuda.synchronize()
        dev.append_queries_dev(nQ, t_q.data_ptr(), nC, t_c.data_ptr(), isTip, bl, out.data_ptr(), 0)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(nQ, nC)
        assert np.array_equal(got, np.tile(got[:nq], (reps, 1)))
        got = got[:nq]
        pi = np.tile(np.arange(nC), nq)
        qi = np.repeat(np.arange(nq), nC)
        want = o.appendProbNode_batch(packed, pi, nC + qi, isTip, bl).reshape(nq, nC)
        lane = dev.append_batch(c_ids[pi], q_ids[qi], isTip, bl).reshape(nq, nC)
        assert np.array_equal(got, lane), np.argwhere(got != lane)[:5]
        fin = np.isfinite(want)
        assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(fin, np.isfinite(got))
        err = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
        assert err.max() <= REL_APPEND, (err.max(), np.argwhere(fin)[np.argmax(err)])
    dev.release(mark)


@pytest.mark.parametrize("mode", STD_MODES)
def test_dense_argmax_ties_dead_rows_and_visit_rank(ctx, mode):
    """append_queries_argmax_dev: per query the best score and its candidate equal the arg-max of the full score matrix, exact
    ties (every candidate three times) going to the smallest visit rank of a permuted rank, rows that are all -inf included."""
    import torch
    dev, dbg, o, fam = use(ctx, mode)
    queries, cands = le.dense_lists(mode)
    ref = le.reference()
    u = bool(le.model(mode).get("usingErrorRate"))
    sd = 777                                                       # a site where every candidate kept below is tail-less R

    def plain_ref_at(gl, s):
        pos = 0
        for e in gl:
            end = e[1] if e[0] in (4, 5) else pos + 1
            if end >= s:
                return e[0] == 4 and len(e) == 2
            pos = end
        return False

    keep = [c for c in cands if plain_ref_at(c, sd)][:40]
    assert len(keep) >= 20
    cset = keep * 3
    dead = le.Builder(ref, u).nuc(sd, le.other(np.random.default_rng(3), int(ref[sd - 1]))).done()
    qs = [dead] + queries
    mark = dev.mark()
    q_ids, c_ids = dev.upload(qs), dev.upload(cset)
    nQ, nC = len(q_ids), len(c_ids)
    assert nQ >= 32
    cu = torch.device("cuda", 0)
    t_q = torch.from_numpy(q_ids.astype(np.int32)).to(cu)
    t_c = torch.from_numpy(c_ids.astype(np.int32)).to(cu)
    rank = np.random.default_rng(11 + le.MODES.index(mode)).permutation(nC).astype(np.int32)
    t_rank = torch.from_numpy(rank).to(cu)
    full = torch.empty(nQ * nC, dtype=torch.float64, device=cu)
    best = torch.empty(nQ, dtype=torch.float64, device=cu)
    idx = torch.empty(nQ, dtype=torch.int32, device=cu)
    torch.cuda.synchronize()
    dev.append_queries_dev(nQ, t_q.data_ptr(), nC, t_c.data_ptr(), False, 0.0, full.data_ptr(), 0)
    dev.append_queries_argmax_dev(nQ, t_q.data_ptr(), nC, t_c.data_ptr(), t_rank.data_ptr(), False, 0.0, best.data_ptr(),
                                  idx.data_ptr(), 0)
    torch.cuda.synchronize()
    m = full.cpu().numpy().reshape(nQ, nC)
    dev.release(mark)
    assert np.isneginf(m[0]).all() and o.appendProbNode(cset[0], dead, False, 0.0) == -math.inf
    for q in range(nQ):
        top = m[q].max()
        ties = np.nonzero(m[q] == top)[0]
        want = ties[np.argmin(rank[ties])]
        assert best[q].item() == top and int(idx[q].item()) == int(want), (q, best[q].item(), top, idx[q].item(), want)
        assert len(ties) >= 3
