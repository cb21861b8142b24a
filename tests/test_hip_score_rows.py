"""GPU differential tests of the score rows of the whole-tree SPR searches: the witness filter (maple_amd/csrc/witness.hip) and
the dense kernel's bitmap form (launch_append_queries with finMask), run on explicit lists through maple_debug_score_rows, then
the bitmap's prefix counts (k_finite_prefix) -- against the C oracle's appendProbNode on every (search, candidate) pair of the
corpus le.witness_corpus (tests/test_list_edges_coverage.py gates what that corpus reaches and how it is balanced).

Bars (those of the rest of the suite, none new): the bitmap, the prefix counts and the pair counts are exact integer identities;
a finite score is within 1e-12 relative of the oracle (REL_APPEND, test_hip_list_edges.py); kernel forms agree bit for bit.  The
table is filled with NaN before the launch: a cell without a finite score must still hold it ("-inf by omission").
"""
import numpy as np
import pytest

import list_edges as le

pytestmark = pytest.mark.gpu
REL_APPEND = 1e-12
DENSE, WITNESS = 0, 1
ERR_MODES = ("gerr", "siteerr")


class Rows:
    """The lists of a mode on the device, and what the oracle and the rule say about every pair (made once, never changed)."""

    def __init__(self, dev, o, mode):
        self.mode = mode
        self.qs, self.cs = le.witness_corpus(mode) if mode in le.WITNESS_MODES else le.dense_lists(mode)
        self.q_ids = dev.upload(self.qs)
        have = [k for k, c in enumerate(self.cs) if c is not None]
        self.c_ids = np.full(len(self.cs), -1, dtype=np.int32)
        self.c_ids[have] = dev.upload([self.cs[k] for k in have])
        self.nQ, self.nC = len(self.qs), len(self.cs)
        self.o = o
        self._want = {}
        self.excl = le.witness_matrix(self.qs, self.cs) if mode in le.WITNESS_MODES else None
        rng = np.random.default_rng(7)
        self.mixTip = rng.random(self.nQ) < 0.5
        self.mixBLen = rng.choice([0.0, 1e-5, 1e-3], size=self.nQ)

    def want(self, tip, bl):
        """The oracle's rows for qTip `tip` (a bool or the mixed vector) and qBLen `bl` (0.0 or the mixed vector)."""
        key = (tip if isinstance(tip, bool) else "mix", "mix" if isinstance(bl, np.ndarray) else bl)
        if key not in self._want:
            w = le.oracle_rows(self.o, self.qs, self.cs, tip, bl)
            w.setflags(write=False)
            self._want[key] = w
        return self._want[key]


@pytest.fixture(scope="module")
def ctx():
    from maple_amd.runtime import Device
    from oracle.oracle_py import Oracle
    ref = le.reference()
    dev = Device(ref, le.ROOT_FREQS, arena_bytes=256 << 20, debug=True)
    o = Oracle(ref, le.ROOT_FREQS)
    rows = {}

    def use(mode):
        dev.set_model(**le.model(mode))
        o.set_model(**le.model(mode))
        dev.set_tuning()
        if mode not in rows:
            rows[mode] = Rows(dev, o, mode)
        return dev, rows[mode]
    yield use
    dev.close()


def bit_rows(mask, nC):
    """bool [nQ, nC] of the bitmap; the bits past nC in the last word must be clear."""
    b = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(len(mask), -1), axis=1, bitorder="little").astype(bool)
    assert not b[:, nC:].any()
    return b[:, :nC]


def check_prefix(mask, prefix):
    pop = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(mask.shape + (8,)), axis=2).sum(axis=2).astype(np.int64)
    cum = np.concatenate([np.zeros((len(mask), 1), dtype=np.int64), np.cumsum(pop, axis=1)], axis=1)
    assert prefix.shape == cum.shape and np.array_equal(prefix, cum), np.argwhere(prefix != cum)[:5]
    assert np.array_equal(prefix[:, -1], pop.sum(axis=1))


def check_rows(got, want, c_ids, col, what):
    """One call's (out, finMask, prefix) against the oracle's rows `want` [nQ, nC]."""
    out, mask, prefix = got[:3]
    nQ, nC = want.shape
    fin = np.isfinite(want)
    bits = bit_rows(mask, nC)
    assert not bits[:, c_ids < 0].any(), what
    assert np.array_equal(bits, fin), (what, np.argwhere(bits != fin)[:5])
    col = np.arange(nC) if col is None else np.asarray(col)
    cells = out[:, col]
    assert np.isfinite(cells[fin]).all(), what
    if fin.any():
        err = np.abs(cells[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
        assert err.max() <= REL_APPEND, (what, err.max(), np.argwhere(fin)[np.argmax(err)])
    written = np.zeros(out.shape, dtype=bool)
    written[:, col] = fin
    assert np.isnan(out[~written]).all(), (what, np.argwhere(~written & ~np.isnan(out))[:5])      # padding columns included
    check_prefix(mask, prefix)


def score(dev, form, R, qsel, csel, tip, bl, permuted):
    """maple_debug_score_rows on a selection of the mode's lists; returns (the call's results, the oracle's rows, ids, columns)."""
    qsel, csel = np.asarray(qsel), np.asarray(csel)
    nC = len(csel)
    ld = nC + 7 if permuted else nC
    col = np.random.default_rng(nC).permutation(ld)[:nC].astype(np.int32) if permuted else None
    tipv = np.broadcast_to(tip, R.nQ)[qsel]
    blv = np.broadcast_to(bl, R.nQ)[qsel]
    got = dev.debug_score_rows(form, R.q_ids[qsel], tipv, blv, R.c_ids[csel], out_col=col, ld_out=ld)
    assert got[0].shape == (len(qsel), ld)
    return got, R.want(tip, bl)[np.ix_(qsel, csel)], R.c_ids[csel], col


def selections(R):
    """The whole corpus, then nC in {1, 64, 65} x nQ in {1, 63} drawn across the families."""
    rng = np.random.default_rng(11)
    yield np.arange(R.nQ), np.arange(R.nC)
    for nC in (1, 64, 65):
        for nQ in (1, 63):
            yield np.sort(rng.permutation(R.nQ)[:nQ]), np.sort(rng.permutation(R.nC)[:nC])


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("mode", le.WITNESS_MODES)
def test_witness_rows_against_the_oracle(ctx, mode):
    """The witness filter's rows: a bit exactly where the oracle's score is finite, that score within 1e-12, every other cell
    untouched; both values of qTip, a permuted outCol with ldOut = nC + 7 and outCol = NULL, nWords = 1, 2 and 4."""
    dev, R = ctx(mode)
    words = set()
    for n, (qsel, csel) in enumerate(selections(R)):
        for tip, permuted in ((False, True), (True, n % 2 == 1)) if n else ((False, True), (True, True), (True, False)):
            got, want, ids, col = score(dev, WITNESS, R, qsel, csel, tip, 0.0, permuted)
            check_rows(got, want, ids, col, (mode, len(qsel), len(csel), tip, permuted))
            assert 0 <= got[3] <= len(qsel) * len(csel)
            words.add(got[1].shape[1])
    assert words == {1, 2, 4}
    assert (R.c_ids < 0).sum() >= 2


@pytest.mark.parametrize("mode", le.WITNESS_MODES + ERR_MODES)
def test_dense_bitmap_rows_against_the_oracle(ctx, mode):
    """The dense kernel's bitmap form (what the over-budget and error-model searches use): per-query qTip and qBLen from
    {0, 1e-5, 1e-3}, outCol, ldOut > nC -- against the oracle, and its finite cells bit for bit against maple_append_batch."""
    dev, R = ctx(mode)
    runs = [(R.mixTip, R.mixBLen, True), (False, 0.0, True), (True, 0.0, False)]
    for n, (qsel, csel) in enumerate(selections(R)):
        for tip, bl, permuted in (runs if n == 0 else runs[:1]):
            got, want, ids, col = score(dev, DENSE, R, qsel, csel, tip, bl, permuted)
            check_rows(got, want, ids, col, (mode, len(qsel), len(csel), permuted))
            assert got[3] == -1
            if n == 0:                                             # (the lane-per-pair kernel on the same pairs)
                have = np.flatnonzero(ids >= 0)
                pi, qi = np.tile(have, len(qsel)), np.repeat(np.arange(len(qsel)), len(have))
                lane = dev.append_batch(ids[pi], R.q_ids[qsel][qi], np.broadcast_to(tip, R.nQ)[qsel][qi],
                                        np.broadcast_to(bl, R.nQ)[qsel][qi]).reshape(len(qsel), len(have))
                cells = got[0][:, np.arange(len(csel)) if col is None else col][:, have]
                fin = np.isfinite(lane)
                assert np.array_equal(fin, np.isfinite(want[:, have])) and np.isneginf(lane[~fin]).all()
                assert same_bits(cells[fin], lane[fin])


@pytest.mark.parametrize("mode", le.WITNESS_MODES)
def test_witness_form_equals_dense_form(ctx, mode):
    """witness.hip: "the rows the dense kernel writes, bit for bit" -- table (fill included), bitmap and prefix counts."""
    dev, R = ctx(mode)
    for n, (qsel, csel) in enumerate(selections(R)):
        a = score(dev, WITNESS, R, qsel, csel, R.mixTip, 0.0, True)[0]
        b = score(dev, DENSE, R, qsel, csel, R.mixTip, 0.0, True)[0]
        assert same_bits(a[0], b[0]), np.argwhere(a[0].view(np.uint64) != b[0].view(np.uint64))[:5]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("mode", le.WITNESS_MODES)
def test_witness_walks_what_the_rule_cannot_exclude(ctx, mode):
    """Pairs walked: at least the pairs no witness can exclude, at most all; on candidates with at most one eligible entry
    (wit_sites, wit_none) exactly what the rule gives -- the filter filters; and a second call, on the reused scratch buffers,
    gives the same count and the same rows."""
    dev, R = ctx(mode)
    allq, allc = np.arange(R.nQ), np.arange(R.nC)
    first = score(dev, WITNESS, R, allq, allc, False, 0.0, True)[0]
    must = int((~R.excl).sum())
    assert must <= first[3] <= R.nQ * R.nC, (must, first[3])
    rng = le.witness_family_ranges(mode)
    csel = np.array(list(rng["wit_sites"][1]) + list(rng["wit_none"][1]))
    assert all(R.cs[k] is None or len(le.witness_eligible(R.cs[k])) <= 1 for k in csel)
    sub = score(dev, WITNESS, R, allq, csel, False, 0.0, True)[0]
    assert sub[3] == int((~R.excl[:, csel]).sum()), (sub[3], int((~R.excl[:, csel]).sum()))
    assert 0 < int(R.excl[:, csel].sum())
    again = score(dev, WITNESS, R, allq, allc, False, 0.0, True)[0]
    assert again[3] == first[3] and same_bits(again[0], first[0])
    assert np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])


@pytest.mark.parametrize("mode", ("unrest", "ratevar"))
def test_tiled_shapes(ctx, mode):
    """nC = 4097 (nWords = 65: the prefix kernel's second pass, word 64) against 8 queries, and nQ = 1025 (the pair-offset scan
    with more than one count per lane) against 65 candidates: tiled columns and rows repeat bit for bit, the first period is
    the oracle's, both forms agree."""
    dev, R = ctx(mode)
    rng = np.random.default_rng(5)
    for nQ, nC in ((8, 4097), (1025, 65)):
        q0 = np.sort(rng.permutation(R.nQ)[:min(nQ, 41)])
        c0 = np.arange(R.nC) if nC > R.nC else np.sort(rng.permutation(R.nC)[:nC])
        qsel, csel = np.resize(q0, nQ), np.resize(c0, nC)
        want = R.want(R.mixTip, 0.0)[np.ix_(qsel, csel)]
        res = []
        for form in (WITNESS, DENSE):
            got = dev.debug_score_rows(form, R.q_ids[qsel], R.mixTip[qsel], 0.0, R.c_ids[csel])
            check_rows(got, want, R.c_ids[csel], None, (mode, form, nQ, nC))
            out, mask = got[0], bit_rows(got[1], nC)
            assert same_bits(out, out[np.arange(nQ) % len(q0)][:, np.arange(nC) % len(c0)])
            assert np.array_equal(mask, mask[np.arange(nQ) % len(q0)][:, np.arange(nC) % len(c0)])
            assert got[2].shape == (nQ, (nC + 63) // 64 + 1)
            res.append(got)
        assert same_bits(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
        assert 0 < res[0][3] <= nQ * nC
        if nC == 4097:
            assert res[0][2].shape[1] == 66 and res[0][1][:, 64].any()       # (word 64 holds a finite score)


def test_witness_form_refuses_an_error_model(ctx):
    """Under an error model the witness form is the library's MAPLE_ERR_STATE, not a row; the context stays usable."""
    from maple_amd.runtime import MapleError
    dev, R = ctx("gerr")
    qsel, csel = np.arange(R.nQ), np.arange(R.nC)
    with pytest.raises(MapleError) as ei:
        score(dev, WITNESS, R, qsel, csel, False, 0.0, True)
    assert ei.value.code == MapleError.ERR_STATE
    got, want, ids, col = score(dev, DENSE, R, qsel, csel, False, 0.0, True)
    check_rows(got, want, ids, col, "gerr, after the refusal")
