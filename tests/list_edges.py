"""Adversarial genome lists for the list operators (appendProbNode, mergeVectors, estimateBranchLengthWithDerivative,
evaluatePlacement): seeded cases aimed at branches that the recorded golden calls never take and synthetic trees rarely do.

A helper module like golden_util.py.  Lists are in the reference's tuple grammar (maple_amd/genome_list.py, M:378-390):
positions increase and every list ends at lRef, O vectors are normalised, d1 only follows d0, and the flag element appears
only under an error model.  `model(mode)` gives the settings of a model mode, `corpus(mode)` its cases, one family per
branch:

  append_d1_O       appendProbNode, R or a nucleotide with d0 and d1 against an O vector at <= 0.02 (M:6611-6633, 6744-6761)
  append_carry      appendProbNode with hundreds of differing sites: three and more carry-overs (M:6772-6783)
  merge_carry       mergeVectors(returnLK=True) with more than 70 differing sites on both sides (M:4830-4840)
  merge_underflow   mergeVectors(returnLK=True) whose running factor falls below DBL_MIN in one step (the reference
                    raises, M:4831-4836)
  merge_updown      mergeVectors(isUpDown=True): N against an entry with d0 under an error model (M:4517-4518), N against
                    an O vector of total length 0 (M:4560-4561)
  blen_none         estimateBranchLengthWithDerivative against a zero rate of Q (M:5171-5172, 5178-5179, 5241-5242):
                    only in the zero-rate modes
  blen_tenth        the early return of 0.1 (M:5341-5342)
  evalplace_fallback  evaluatePlacement whose top merge is None: bestTop = defaultBLen * 0.1 (M:6798-6802)
  skip_edges        lists at the edges of the skipping form of append_lds.h (skip_form_drops): a single-site entry at
                    position 1 and at lRef, adjacent single-site entries, a tail-less R in front of an N run or of an R with
                    a tail, a list without any R entry
  long              lists longer than the dense kernel stages (> MAPLE_QLDS entries, chunks over MAPLE_LDS_CAPW/CAPA)
"""
import numpy as np

L_REF = 1500
ROOT_FREQS = [0.3, 0.2, 0.2, 0.3]
Q_JC = [[-1.0 if i == j else 1.0 / 3.0 for j in range(4)] for i in range(4)]
Q_UNREST = [[-0.9, 0.2, 0.5, 0.2], [0.3, -1.4, 0.1, 1.0], [0.8, 0.1, -1.3, 0.4], [0.1, 0.6, 0.1, -0.8]]
# two rates of zero (A->C, G->T): the None exits of estimateBranchLengthWithDerivative (maple_set_model does not validate Q)
Q_ZERO = [[-0.7, 0.0, 0.5, 0.2], [0.3, -1.4, 0.1, 1.0], [0.8, 0.1, -0.9, 0.0], [0.1, 0.6, 0.1, -0.8]]
ZERO_RATES = [(0, 1), (2, 3)]
MODES = ["jc", "unrest", "ratevar", "gerr", "siteerr", "zeroq", "zeroq_err"]


def reference():
    """The reference genome of every mode: rich in C and G, whose rates under Q_UNREST are above 1 -- the genome's total rate
    is above lRef, which the evaluatePlacement family needs (c1 < 0 on lists that are N nearly everywhere)."""
    rng = np.random.default_rng(1)
    return rng.choice(4, size=L_REF, p=[0.2, 0.3, 0.3, 0.2]).astype(np.uint8)


def model(mode):
    """kwargs of Oracle.set_model / Device.set_model for a mode."""
    rng = np.random.default_rng(2)
    sr = rng.uniform(0.3, 2.0, L_REF)
    er = rng.uniform(1e-5, 5e-3, L_REF)
    return {
        "jc": dict(Q=Q_JC),
        "unrest": dict(Q=Q_UNREST),
        "ratevar": dict(Q=Q_UNREST, siteRates=list(sr)),
        "gerr": dict(Q=Q_UNREST, usingErrorRate=True, errorRateGlobal=1e-3),
        "siteerr": dict(Q=Q_UNREST, siteRates=list(sr), usingErrorRate=True, errorRateGlobal=1e-3, errorRates=list(er)),
        "zeroq": dict(Q=Q_ZERO),
        "zeroq_err": dict(Q=Q_ZERO, siteRates=list(sr), usingErrorRate=True, errorRateGlobal=1e-3, errorRates=list(er)),
    }[mode]


def site_rates(mode, ref):
    """-Q[ref][ref] * siteRate per site (1-based position p at index p - 1): what cumulativeRate sums."""
    m = model(mode)
    q = np.asarray(m["Q"], dtype=np.float64)
    r = -q[ref, ref]
    if m.get("siteRates") is not None:
        r = r * np.asarray(m["siteRates"])
    return r


class Builder:
    """One list, entry by entry, in increasing position; gaps become tail-less reference runs."""

    def __init__(self, ref, u):
        self.ref, self.u, self.L = ref, u, len(ref)
        self.out, self.cur = [], 0

    def _tail(self, d0, d1, flag):
        if d0 is None:
            return ()
        t = (float(d0),) if d1 is None else (float(d0), float(d1))
        return t + ((bool(flag),) if self.u else ())

    def _gap(self, p):
        if p - 1 > self.cur:
            self.out.append((4, p - 1))
            self.cur = p - 1
        assert p - 1 == self.cur, (p, self.cur)

    def nuc(self, p, nuc, d0=None, d1=None, flag=False):
        r = int(self.ref[p - 1])
        assert nuc != r and 0 <= nuc < 4
        self._gap(p)
        self.out.append((int(nuc), r) + self._tail(d0, d1, flag))
        self.cur = p
        return self

    def o(self, p, vec, d0=None):
        self._gap(p)
        v = [float(x) for x in vec]
        s = sum(v)
        v = [x / s for x in v]
        self.out.append((6, int(self.ref[p - 1]), v) if d0 is None else (6, int(self.ref[p - 1]), float(d0), v))
        self.cur = p
        return self

    def run(self, typ, start, end, d0=None, d1=None, flag=False):
        self._gap(start)
        self.out.append((typ, int(end)) + (self._tail(d0, d1, flag) if typ == 4 else ()))
        self.cur = end
        return self

    def done(self):
        if self.cur < self.L:
            self.out.append((4, self.L))
        return self.out


def other(rng, r, avoid=()):
    return int(rng.choice([x for x in range(4) if x != r and x not in avoid]))


def o_vec(rng, low_at, low):
    """A normalised vector whose entry low_at is `low` (before normalisation the rest sums to 1 - low)."""
    rest = rng.dirichlet([1.0, 1.0, 1.0]) * (1.0 - low)
    v, k = [], 0
    for i in range(4):
        if i == low_at:
            v.append(low)
        else:
            v.append(float(rest[k]))
            k += 1
    return v


def random_list(rng, ref, u, n_sites, lo=1, hi=None, tails=True, flags=True):
    """A tip-like list: n_sites non-reference nucleotides at random positions in [lo, hi], some with a tail."""
    L = len(ref)
    hi = hi or L
    sites = np.sort(rng.choice(np.arange(lo, hi + 1), size=n_sites, replace=False))
    b = Builder(ref, u)
    for p in sites:
        p = int(p)
        d0 = float(rng.choice([1e-5, 3e-4])) if (tails and rng.random() < 0.3) else None
        if u and d0 is None and flags and rng.random() < 0.3:
            d0 = 0.0
        b.nuc(p, other(rng, int(ref[p - 1])), d0=d0, flag=flags and bool(rng.random() < 0.5))
    return b.done()


# ---- the families -------------------------------------------------------------------------------------------------------
def fam_append_d1_O(rng, ref, u, n=48):
    """Parent with R or a nucleotide carrying d0 and d1 at site s; the child an O vector at s whose entry for that nucleotide
    is 0.001-0.02 (the 0.02 shortcut does not apply)."""
    out = []
    L = len(ref)
    for k in range(n):
        s = int(rng.integers(20, L - 20))
        r = int(ref[s - 1])
        d0 = float(rng.choice([0.0, 1e-4, 0.01]))
        d1 = float(rng.choice([1e-5, 2e-3]))
        flag = bool(k % 3 == 0)
        P = Builder(ref, u)
        if k % 2 == 0:                                        # R with both lengths over s
            P.run(4, s - 3, s + 4, d0=d0, d1=d1, flag=flag)
            i1 = r
        else:                                                 # a nucleotide with both lengths at s
            i1 = other(rng, r)
            P.nuc(s, i1, d0=d0, d1=d1, flag=flag)
        P.nuc(s + 10, other(rng, int(ref[s + 9])), d0=1e-4, d1=3e-4, flag=not flag)
        Cb = Builder(ref, u)
        Cb.nuc(s - 7, other(rng, int(ref[s - 8])))
        Cb.o(s, o_vec(rng, i1, float(rng.uniform(0.001, 0.02))), d0=(None if k % 4 < 2 else 2e-4))
        out.append(dict(P=P.done(), C=Cb.done(), isTipC=bool(k % 5 != 0), bLen=float(rng.choice([0.0, 1e-5, 1e-3]))))
    return out


def fam_append_carry(rng, ref, u, n=8):
    """Hundreds of differing sites: factors near 1e-4 each, so the running product is carried over three times and more."""
    out = []
    for k in range(n):
        P = random_list(rng, ref, u, int(rng.integers(250, 400)), flags=False)
        Cl = random_list(rng, ref, u, int(rng.integers(250, 400)), tails=False)
        out.append(dict(P=P, C=Cl, isTipC=bool(k % 2), bLen=float(rng.choice([1e-5, 1e-4]))))
    return out


def fam_merge_carry(rng, ref, u, n=8):
    out = []
    for k in range(n):
        a = random_list(rng, ref, u, int(rng.integers(75, 300)))
        b = random_list(rng, ref, u, int(rng.integers(75, 300)))
        out.append(dict(pv1=a, b1=float(rng.choice([1e-5, 1e-4])), tip1=bool(k % 2), pv2=b, b2=float(rng.choice([1e-5, 2e-4])),
                        tip2=bool(k % 3 == 0), returnLK=True, isUpDown=bool(k % 4 == 3)))
    return out


def fam_merge_underflow(rng, ref, u, n=6):
    """Two lists that differ at a few sites over branches of 1e-170: each such site multiplies the running factor by about
    1e-170, and the second one takes it below DBL_MIN without passing the carry-over threshold first."""
    out = []
    L = len(ref)
    for k in range(n):
        b1, b2 = Builder(ref, u), Builder(ref, u)
        for s in sorted(int(x) for x in rng.choice(np.arange(5, L - 5), size=3, replace=False)):
            r = int(ref[s - 1])
            if k % 2:
                b1.nuc(s, other(rng, r))
            else:
                x = other(rng, r)
                b1.nuc(s, x)
                b2.nuc(s, other(rng, r, (x,)))
        out.append(dict(pv1=b1.done(), b1=1e-170, tip1=False, pv2=b2.done(), b2=1e-170, tip2=False, returnLK=True,
                        isUpDown=bool(k % 3 == 0)))
    return out


def fam_merge_updown(rng, ref, u, n=16):
    """isUpDown merges: pv1 is N over stretches where pv2 has entries with d0 (and a flag, under an error model) and O
    vectors without any length (bLen2 = 0)."""
    out = []
    L = len(ref)
    for k in range(n):
        s = int(rng.integers(50, L - 60))
        a = Builder(ref, u).run(5, s - 5, s + 30).done()
        b = Builder(ref, u)
        b.nuc(s, other(rng, int(ref[s - 1])), d0=float(rng.choice([1e-4, 0.0 if u else 2e-3])), flag=bool(k % 2))
        b.run(4, s + 2, s + 6, d0=3e-4, flag=bool(k % 3 == 0))
        b.o(s + 8, rng.dirichlet([1.0] * 4))
        b.o(s + 9, rng.dirichlet([1.0] * 4), d0=1e-4)
        pv2 = b.done()
        b2 = 0.0 if k % 2 == 0 else 1e-4
        out.append(dict(pv1=a, b1=1e-4, tip1=False, pv2=pv2, b2=b2, tip2=False, returnLK=bool(k % 4 == 1), isUpDown=True))
    return out


def fam_blen_none(rng, ref, u, n=12):
    """Only in the zero-rate modes: every coefficient site meets a zero rate of Q (no other sites, so that the reference's
    unguarded division of M:5246 is never reached)."""
    out = []
    L = len(ref)
    at = {x: [p for p in range(30, L - 30) if int(ref[p - 1]) == x] for x in range(4)}     # sites whose reference is x
    for k in range(n):
        fr, to = ZERO_RATES[k % 2]
        s = int(rng.choice(at[fr]))
        P, Cb = Builder(ref, u), Builder(ref, u)
        kind = k % 3
        if kind == 0:                                         # R with d1 over s, the child's nucleotide `to` (M:5171-5172)
            P.run(4, s - 2, s + 2, d0=1e-4, d1=2e-4)
            Cb.nuc(s, to)
            tip = False
        elif kind == 1:                                       # tail-less R, a flagged `to` (M:5178-5179; error model only)
            Cb.nuc(s, to, d0=1e-4 if u else None, flag=True)
            tip = bool(u)
        else:                                                 # a nucleotide `fr` with d1 where the reference is `to`, the
            P.nuc(int(rng.choice(at[to])), fr, d0=1e-4, d1=3e-4)  # child R there: coeff1 = rf[fr] * Q[fr][to] (M:5241-5242)
            tip = False
        out.append(dict(P=P.done(), C=Cb.done(), fromTipC=tip))
    return out


def fam_blen_tenth(rng, ref, u, rates, n=4):
    """Both lists N outside a window of reference sites; in it the child has one tail-less nucleotide (a zero coefficient) and
    one with a tail of 1.0 (a coefficient of 1.0).  The window is grown until c1 = lRef - (rate of every site but the
    window's reference-against-reference ones) lies in [3, 9]: then tDown = 0.1 and vDown = 10 + 1 / 1.1 > c1."""
    out = []
    L = len(ref)
    tot = float(np.sum(rates))
    for k in range(n):
        a = int(rng.integers(100, 300)) + 200 * k
        s1, s2 = a + 1, a + 3
        w = 5
        while True:
            rr = [p for p in range(a, a + w) if p not in (s1, s2)]
            c1 = L - (tot - float(np.sum(rates[np.asarray(rr) - 1])))
            if 3.0 <= c1 <= 9.0 or w > L - a - 10:
                break
            w += 1
        assert 3.0 <= c1 <= 9.0, c1
        end = a + w - 1
        P = Builder(ref, u).run(5, 1, a - 1).run(4, a, end).run(5, end + 1, L).done()
        Cb = Builder(ref, u).run(5, 1, a - 1)
        Cb.nuc(s1, other(rng, int(ref[s1 - 1])))
        Cb.nuc(s2, other(rng, int(ref[s2 - 1])), d0=1.0)
        Cb.run(4, s2 + 1, end).run(5, end + 1, L)
        out.append(dict(P=P, C=Cb.done(), fromTipC=False))
    return out


def fam_evalplace_fallback(rng, ref, u, n=6):
    """evaluatePlacement(midTot, down, up, distance, removed): up and removed are N but for a site where they have two
    different nucleotides, midTot is removed and down is N.  bestApp and bestTop both come out 0 (no coefficient site; c1 <
    0 because the genome's total rate is at least lRef), so the top merge meets a zero-length mismatch and returns None."""
    out = []
    L = len(ref)
    for k in range(n):
        s = int(rng.integers(10, L - 10))
        r = int(ref[s - 1])
        y = other(rng, r)
        x = other(rng, r, (y,))
        up = Builder(ref, u).run(5, 1, s - 1).nuc(s, y).run(5, s + 1, L).done()
        rem = Builder(ref, u).run(5, 1, s - 1).nuc(s, x).run(5, s + 1, L).done()
        down = [(5, L)]
        out.append(dict(midTot=rem, down=down, up=up, distance=float(rng.choice([1e-4, 2e-3])), rem=rem, isRemovedTip=False,
                        fromTip1=bool(k % 2)))
    return out


def skip_edge_lists(rng, ref, u):
    """Lists at the edges of the skipping form (append_lds.h): each one is a named shape."""
    L = len(ref)
    r = lambda p: int(ref[p - 1])                              # noqa: E731
    out = {}
    out["site_at_1"] = Builder(ref, u).nuc(1, other(rng, r(1))).nuc(40, other(rng, r(40))).done()
    out["O_at_1"] = Builder(ref, u).o(1, o_vec(rng, r(1), 0.01)).done()
    out["site_at_lRef"] = Builder(ref, u).nuc(300, other(rng, r(300))).nuc(L, other(rng, r(L))).done()
    out["O_at_lRef"] = Builder(ref, u).o(L, o_vec(rng, r(L), 0.005), d0=1e-4).done()
    b = Builder(ref, u)
    for p in range(500, 508):
        if p % 3 == 0:
            b.o(p, o_vec(rng, r(p), 0.01))
        else:
            b.nuc(p, other(rng, r(p)), d0=1e-4 if p % 2 else None, flag=True)
    out["adjacent_sites"] = b.done()
    out["R_before_N"] = Builder(ref, u).run(5, 200, 260).nuc(261, other(rng, r(261))).run(5, 700, 710).done()
    out["R_before_tailR"] = (Builder(ref, u).run(4, 600, 640, d0=2e-4, flag=True).nuc(641, other(rng, r(641)))
                             .run(4, 900, 950, d0=1e-4, d1=1e-3).done())
    b = Builder(ref, u).run(5, 1, 99)
    for p in (100, 101, 102):
        b.nuc(p, other(rng, r(p)))
    out["no_R"] = b.run(5, 103, L).done()
    out["no_R_sites_only_ends"] = Builder(ref, u).nuc(1, other(rng, r(1))).run(5, 2, L - 1).nuc(L, other(rng, r(L))).done()
    out["all_N"] = [(5, L)]
    out["all_R"] = [(4, L)]
    out["all_R_tail"] = Builder(ref, u).run(4, 1, L, d0=1e-4, d1=2e-4, flag=False).done()
    return out


def fam_skip_edges(rng, ref, u):
    """Every pair of the named edge lists, both ways round."""
    lists = skip_edge_lists(rng, ref, u)
    names = sorted(lists)
    out = []
    for i, a in enumerate(names):
        for j, b in enumerate(names):
            out.append(dict(P=lists[a], C=lists[b], isTipC=bool((i + j) % 2), bLen=float([0.0, 1e-5, 1e-3][(i * 3 + j) % 3]),
                            name=(a, b)))
    return out


def long_lists(rng, ref, u, n=6):
    """Lists of 300+ entries (not staged as queries, > MAPLE_QLDS) and lists heavy in stored lengths and O vectors (a chunk
    of them is over MAPLE_LDS_CAPA aux doubles)."""
    out = [random_list(rng, ref, u, int(rng.integers(160, 260))) for _ in range(n)]
    for k in range(n):
        b = Builder(ref, u)
        for p in sorted(int(x) for x in rng.choice(np.arange(2, len(ref)), size=40, replace=False)):
            if p % 2:
                b.o(p, rng.dirichlet([1.0] * 4), d0=1e-4)
            else:
                b.nuc(p, other(rng, int(ref[p - 1])), d0=1e-4, d1=2e-4, flag=True)
        out.append(b.done())
    return out


def corpus(mode):
    """{family: [case dict]} of a mode (a family a mode cannot reach is left out)."""
    ref = reference()
    m = model(mode)
    u = bool(m.get("usingErrorRate"))
    rng = np.random.default_rng(100 + MODES.index(mode))
    if mode.startswith("zeroq"):
        return {"blen_none": fam_blen_none(rng, ref, u)}
    rates = site_rates(mode, ref)
    fams = {
        "append_d1_O": fam_append_d1_O(rng, ref, u),
        "append_carry": fam_append_carry(rng, ref, u),
        "merge_carry": fam_merge_carry(rng, ref, u),
        "merge_underflow": fam_merge_underflow(rng, ref, u),
        "merge_updown": fam_merge_updown(rng, ref, u),
        "blen_tenth": fam_blen_tenth(rng, ref, u, rates),
        "evalplace_fallback": fam_evalplace_fallback(rng, ref, u),
        "skip_edges": fam_skip_edges(rng, ref, u),
        "long": [dict(P=a, C=b, isTipC=True, bLen=1e-4) for a, b in zip(*(2 * [iter(long_lists(rng, ref, u))]))],
    }
    return fams


def dense_lists(mode):
    """(queries, candidates) for the dense kernel: the family lists of a mode plus the skipping-form edges and long lists, in
    an order that gives staged and unstaged chunks (short candidates first, long ones after) and a partial last chunk."""
    ref = reference()
    u = bool(model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(200 + MODES.index(mode))
    fam = corpus(mode)
    edges = list(skip_edge_lists(rng, ref, u).values())
    longs = long_lists(rng, ref, u)
    cands = [c["P"] for c in fam["append_d1_O"]] + edges
    cands = (cands * 3)[:64]                                   # chunk 0: 64 short lists
    cands += longs * 11                                        # chunks 1-2: heavy (unstaged)
    cands += [c["P"] for c in fam["append_d1_O"]][:21] + edges  # a partial last chunk
    queries = [c["C"] for c in fam["append_d1_O"]] + edges + longs
    return queries, cands


def check_grammar(gl, L, u):
    """Raise AssertionError unless gl follows the tuple grammar."""
    pos = 0
    for e in gl:
        t = e[0]
        if t in (4, 5):
            assert e[1] > pos, (e, pos)
            pos = e[1]
        else:
            pos += 1
        if t == 6:
            v = e[-1]
            assert len(e) in (3, 4) and abs(sum(v) - 1.0) < 1e-12 and min(v) >= 0.0, e
        elif t == 5:
            assert len(e) == 2, e
        else:
            if u:
                assert len(e) in (2, 4, 5) and (len(e) == 2 or isinstance(e[-1], bool)), e
            else:
                assert len(e) in (2, 3, 4) and not any(isinstance(x, bool) for x in e), e
    assert pos == L, (pos, L)
