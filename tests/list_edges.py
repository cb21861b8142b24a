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
  sink_flag         (error models) three lists of a five-node tree (tests/sink_trees.py) whose new-root merges hand flagged R runs
                    and nucleotides, several hundred of them, to findProbRoot: from a tip against N (`U && tip` of
                    merge_step_body.inc) and from stored flags
  sink_abandon      five-node trees, one per place where findBestRoot gives a rooting up (M:7803-7840): upVect underflows or is
                    None, the new root's merge underflows or is None, a side given up next to a scored one

`struct_corpus(mode)` gives the families of the structural operators (passGenomeListThroughBranch, shorten,
areVectorsDifferent, rootVector, findProbRoot, isMinorSequence), one per group of counters of oracle/maple_oracle_bc.h:

  shorten_runs      runs of adjacent R entries in every tail form: the run-head rule (a candidate is compared with the run's
                    FIRST entry: d0 = a, a + 0.8 * thresholdProb, a + 1.6 * thresholdProb keeps two entries, a neighbour rule
                    one), refusals on the flag alone, runs that straddle entry 64 and entry 128 of a list, a list of more
                    than 512 entries
  pass_edges        named shapes: a mutation at position 1 and at lRef, on the first / last site of an R run, on adjacent
                    sites, three and more in one run, R runs with every tail form, N runs that skip mutations, nucleotides
                    that become R or keep their type, O entries -- each in both directions
  pass_random       rich lists of more than 64 entries against mutation lists of 1, 2 and several dozen mutations
  differ_edges      a list against a copy changed in one place, one case per return of areVectorsDifferent, and the
                    fold-change window of O components (`expect` holds the answer where it is known by construction)
  rootvec           lower lists with paths of 0, 1 and 3 mutated branches, bLen 0 and > 0, both values of isFromTip
  rootprob          root-frame lower lists: flagged R runs and nucleotides, several hundred O entries (carry-overs)
  minor             pairs of tip-like lists for isMinorSequence: every arm of the type ladder on both sides, O against O

`witness_corpus(mode)` gives (queries, candidates) for the score rows of the whole-tree SPR searches (the witness filter of
maple_amd/csrc/witness.hip and the dense kernel's bitmap form), in the modes without an error model, one family per arm of the
filter's eligibility and range rules and per boundary of its bucket and bitmap arithmetic:

  wit_sites          candidates whose only eligible entry is at site 1, 2, lRef - 1 or lRef; queries with every kind of entry there
  wit_rarest         several eligible entries per candidate, common and rare ones, ties in rarity
  wit_none           candidates without an eligible entry (stored lengths, O vectors, N, R only) and slots without a list (None)
  wit_query_extremes N everywhere, tail-less R everywhere, more than 512 entries, an N run over hundreds of buckets
  wit_rootframe      lists passed upwards through a reference branch by the oracle, on both sides
  wit_random         rich random lists, queries with little coverage, candidates' own lists as queries

`witness_may_exclude` states the filter's rule on the tuple grammar; `oracle_rows` gives the oracle's score of every pair.
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


def sink_case(name, k0, bk0, tipk0, k1, b1, tip1, pas, b2, tip2, expect=None):
    """A five-node tree root -> (c1 -> (k0, k1), c2) as its three lists: lower[k0], lower[k1] = pv1 and lower[c2] = pv2, which c1
    is handed from above over b2 = dist[c1] + dist[c2].  expect: per side what becomes of rooting above it."""
    return dict(k0=k0, bk0=float(bk0), tipk0=bool(tipk0), pv1=k1, b1=float(b1), tip1=bool(tip1), pv2=pas, b2=float(b2), tip2=bool(tip2),
                returnLK=True, isUpDown=False, name=name, expect=expect)


def fam_sink_flag(rng, ref, u, n=4):
    """Error models only.  lower[k1] and lower[c2] are N over a stretch, so upVect is; lower[k0] alternates single-site R runs and
    nucleotides there.  Rooting above k0 merges N with them: as a tip's they come out as (type, pos, d / 2, True) (even cases), as a
    non-tip's with stored lengths they keep their own flags, some of them False (odd cases).  Rooting above k1 first puts the
    flags into upVect and then merges that with N.  Behind the stretch all three lists differ site by site."""
    assert u
    out = []
    L = len(ref)
    for k in range(n):
        s = [1300, 1100, 1400, 1200][k % 4]
        k1 = Builder(ref, u).run(5, 1, s)
        pas = Builder(ref, u).run(5, 1, s + 20)
        for p in range(s + 25, L - 2, 5):
            k1.nuc(p, other(rng, int(ref[p - 1])))
            pas.nuc(p + 1, other(rng, int(ref[p])), d0=(1e-4 if p % 2 else None), flag=False)
        b = Builder(ref, u)
        tip = k % 2 == 0
        for p in range(2, L - 1, 2):
            if tip:
                b.nuc(p, other(rng, int(ref[p - 1])))
            else:
                fl = bool(p % 16 != 0)
                b.run(4, p - 1, p - 1, d0=1e-4, flag=fl)
                b.nuc(p, other(rng, int(ref[p - 1])), d0=(0.0 if p % 3 else 2e-5), flag=bool(p % 10 != 0))
        out.append(sink_case(("sink_flag", k), b.done(), [1e-4, 2e-5][k % 2], tip, k1.done(), [2e-4, 1e-5][k // 2 % 2], False,
                             pas.done(), [1e-4, 3e-4][k % 2], bool(k == 3)))
    return out


def fam_sink_abandon(rng, ref, u):
    """One tree per place of abandonment.  Every side is a non-tip.  Two nodes that show different nucleotides at a site over a total
    length of 0 have no merge (M:4757-4762); over 1e-170 they multiply the running factor by about 1e-170, and the second such
    site of ONE merge takes it below DBL_MIN (fam_merge_underflow).  Rooting above k0 merges k1 with what comes from above (pas)
    and the result with k0; rooting above k1 merges k0 with pas and the result with k1; c1 merges k0 with k1 and the root pas with
    c1 -- those two must succeed.  x, y, z are three nucleotides other than the reference's, `-` is N, R the reference:
        name                 site: k0 k1 pas     lengths k0, k1, pas     above k0          above k1
        up_none              s:    R  x  y       1e-4    0     0         upVect None       new root None
        new_none             s:    z  -  y       0       1e-4  0         new root None     upVect None
        up_underflow         s, t: R  x  y       1e-4    tiny  tiny      upVect underflows new root underflows
        new_underflow        s, t: z  -  y       tiny    1e-4  tiny      new root underfl. upVect underflows
        sibling_scored_up    s:    x  x  y       tiny    tiny  tiny      upVect underflows scored (one tiny factor per merge)
                             t:    y  x  y
        sibling_scored_new   s:    z  -  y       tiny    tiny  tiny      new root underfl. scored
                             t:    z  y  -
    A few sites where all three agree on a nucleotide keep the lists from being empty elsewhere."""
    out = []
    L = len(ref)
    tiny = 1e-170
    specs = [("up_none", ["Rxy"], (1e-4, 0.0, 0.0), ("up_none", "new_none")),
             ("new_none", ["z-y"], (0.0, 1e-4, 0.0), ("new_none", "up_none")),
             ("up_underflow", ["Rxy", "Rxy"], (1e-4, tiny, tiny), ("up_underflow", "new_underflow")),
             ("new_underflow", ["z-y", "z-y"], (tiny, 1e-4, tiny), ("new_underflow", "up_underflow")),
             ("sibling_scored_up", ["xxy", "yxy"], (tiny, tiny, tiny), ("up_underflow", "scored")),
             ("sibling_scored_new", ["z-y", "zy-"], (tiny, tiny, tiny), ("new_underflow", "scored"))]
    for name, cols, (bk0, b1, b2), expect in specs:
        ps = sorted(int(p) for p in rng.choice(np.arange(10, L - 10, 3), size=len(cols) + 6, replace=False))
        special = [ps[2], ps[5]][:len(cols)]
        bs = [Builder(ref, u) for _ in range(3)]
        for p in ps:
            r = int(ref[p - 1])
            x = other(rng, r)
            y = other(rng, r, (x,))
            z = other(rng, r, (x, y))
            if p in special:
                for b, ch in zip(bs, cols[special.index(p)]):
                    if ch == "-":
                        b.run(5, p, p)
                    elif ch != "R":
                        b.nuc(p, dict(x=x, y=y, z=z)[ch])
            else:                                                  # all three agree
                for b in bs:
                    b.nuc(p, x)
        out.append(sink_case(("sink_abandon", name), bs[0].done(), bk0, False, bs[1].done(), b1, False, bs[2].done(), b2, False,
                             expect=dict(k0=expect[0], k1=expect[1])))
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
    if u:                                                          # (the sink families come last: the others' draws stay as they were)
        fams["sink_flag"] = fam_sink_flag(rng, ref, u)
    fams["sink_abandon"] = fam_sink_abandon(rng, ref, u)
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


# ---- the structural operators ---------------------------------------------------------------------------------------------
THR = 1e-8                                                        # thresholdProb of the devices and oracles the tests make


def tail_forms(u):
    """The tail forms of the grammar as (d1?, flag) choices: a tail is (d0,) or (d0, d1), plus the flag under an error model."""
    return [(False, False), (True, False)] + ([(False, True), (True, True)] if u else [])


def prefix_sites(b, rng, k):
    """k adjacent single-site entries at positions 1..k: the next entry is entry number k of the list."""
    for p in range(1, k + 1):
        b.nuc(p, other(rng, int(b.ref[p - 1])))
    return b


def fam_shorten_runs(rng, ref, u):
    out = []
    a = 1e-4
    heads = {"far": (a, a + 0.8 * THR, a + 1.6 * THR),            # the third is within THR of its neighbour, not of the head
             "back": (a, a + 0.8 * THR, a),                       # all within THR of the head
             "swing": (a, a + 0.8 * THR, a - 0.8 * THR)}          # the third is outside THR of its neighbour, within of the head
    for lead in (0, 5, 62, 63, 64, 126, 127):                     # entries in front of the run: it straddles entry 64 / 128
        for (has1, flag) in tail_forms(u):
            for name, ds in heads.items():
                for on_d1 in ((False, True) if has1 else (False,)):
                    b = prefix_sites(Builder(ref, u), rng, lead)
                    for k, d in enumerate(ds):
                        d0, d1 = (3e-4, d) if on_d1 else (d, (2e-4 if has1 else None))
                        b.run(4, lead + 1 + 2 * k, lead + 2 + 2 * k, d0=d0, d1=d1, flag=flag)
                    b.nuc(lead + 9, other(rng, int(ref[lead + 8])))
                    out.append(dict(vec=b.done(), name=("head", lead, has1, flag, name, on_d1)))
    if u:                                                         # refused on the flag alone, in the middle and at the head
        for lead in (3, 63):
            for has1 in (False, True):
                for flags in ((False, True, False), (True, True, False), (False, False, False)):
                    b = prefix_sites(Builder(ref, u), rng, lead)
                    for k, f in enumerate(flags):
                        b.run(4, lead + 1 + k, lead + 1 + k, d0=1e-4, d1=(2e-4 if has1 else None), flag=f)
                    out.append(dict(vec=b.done(), name=("flag", lead, has1, flags)))
    # tail-less runs, runs whose neighbours differ in form, and lists that shorten leaves alone
    b = Builder(ref, u).run(4, 1, 10).run(4, 11, 20).run(4, 21, 30, d0=1e-4).run(4, 31, 40, d0=1e-4, d1=1e-4).run(4, 41, 50)
    out.append(dict(vec=b.run(5, 51, 60).run(4, 61, 70).run(4, 71, 80).done(), name="forms"))
    out.append(dict(vec=[(4, len(ref))], name="all_R"))
    out.append(dict(vec=Builder(ref, u).run(4, 1, 700).done(), name="two_R"))
    for k in range(6):
        out.append(dict(vec=random_list(rng, ref, u, int(rng.integers(5, 90))), name="tip"))
    # long runs with drifting lengths: every entry is within THR of its neighbour, the head moves on when the drift passes THR
    for n_run, step in ((40, 0.3), (150, 0.15), (600, 0.4)):      # (600 entries: more than the wavefront form stages)
        for (has1, flag) in tail_forms(u)[:2 if n_run == 600 else None]:
            b = Builder(ref, u)
            for k in range(n_run):
                b.run(4, 2 * k + 1, 2 * k + 2, d0=a + k * step * THR, d1=(5e-4 if has1 else None), flag=flag and k % 50 != 49)
            out.append(dict(vec=b.done(), name=("drift", n_run, has1, flag)))
    return out


def rich_list(rng, ref, u, mean_gap, d1=True, flags=True, n_runs=True):
    """A list with every kind of entry: nucleotides and O vectors with and without tails, N runs, R runs with tails, some of
    them adjacent.  d1=False gives the grammar of a lower list (no second length)."""
    L = len(ref)
    b = Builder(ref, u)
    p = 1
    while True:
        p += int(rng.choice([0, 0, 1, int(rng.integers(1, 2 * mean_gap))]))
        if p > L - 45:
            break
        kind = int(rng.integers(0, 6 if n_runs else 5))
        d0 = [None, 0.0, 1e-5, 3e-4][int(rng.integers(0, 4))]
        if kind in (3, 4) and d0 is None:
            d0 = 2e-5                                             # (no tail-less R run next to another: shorten would join them)
        dd1 = float(rng.choice([1e-5, 2e-4])) if (d1 and d0 is not None and rng.random() < 0.5) else None
        fl = bool(flags and rng.random() < 0.5)
        if kind in (0, 1):
            b.nuc(p, other(rng, int(ref[p - 1])), d0=d0, d1=dd1, flag=fl)
        elif kind == 2:
            b.o(p, rng.dirichlet([1.0] * 4), d0=d0)
        elif kind in (3, 4):
            end = p + int(rng.integers(0, 30))
            b.run(4, p, end, d0=d0, d1=dd1, flag=fl)
            p = end
        else:
            end = p + int(rng.integers(0, 40))
            b.run(5, p, end)
            p = end
        p += 1
    return b.done()


def sites_of(gl):
    """[(position, entry)] of the single-site entries of a list."""
    out, pos = [], 0
    for e in gl:
        if e[0] in (4, 5):
            pos = e[1]
        else:
            pos += 1
            out.append((pos, e))
    return out


def mutation(ref, p, up, other_nuc):
    """(pos, from, to) of a branch whose frame on the list's side has the reference nucleotide at p."""
    r = int(ref[p - 1])
    return (p, other_nuc, r) if up else (p, r, other_nuc)


def fam_pass_edges(rng, ref, u):
    L = len(ref)
    r = lambda p: int(ref[p - 1])                              # noqa: E731
    out = []
    for up in (False, True):
        mut = lambda p, x=None: mutation(ref, p, up, other(rng, r(p)) if x is None else x)      # noqa: E731
        add = lambda name, pv, ms: out.append(dict(pv=pv, mutations=sorted(ms), dirIsUp=up, name=(name, up)))  # noqa: E731
        add("ends_all_R", [(4, L)], [mut(1), mut(L)])
        add("ends_sites", Builder(ref, u).nuc(1, other(rng, r(1))).o(L, rng.dirichlet([1.0] * 4), d0=1e-4).done(), [mut(1), mut(L)])
        add("ends_N", Builder(ref, u).run(5, 1, 3).run(5, L - 2, L).done(), [mut(1), mut(L)])
        add("one_at_1", [(4, L)], [mut(1)])
        add("one_at_lRef", Builder(ref, u).run(4, 1, 10, d0=1e-4).done(), [mut(L)])
        for (has1, flag) in [(None, False)] + tail_forms(u):
            tail = dict() if has1 is None else dict(d0=1e-4, d1=(2e-4 if has1 else None), flag=flag)
            run = lambda: Builder(ref, u).nuc(99, other(rng, r(99))).run(4, 100, 140, **tail).nuc(141, other(rng, r(141)))  # noqa: E731
            add(("R_first", has1, flag), run().done(), [mut(100)])
            add(("R_last", has1, flag), run().done(), [mut(140)])
            add(("R_first_last", has1, flag), run().done(), [mut(100), mut(140)])
            add(("R_adjacent", has1, flag), run().done(), [mut(110), mut(111), mut(113)])
            add(("R_all", has1, flag), run().done(), [mut(p) for p in range(100, 141)])
            add(("R_many", has1, flag), run().done(), [mut(p) for p in (100, 101, 102, 120, 139, 140)])
            add(("R_single_site", has1, flag), Builder(ref, u).run(4, 200, 200, **tail).run(4, 201, 201, d0=5e-4, flag=False).done(),
                [mut(200), mut(201)])
        add("N_skip", Builder(ref, u).run(5, 50, 60).run(5, 300, 400).run(5, L - 20, L).done(),
            [mut(55)] + [mut(p) for p in (300, 301, 350, 400)] + [mut(L - 20), mut(L)])
        add("N_edges", Builder(ref, u).run(5, 50, 60).done(), [mut(49), mut(50), mut(60), mut(61)])
        for (has1, flag) in [(None, False)] + tail_forms(u):
            tail = dict() if has1 is None else dict(d0=1e-4, d1=(2e-4 if has1 else None), flag=flag)
            x, y = other(rng, r(500)), other(rng, r(502))
            b = Builder(ref, u).nuc(500, x, **tail).nuc(501, other(rng, r(501)), **tail).nuc(502, y, **tail)
            add(("nuc", has1, flag), b.done(), [mut(500, x), mut(502, other(rng, r(502), (y,)))])
        add("O", Builder(ref, u).o(600, rng.dirichlet([1.0] * 4)).o(601, rng.dirichlet([1.0] * 4), d0=2e-4).o(602, rng.dirichlet([1.0] * 4)).done(),
            [mut(600), mut(601)])
    return out


def fam_pass_random(rng, ref, u, n=24):
    """Rich lists of more than 64 entries; half of the mutations fall on the lists' own single-site entries, and half of
    those turn the nucleotide into the new reference."""
    L = len(ref)
    out = []
    for k in range(n):
        pv = rich_list(rng, ref, u, mean_gap=[6, 10, 25][k % 3])
        up = bool(k % 2)
        n_mut = [1, 2, 40, 70, 12, 3][k % 6]
        own = sites_of(pv)
        ms = {}
        for j in rng.permutation(len(own))[: n_mut // 2]:
            p, e = own[int(j)]
            x = e[0] if (e[0] < 4 and rng.random() < 0.5) else other(rng, int(ref[p - 1]))
            ms[p] = mutation(ref, p, up, x)
        while len(ms) < n_mut:
            p = int(rng.integers(1, L + 1))
            ms.setdefault(p, mutation(ref, p, up, other(rng, int(ref[p - 1]))))
        out.append(dict(pv=pv, mutations=[ms[p] for p in sorted(ms)], dirIsUp=up, name=("random", k)))
    return out


def o_pair(rng, x, y, at):
    """Two normalised vectors whose component `at` is x and y; the other three share 1 - x and 1 - y in the same proportions."""
    w = rng.dirichlet([1.0, 1.0, 1.0])
    mk = lambda z: [z if i == at else float(w[i - (i > at)] * (1.0 - z)) for i in range(4)]    # noqa: E731
    return mk(x), mk(y)


# one O component against another under the device defaults (thresholdProb 1e-8, thresholdDiffForUpdate 1e-5,
# thresholdFoldChangeUpdate 1.01): (x, y, different?)
WINDOW = [(1e-6, 4e-6, True),          # fold change, by the first quotient only
          (4e-6, 1e-6, True),          # ... by the second quotient only
          (4e-6, 6e-6, False),         # inside the window, both quotients small
          (1e-6, 1.005e-6, False),     # difference <= thresholdProb
          (0.0, 1e-9, True),           # a zero component
          (1e-9, 0.0, True),
          (0.3, 0.30002, True),        # above thresholdDiffForUpdate
          (0.3, 0.300009, False),      # below it, quotients small
          (2e-8, 5e-8, True),          # just above thresholdProb, first quotient
          (5e-8, 2e-8, True)]


def replace_entry(gl, k, e):
    return gl[:k] + [e] + gl[k + 1:]


def fam_differ_edges(rng, ref, u):
    out = []
    base = rich_list(rng, ref, u, mean_gap=12)
    add = lambda name, a, b, expect=None: out.append(dict(pv1=a, pv2=b, name=name, expect=expect))  # noqa: E731
    add("equal", base, list(base), False)
    for s_at in (3, 700, 1400):                                    # an O entry early, in the middle and late in the walk
        for at in range(4):
            for (x, y, diff) in WINDOW:
                if s_at != 700 and at != 1:
                    continue
                v1, v2 = o_pair(rng, x, y, at)
                d0 = None if at % 2 else 1e-4
                n1 = other(rng, int(ref[s_at - 2]))
                a = Builder(ref, u).nuc(s_at - 1, n1).o(s_at, v1, d0=d0).done()
                b = Builder(ref, u).nuc(s_at - 1, n1).o(s_at, v2, d0=d0).done()
                add(("window", s_at, at, x, y), a, b, diff)
    # one entry of the base list changed in one place
    idx = {}
    for k, e in enumerate(base):
        kind = (e[0] if e[0] >= 4 else 0, len(e))
        idx.setdefault(kind, []).append(k)
    for kind, ks in sorted(idx.items()):
        for k in ks[:2]:
            e = base[k]
            t = e[0]
            if t == 6:
                if len(e) == 4:
                    add(("O_d0_far", k), base, replace_entry(base, k, (6, e[1], e[2] + 2 * THR, e[3])), True)
                    add(("O_d0_near", k), base, replace_entry(base, k, (6, e[1], e[2] + 0.5 * THR, e[3])), False)
                    add(("O_len", k), base, replace_entry(base, k, (6, e[1], e[3])), True)
                else:
                    add(("O_len", k), base, replace_entry(base, k, (6, e[1], 1e-4, e[2])), True)
                add(("O_to_nuc", k), base, replace_entry(base, k, (other(rng, e[1]), e[1])), True)
                continue
            if t == 5:
                add(("N_to_R", k), base, replace_entry(base, k, (4, e[1])), True)
                continue
            if len(e) == 2:
                add(("bare_to_tail", k), base, replace_entry(base, k, (t, e[1], 1e-4) + ((False,) if u else ())), True)
                if t < 4:
                    add(("nuc_type", k), base, replace_entry(base, k, (other(rng, e[1], (t,)), e[1])), True)
                continue
            add(("d0_far", k), base, replace_entry(base, k, e[:2] + (e[2] + 2 * THR,) + e[3:]), True)
            add(("d0_near", k), base, replace_entry(base, k, e[:2] + (e[2] + 0.5 * THR,) + e[3:]), False)
            if len(e) == 4 + u:
                add(("d1_far", k), base, replace_entry(base, k, e[:3] + (e[3] - 2 * THR,) + e[4:]), True)
                add(("d1_near", k), base, replace_entry(base, k, e[:3] + (e[3] + 0.5 * THR,) + e[4:]), False)
                add(("len", k), base, replace_entry(base, k, e[:3] + e[4:]), True)
            if u:
                add(("flag", k), base, replace_entry(base, k, e[:-1] + (not e[-1],)), True)
    # an R run cut in two: the same sites, other entries
    k = next(k for k, e in enumerate(base) if e[0] == 4 and len(e) == 2 and e[1] - (base[k - 1][1] if k and base[k - 1][0] in (4, 5) else 0) > 3)
    add("run_cut", base, base[:k] + [(5, base[k][1] - 2), base[k]] + base[k + 1:], True)
    # two long lists (more than the wavefront form stages) that differ in their last entry only
    a = prefix_sites(Builder(ref, u), rng, 600).done()
    add("long_equal", a, list(a), False)
    add("long_last", a, a[:-1] + [(5, len(ref))], True)
    return out


def path_mutations(rng, ref, n_branches, n_mut):
    """Mutation lists of n_branches branches on the way up from a node whose frame is `ref`, at distinct positions."""
    L = len(ref)
    ps = rng.choice(np.arange(1, L + 1), size=n_branches * n_mut, replace=False)
    out = []
    for k in range(n_branches):
        out.append(sorted(mutation(ref, int(p), True, other(rng, int(ref[int(p) - 1]))) for p in ps[k * n_mut:(k + 1) * n_mut]))
    return out


def fam_rootvec(rng, ref, u, n=30):
    out = []
    L = len(ref)
    for k in range(n):
        pv = rich_list(rng, ref, u, mean_gap=[8, 30][k % 2], d1=False)
        if k % 5 == 0:                                             # O entries with a length of 0.0 of their own, at both ends
            pv = Builder(ref, u).o(1, rng.dirichlet([1.0] * 4), d0=0.0).o(2, rng.dirichlet([1.0] * 4)).o(L, rng.dirichlet([1.0] * 4), d0=0.0).done()
        n_br = [0, 1, 3][k % 3]
        path = path_mutations(rng, ref, n_br, [1, 5, 20][(k // 3) % 3]) if n_br else []
        if n_br and k % 4 == 0:                                    # mutations on the list's own sites, and a branch without any
            taken = {m[0] for br in path for m in br}
            own = [p for p, e in sites_of(pv) if p not in taken][:6]
            path[0] = sorted(path[0] + [mutation(ref, p, True, other(rng, int(ref[p - 1]))) for p in own])
            path.insert(1, [])
        out.append(dict(pv=pv, bLen=[0.0, 1e-4][(k // 2) % 2], isFromTip=bool((k // 4) % 2), path=path, name=("rootvec", k)))
    return out


def fam_rootprob(rng, ref, u, n=24):
    out = []
    L = len(ref)
    for k in range(n):
        out.append(dict(pv=rich_list(rng, ref, u, mean_gap=[4, 10, 40][k % 3], d1=False), name=("rich", k)))
    for k in range(4):                                             # several hundred O entries heavy on the rarest nucleotides:
        b = Builder(ref, u)                                        # each factor is about 0.2, the product is carried over
        for p in range(3, 3 + 2 * [420, 700][k % 2], 2):
            v = rng.dirichlet([1.0] * 4) * 0.02
            v[1] += 0.49
            v[2] += 0.49
            b.o(p, v, d0=(1e-4 if p % 3 == 0 else None))
        out.append(dict(pv=b.done(), name=("carry_O", k)))
    if u:                                                          # the same with flagged nucleotides and flagged runs between them
        for k in range(2):
            b = Builder(ref, u)
            for p in range(2, L - 1, 2):
                b.run(4, p - 1, p - 1, d0=1e-4, flag=True)
                b.nuc(p, other(rng, int(ref[p - 1])), d0=0.0, flag=True)
            out.append(dict(pv=b.done(), name=("carry_flag", k)))
        out.append(dict(pv=Builder(ref, u).run(4, 1, L, d0=1e-4, flag=True).done(), name="all_flagged_R"))
    out.append(dict(pv=[(4, L)], name="all_R"))
    out.append(dict(pv=[(5, L)], name="all_N"))
    return out


def tip_list(rng, ref, u, n_sites, n_n, n_o):
    """A sample's list: nucleotides, N runs and ambiguity vectors, no lengths."""
    L = len(ref)
    b = Builder(ref, u)
    starts = np.sort(rng.choice(np.arange(1, L - 40, 45), size=n_sites + n_n + n_o, replace=False))
    kinds = rng.permutation([0] * n_sites + [1] * n_n + [2] * n_o)
    for p, kd in zip(starts, kinds):
        p = int(p) + int(rng.integers(0, 3))
        if kd == 0:
            b.nuc(p, other(rng, int(ref[p - 1])))
        elif kd == 1:
            b.run(5, p, p + int(rng.integers(0, 30)))
        else:
            v = [0.0] * 4
            i, j = rng.choice(4, size=2, replace=False)
            v[int(i)] = v[int(j)] = 0.5
            b.o(p, v)
    return b.done()


def fam_minor(rng, ref, u, n=16):
    L = len(ref)
    r = lambda p: int(ref[p - 1])                              # noqa: E731
    out = []
    add = lambda name, a, b: out.append(dict(pv1=a, pv2=b, name=name))   # noqa: E731
    s = 400
    x = other(rng, r(s))
    y = other(rng, r(s), (x,))
    z = next(i for i in range(4) if i not in (x, y, r(s)))
    B = lambda: Builder(ref, u).nuc(100, other(np.random.default_rng(5), r(100)))    # noqa: E731
    vec = lambda *big: [0.5 if i in big else 0.0 for i in range(4)]       # noqa: E731
    shapes = {"R": B().done(), "N": B().run(5, s, s).done(), "N_run": B().run(5, s - 20, s + 20).done(), "x": B().nuc(s, x).done(),
              "y": B().nuc(s, y).done(), "O_xr": B().o(s, vec(x, r(s))).done(), "O_xy": B().o(s, vec(x, y)).done(),
              "O_yz": B().o(s, vec(y, z)).done(), "O_xr_again": B().o(s, vec(x, r(s))).done(),
              "O_soft": B().o(s, [0.85 if i == x else 0.05 for i in range(4)]).done(),
              "N_first": Builder(ref, u).run(5, 1, 30).done(), "N_last": B().run(5, L - 30, L).done(),
              "site_last": B().nuc(L, other(rng, r(L))).done(), "O_last": B().o(L, vec(r(L), other(rng, r(L)))).done()}
    for a in sorted(shapes):
        for b in sorted(shapes):
            add((a, b), shapes[a], shapes[b])
    # one side bigger early and the other late (the early exit), or only at the last site (the returns after the loop)
    add("both_bigger", B().run(5, 200, 210).done(), B().run(5, 900, 910).done())
    add("both_bigger_O", B().o(s, vec(x, y)).run(5, 900, 910).done(), B().nuc(s, x).done())
    for k in range(n):
        a = tip_list(rng, ref, u, int(rng.integers(2, 12)), int(rng.integers(0, 4)), int(rng.integers(0, 3)))
        bb = list(a)
        if k % 4:                                                  # b = a with some sites masked: a is at least as informative
            own = [(i, q) for i, (q, e) in zip([i for i, e in enumerate(a) if e[0] < 4 or e[0] == 6], sites_of(a))]
            for j in rng.permutation(len(own))[: 1 + k % 3]:
                i, q = own[int(j)]
                bb[i] = (5, q)
            bb = merge_n_runs(bb)
        add(("derived", k), a, bb)
        add(("random", k), a, tip_list(rng, ref, u, 3, 1, 1))
    return out


def merge_n_runs(gl):
    """Join adjacent N entries (a list never has two in a row)."""
    out = []
    for e in gl:
        if out and out[-1][0] == 5 and e[0] == 5:
            out[-1] = e
        else:
            out.append(e)
    return out


STRUCT_FAMILIES = ("shorten_runs", "pass_edges", "pass_random", "differ_edges", "rootvec", "rootprob", "minor")


def struct_corpus(mode):
    """{family: [case dict]} of the structural operators for a mode (the five standard modes)."""
    ref = reference()
    u = bool(model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(300 + MODES.index(mode))
    return {"shorten_runs": fam_shorten_runs(rng, ref, u), "pass_edges": fam_pass_edges(rng, ref, u),
            "pass_random": fam_pass_random(rng, ref, u), "differ_edges": fam_differ_edges(rng, ref, u),
            "rootvec": fam_rootvec(rng, ref, u), "rootprob": fam_rootprob(rng, ref, u), "minor": fam_minor(rng, ref, u)}


# ---- the score rows of the whole-tree searches (witness filter, maple_amd/csrc/witness.hip) --------------------------------
# Candidates look like probVectTotUp lists, queries like lower lists; no mode has an error model (the filter refuses one).
WITNESS_MODES = ("jc", "unrest", "ratevar", "zeroq")
WITNESS_FAMILIES = ("wit_sites", "wit_rarest", "wit_none", "wit_query_extremes", "wit_rootframe", "wit_random")
WIT_SITES = (1, 2, L_REF - 1, L_REF)                              # where wit_sites puts its candidates' only eligible entry


def assemble(ref, specs):
    """A list from (kind, first position, Builder arguments) in any order: kind is "nuc", "o" or "run"."""
    b = Builder(ref, False)
    for kind, p, kw in sorted(specs, key=lambda s: s[1]):
        if kind == "nuc":
            b.nuc(p, **kw)
        elif kind == "o":
            b.o(p, **kw)
        else:
            b.run(kw["typ"], p, kw["end"], d0=kw.get("d0"), d1=kw.get("d1"))
    return b.done()


def open_list(gl, rng):
    """Every R or nucleotide entry without a stored length, or with a stored 0.0, gets one above 0: no site of the list can be a
    zero-length mismatch."""
    out = []
    for e in gl:
        d = float(rng.choice([1e-5, 2e-4, 1e-3]))
        if e[0] <= 4 and len(e) == 2:
            e = e + (d,)
        elif e[0] <= 4 and e[2] == 0.0:
            e = e[:2] + (d,) + e[3:]
        out.append(e)
    return out


def windowed(gl, rng, n_win=3, width=120):
    """The list with N outside a few windows (a sample with little coverage)."""
    L = L_REF
    starts = np.sort(rng.choice(np.arange(2, L - width, width + 5), size=n_win, replace=False))
    keep = np.zeros(L + 2, dtype=bool)
    for a in starts:
        keep[int(a):int(a) + width] = True
    out, pos = [], 0
    for e in gl:
        end = e[1] if e[0] in (4, 5) else pos + 1
        p = pos + 1
        while p <= end:                                            # the entry cut into pieces inside and outside the windows
            q = p
            while q < end and keep[q + 1] == keep[p]:
                q += 1
            if not keep[p] or e[0] == 5:
                out.append((5, q))
            else:
                out.append(((e[0], q) + e[2:]) if e[0] == 4 else e)
            p = q + 1
        pos = end
    return merge_n_runs(out)


def lower_form(gl):
    """The list without second lengths (the grammar of a lower list)."""
    return [e[:3] if (e[0] <= 4 and len(e) == 4) else e for e in gl]


def fam_wit_sites(rng, ref):
    L = len(ref)
    qs, cs = [], []
    for i, s in enumerate(WIT_SITES):
        r = int(ref[s - 1])
        x = other(rng, r)
        y = other(rng, r, (x,))
        z = other(rng, r, (x, y))
        far = 700 + 10 * i                                         # (an entry that is not eligible, far from s)
        cs.append(assemble(ref, [("nuc", s, dict(nuc=x))]))
        cs.append(assemble(ref, [("nuc", s, dict(nuc=x)), ("nuc", far, dict(nuc=other(rng, int(ref[far - 1])), d0=1e-4, d1=2e-4))]))
        cs.append(assemble(ref, [("nuc", s, dict(nuc=y))]))
        cs.append(assemble(ref, [("nuc", s, dict(nuc=y)), ("o", far + 1, dict(vec=rng.dirichlet([1.0] * 4), d0=1e-4)),
                                 ("run", far + 3, dict(typ=5, end=far + 9))]))
        d = [1e-5, 2e-4, 1e-3, 3e-4][i]
        q = lambda *specs: qs.append(assemble(ref, list(specs)))   # noqa: E731
        mid = ("run", 3, dict(typ=5, end=L - 2))                   # (N between the four sites: the site alone decides)
        q(("nuc", s, dict(nuc=x)), mid)                            # the same nucleotide: walked, finite
        q(("nuc", s, dict(nuc=z)), mid)                            # another nucleotide: excluded
        if s < L:                                                  # tail-less R up to the site, lengths after it: excluded
            q(("run", 1, dict(typ=4, end=s)), ("run", s + 1, dict(typ=4, end=L, d0=d)))
        else:
            q(("run", 1, dict(typ=4, end=L)))
        if s > 1:                                                  # lengths up to the site, tail-less R from it on: excluded
            q(("run", 1, dict(typ=4, end=s - 1, d0=d)), ("run", s, dict(typ=4, end=L)))
        q(("run", 1, dict(typ=4, end=2, d0=d)), mid, ("run", L - 1, dict(typ=4, end=L, d0=d)))   # R with d0 > 0 over it: walked, finite
        q(("run", 1, dict(typ=4, end=2, d0=d, d1=2 * d)), mid, ("run", L - 1, dict(typ=4, end=L, d0=d, d1=2 * d)))   # ... with d0 and d1
        if s > 1:                                                  # an N run that ends one site before it: excluded
            q(("run", 1, dict(typ=5, end=s - 1)))
        if s < L:                                                  # ... that starts one site after it: excluded
            q(("run", s + 1, dict(typ=5, end=L)))
        q(("run", s, dict(typ=5, end=s)))                          # N on exactly the site: walked
        q(("o", s, dict(vec=o_vec(rng, x, 0.3))), mid)             # an O entry on it: walked
        q(("o", s, dict(vec=o_vec(rng, y, 0.0), d0=d)), mid)       # ... with a length, nothing for y
        q(("nuc", s, dict(nuc=z, d0=d)), mid)                      # another nucleotide with d0 > 0: walked, finite
        q(("nuc", s, dict(nuc=z, d0=0.0)), mid)                    # ... with a stored 0.0: walked, -inf
        q(("nuc", s, dict(nuc=x, d0=0.0)), mid)                    # the same with a stored 0.0
    return qs, cs


def fam_wit_rarest(rng, ref, n=48):
    """Candidates with eligible entries at three common sites (shared by most) and at a rare one (shared by one or two)."""
    L = len(ref)
    common = [(300, other(rng, int(ref[299]))), (600, other(rng, int(ref[599]))), (601, other(rng, int(ref[600])))]
    rare_of, nuc_at, cs, qs = [], {}, [], []
    for k in range(n):
        has = [True, k % 4 != 0, k % 2 == 0]
        if k >= n - 4:
            has = [True, True, False]                              # common entries only: the rarer of the two is the witness
            rare = []
        elif k % 6 == 5:                                           # two rare entries of its own: equally rare, the first is taken
            rare = [900 + 4 * k, 902 + 4 * k]
        else:
            rare = [900 + 4 * (k - k % 2 if (k // 2) % 2 == 0 else k)]      # (every other pair of candidates shares its rare entry)
        rare = [(p, nuc_at.setdefault(p, other(rng, int(ref[p - 1])))) for p in rare]
        rare_of.append(rare)
        specs = [("nuc", p, dict(nuc=x)) for (p, x), h in zip(common, has) if h] + [("nuc", p, dict(nuc=x)) for p, x in rare]
        if k % 5 == 0:                                             # (an entry that is not eligible in between)
            specs.append(("nuc", 450, dict(nuc=other(rng, int(ref[449])), d0=1e-4)))
        cs.append(assemble(ref, specs))
    com = [("nuc", p, dict(nuc=x)) for p, x in common]
    for k in (1, 2, 5, 6, 11, 12):
        mine = [("nuc", p, dict(nuc=x)) for p, x in rare_of[k]]
        qs.append(assemble(ref, mine + com[1:]))                   # agrees with the rare entry, tail-less R at site 300
        qs.append(assemble(ref, mine + com))                       # agrees with every entry
        qs.append(assemble(ref, list(com)))                        # contradicts the rare entry only
        qs.append(assemble(ref, mine + [("run", 250, dict(typ=5, end=650))]))          # N over the common sites
    qs.append(assemble(ref, [("run", 250, dict(typ=5, end=L - 100))]))
    qs.append(open_list(assemble(ref, com[:1]), rng))
    return qs, cs


def fam_wit_none(rng, ref):
    """Candidates without an eligible entry (bucket 0: every search walks them) and the slots without a list (None)."""
    L = len(ref)
    nuc = lambda p, **kw: ("nuc", p, dict(nuc=other(rng, int(ref[p - 1])), **kw))      # noqa: E731
    cs = [[(4, L)],
          assemble(ref, [nuc(1, d0=0.0), nuc(400, d0=0.0), nuc(L, d0=0.0)]),
          assemble(ref, [nuc(10, d0=0.0), nuc(11, d0=1e-4)]),
          assemble(ref, [nuc(2, d0=1e-4), nuc(800, d0=3e-4), nuc(L - 1, d0=1e-5)]),
          assemble(ref, [nuc(200, d0=2e-4), nuc(201, d0=2e-4)]),
          assemble(ref, [nuc(1, d0=0.0, d1=1e-4), nuc(L, d0=1e-4, d1=0.0)]),
          assemble(ref, [nuc(500, d0=1e-4, d1=2e-4), nuc(900, d0=1e-5, d1=1e-5)]),
          None,
          assemble(ref, [("o", 1, dict(vec=rng.dirichlet([1.0] * 4))), ("o", 640, dict(vec=rng.dirichlet([1.0] * 4), d0=1e-4)),
                         ("o", L, dict(vec=rng.dirichlet([1.0] * 4)))]),
          assemble(ref, [("o", p, dict(vec=rng.dirichlet([1.0] * 4))) for p in range(63, 67)]),
          [(5, L)],
          assemble(ref, [("run", 1, dict(typ=5, end=40)), ("run", 700, dict(typ=5, end=1100)), ("run", L, dict(typ=5, end=L))]),
          None,
          assemble(ref, [("run", 1, dict(typ=4, end=L, d0=1e-4, d1=2e-4))]),
          assemble(ref, [("run", 1, dict(typ=4, end=750, d0=0.0)), ("run", 751, dict(typ=4, end=L, d0=1e-4))]),
          None]
    qs = [random_list(rng, ref, False, n, tails=False) for n in (1, 4, 9)]             # no lengths: -inf against a tail-less R
    qs += [open_list(random_list(rng, ref, False, n, tails=False), rng) for n in (2, 7)]
    qs.append(assemble(ref, [nuc(1), nuc(L)]))
    qs.append(assemble(ref, [("run", 1, dict(typ=5, end=40)), nuc(41), ("run", 700, dict(typ=5, end=1100))]))
    qs.append(assemble(ref, [("o", 64, dict(vec=rng.dirichlet([1.0] * 4))), ("o", 640, dict(vec=rng.dirichlet([1.0] * 4), d0=2e-4))]))
    return qs, cs


def fam_wit_query_extremes(rng, ref):
    L = len(ref)
    many = [("nuc", p, dict(nuc=other(rng, int(ref[p - 1])), d0=(None if p % 3 else 1e-4))) for p in range(2, 602)]
    assert len(many) > 512
    qs = [[(5, L)],                                                # N everywhere: walks every candidate
          [(4, L)],                                                # tail-less R everywhere: walks bucket 0 only
          assemble(ref, many),
          assemble(ref, [("nuc", 50, dict(nuc=other(rng, int(ref[49])))), ("run", 100, dict(typ=5, end=1400))]),
          assemble(ref, [("run", 1, dict(typ=4, end=99, d0=1e-4)), ("run", 100, dict(typ=5, end=1400)),
                         ("run", 1401, dict(typ=4, end=L, d0=2e-4))])]
    return qs, []


def fam_wit_rootframe(mode):
    """The upward cases of struct_corpus's pass_edges / pass_random through the oracle's passGenomeListThroughBranch: lists with
    the entries a re-expression in an enclosing frame leaves behind (what lists_to_root_frame hands the filter), on both sides."""
    from oracle.oracle_py import Oracle
    o = Oracle(reference(), ROOT_FREQS)
    o.set_model(**model(mode))
    sc = struct_corpus(mode)
    cases = [c for f in ("pass_edges", "pass_random") for c in sc[f] if c["dirIsUp"]]
    res = [o.passGenomeListThroughBranch(c["pv"], c["mutations"], True) for c in cases]
    return res[1::3], res


def fam_wit_random(rng, ref, n=70):
    cs = [rich_list(rng, ref, False, mean_gap=[15, 40, 100][k % 3]) for k in range(n)]
    qs = [rich_list(rng, ref, False, mean_gap=[15, 40, 100][k % 3], d1=False) for k in range(8)]
    qs += [open_list(rich_list(rng, ref, False, mean_gap=[15, 40, 100][k % 3], d1=False), rng) for k in range(4)]
    qs += [windowed(open_list(rich_list(rng, ref, False, mean_gap=[8, 15, 40][k % 3], d1=False), rng), rng, *[(3, 120), (2, 40), (1, 25)][k % 3])
           for k in range(21)]
    qs += [lower_form(cs[k]) for k in range(1, n, 7)]              # a candidate's own list: agrees with each of its entries
    return qs, cs


_WIT_FAMILIES = {}


def witness_families(mode):
    """{family: (queries, candidates)} of a mode, built once (a candidate None is a slot without a list, id -1)."""
    if mode not in _WIT_FAMILIES:
        assert mode in WITNESS_MODES
        ref = reference()
        rng = np.random.default_rng(400 + MODES.index(mode))
        _WIT_FAMILIES[mode] = {"wit_sites": fam_wit_sites(rng, ref), "wit_rarest": fam_wit_rarest(rng, ref),
                               "wit_none": fam_wit_none(rng, ref), "wit_query_extremes": fam_wit_query_extremes(rng, ref),
                               "wit_rootframe": fam_wit_rootframe(mode), "wit_random": fam_wit_random(rng, ref)}
    return _WIT_FAMILIES[mode]


def witness_corpus(mode):
    """(queries, candidates): the families of witness_families(mode) one after the other, in the order of WITNESS_FAMILIES."""
    fams = witness_families(mode)
    return [q for f in WITNESS_FAMILIES for q in fams[f][0]], [c for f in WITNESS_FAMILIES for c in fams[f][1]]


def witness_family_ranges(mode):
    """{family: (range of its queries, range of its candidates)} within witness_corpus(mode)."""
    out, q0, c0 = {}, 0, 0
    for f in WITNESS_FAMILIES:
        qs, cs = witness_families(mode)[f]
        out[f] = (range(q0, q0 + len(qs)), range(c0, c0 + len(cs)))
        q0, c0 = q0 + len(qs), c0 + len(cs)
    return out


# The rule of witness.hip's header, stated on the tuple grammar (not the library's code): a candidate entry is ELIGIBLE if it is a
# nucleotide other than the reference's without a stored length; a search's list contradicts it if, at the entry's site, it holds
# another nucleotide or the reference, again without a stored length.  Over a removed branch of length 0 and without an error
# model appendProbNode of such a pair is -inf.
ARMS = ("N", "O", "lengths", "same_nucleotide", "other_nucleotide", "reference")
_ARM_N, _ARM_O, _ARM_LEN, _ARM_R = 5, 6, 7, 4


def witness_eligible(cand_list):
    """[(site, nucleotide)] of the eligible entries of a candidate list."""
    return [(p, e[0]) for p, e in sites_of(cand_list) if e[0] < 4 and len(e) == 2 and e[0] != e[1]]


def witness_arms(query_list, lengthless=lambda e: len(e) == 2):
    """Per site (index = position), what a search's list holds there: 0-3 a nucleotide without a stored length, 4 the reference
    without one, 5 N, 6 an O vector, 7 a nucleotide or the reference with lengths attached."""
    arm = np.zeros(L_REF + 1, dtype=np.int8)
    pos = 0
    for e in query_list:
        end = e[1] if e[0] in (4, 5) else pos + 1
        arm[pos + 1:end + 1] = _ARM_N if e[0] == 5 else _ARM_O if e[0] == 6 else (e[0] if lengthless(e) else _ARM_LEN)
        pos = end
    assert pos == L_REF
    return arm


_WIT_VIEWS = {}


def _wit_view(gl, fn):
    key = (id(gl), fn.__name__)
    if key not in _WIT_VIEWS:
        _WIT_VIEWS[key] = (gl, fn(gl))                            # (the list is kept: its id stays its own)
    return _WIT_VIEWS[key][1]


def witness_may_exclude(cand_list, query_list, counts=None):
    """May the pair be left out of the walk -- does ANY eligible entry of the candidate meet a contradicting entry of the search's
    list?  (The library picks one witness per candidate: what it excludes is a subset.)  counts, a dict, takes the arm of every
    eligible entry met ("no_eligible" for a candidate without one or a slot without a list)."""
    elig = _wit_view(cand_list, witness_eligible) if cand_list is not None else []
    arm = _wit_view(query_list, witness_arms)
    if counts is not None and not elig:
        counts["no_eligible"] = counts.get("no_eligible", 0) + 1
    excl = False
    for p, x in elig:
        a = int(arm[p])
        name = {_ARM_N: "N", _ARM_O: "O", _ARM_LEN: "lengths", _ARM_R: "reference"}.get(a, "same_nucleotide" if a == x else "other_nucleotide")
        if counts is not None:
            counts[name] = counts.get(name, 0) + 1
        excl = excl or name in ("other_nucleotide", "reference")
    return excl


def witness_matrix(queries, cands, counts=None):
    """witness_may_exclude of every pair: bool [len(queries), len(cands)]."""
    return np.array([[witness_may_exclude(c, q, counts) for c in cands] for q in queries], dtype=bool).reshape(len(queries), len(cands))


def oracle_rows(o, queries, cands, qTip, qBLen):
    """appendProbNode(candidate, query, qTip[q], qBLen[q]) of every pair by the oracle `o` (its model set): float64
    [len(queries), len(cands)], -inf in the column of a candidate None."""
    nQ, nC = len(queries), len(cands)
    have = [k for k, c in enumerate(cands) if c is not None]
    packed = o.pack_many([cands[k] for k in have] + list(queries))
    pi = np.tile(np.arange(len(have)), nQ)
    qi = np.repeat(np.arange(nQ), len(have))
    tip = np.broadcast_to(qTip, nQ)[qi]
    bl = np.broadcast_to(np.asarray(qBLen, dtype=np.float64), nQ)[qi]
    want = np.full((nQ, nC), -np.inf)
    want[:, have] = o.appendProbNode_batch(packed, pi, len(have) + qi, tip, bl).reshape(nQ, len(have))
    return want


# ---- the fused items of the list repair (k_update_items / k_update_items_wave of maple_amd/csrc/update.hip) -------------------------
# An item is (l1, b1, t1, l2, b2, t2, upDown, mode, old): mergeVectors, then by mode 0: shorten, areVectorsDifferent(new, old);
# 1: shorten; 2: areVectorsDifferent(old, unshortened new), shorten only if different.  Every item of the family runs in all three modes.
UPDATE_SIZES = (1, 63, 64, 65, 256, 257)                          # entries of an input list: around a chunk of lanes and the staging limit
UPDATE_MERGED = (64, 65, 128)                                     # entries of a merged list (and one of at least 449)
ALL_N = [(5, L_REF)]


def sized(ref, u, rng, n, first):
    """a list of exactly n entries: n - 1 adjacent single-site entries from position `first` on, then R to the end (n = 1: all R)"""
    b = Builder(ref, u)
    if first > 1 and n > 1:
        b.run(4, 1, first - 1)
        n -= 1
    for p in range(first, first + n - 1):
        b.nuc(p, other(rng, int(ref[p - 1])))
    out = b.done()
    return out


def tied_runs(ref, u, n_runs, width, second):
    """n_runs entries that all end at multiples of `width`: two such lists end every merge step at the same position (the tie rule
    of merge_path at every step, also at steps 63 / 64 and 127 / 128).  second: the other list, N and R runs in turn."""
    b = Builder(ref, u)
    for k in range(n_runs):
        s, e = k * width + 1, (k + 1) * width
        if second:
            b.run(5 if k % 3 == 1 else 4, s, e, d0=(2e-4 if k % 3 == 2 else None), flag=False)
        else:
            b.run(4, s, e, d0=1e-4 * (1 + k % 5), flag=bool(k % 2))
    return b.done()


def perturbed_copies(rng, new, u, limit=None):
    """[(name, threshold case?, copy of `new` changed in one place)] the way fam_differ_edges and the stop-rule test perturb: the
    type, the tuple length, d0, d1 and the flag of an entry, O components as in WINDOW.  limit: at most this many, taken evenly."""
    out = []
    seen = {}
    for k, e in enumerate(new):
        kind = (e[0] if e[0] >= 4 else 0, len(e))
        if seen.setdefault(kind, 0) >= 1:
            continue
        seen[kind] += 1
        t = e[0]
        if t == 6:
            vec = e[-1]
            i = int(np.argmin(vec))
            for (x, y, _) in WINDOW:
                moved = vec[i] * (y / x) if x > 0.0 else 0.0
                if moved == vec[i] or moved >= 1.0 or vec[i] >= 1.0:
                    continue
                scale = (1.0 - moved) / (1.0 - vec[i])
                out.append((("O", x, y), True, replace_entry(new, k, e[:-1] + ([moved if j == i else vec[j] * scale for j in range(4)],))))
            if len(e) == 4:
                out.append(("O_d0_far", False, replace_entry(new, k, (6, e[1], e[2] + 2 * THR, e[3]))))
                out.append(("O_d0_near", True, replace_entry(new, k, (6, e[1], e[2] + 0.5 * THR, e[3]))))
                out.append(("O_len", False, replace_entry(new, k, (6, e[1], e[3]))))
            out.append(("O_to_nuc", False, replace_entry(new, k, ((e[1] + 1) % 4, e[1]))))
        elif t == 5:
            out.append(("N_to_R", False, replace_entry(new, k, (4, e[1]))))
        elif len(e) == 2:
            out.append(("bare_to_tail", False, replace_entry(new, k, (t, e[1], 1e-4) + ((False,) if u else ()))))
            if t < 4:
                out.append(("nuc_type", False, replace_entry(new, k, (next(z for z in range(4) if z not in (t, e[1])), e[1]))))
        else:
            out.append(("d0_far", False, replace_entry(new, k, e[:2] + (e[2] + 2 * THR,) + e[3:])))
            out.append(("d0_near", True, replace_entry(new, k, e[:2] + (e[2] + 0.5 * THR,) + e[3:])))
            if len(e) == 4 + u:
                out.append(("d1_far", False, replace_entry(new, k, e[:3] + (e[3] + 2 * THR,) + e[4:])))
                out.append(("d1_near", True, replace_entry(new, k, e[:3] + (e[3] + 0.5 * THR,) + e[4:])))
                out.append(("len", False, replace_entry(new, k, e[:3] + e[4:])))
            if u:
                out.append(("flag", False, replace_entry(new, k, e[:-1] + (not e[-1],))))
    if limit is not None and len(out) > limit:
        out = [out[int(j)] for j in np.linspace(0, len(out) - 1, limit).round()]
    return out


def fam_update_items(mode, o):
    """(lists, items) of a mode for the oracle o (set to that mode).  items: dicts with i1, i2, iold (indices into lists; iold -1: no
    old list), b1, t1, b2, t2, ud, name = (pair name, form of old), threshold (the verdict hangs on a value within the thresholds
    of areVectorsDifferent), and the oracle's m (the merge, None if there is none) and s (shorten(m)).  Pairs come from the merge
    families and the skipping-form edges, from the shorten families merged with an all-N list (so that shorten after the merge has
    runs to absorb and to refuse: the run-head rule, the flag), and from lists built for the shapes the fused kernels cut their
    work along (the names starting with "shape")."""
    ref = reference()
    u = bool(model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(500 + MODES.index(mode))
    corp = corpus(mode)
    pairs = []                                                     # (name, pv1, b1, t1, pv2, b2, t2, ud)
    for fam in ("merge_updown", "merge_carry"):
        for k, c in enumerate(corp[fam]):
            pairs.append(((fam, k), c["pv1"], c["b1"], c["tip1"], c["pv2"], c["b2"], c["tip2"], c["isUpDown"]))
    longs = long_lists(rng, ref, u)
    for k in range(0, len(longs) - 1, 2):
        pairs.append((("long", k), longs[k], 1e-4, False, longs[k + 1], 2e-4, bool(k % 4 == 0), bool(k % 4 == 2)))
    edges = skip_edge_lists(rng, ref, u)
    names = sorted(edges)
    for i, a in enumerate(names):
        b = names[(i + 5) % len(names)]
        pairs.append((("skip", a, b), edges[a], 1e-4, False, edges[b], 3e-4, bool(i % 2), bool(i % 3 == 0)))
    for k in range(10):
        up_down = bool(k % 2)
        pairs.append((("rich", k), rich_list(rng, ref, u, [8, 20][k % 2], d1=up_down), 1e-4, False, rich_list(rng, ref, u, 15, d1=False), 2e-4,
                      False, up_down))
    for c in fam_shorten_runs(rng, ref, u):                        # shorten after the merge absorbs, or refuses on the head or the flag
        lower_form_ok = all(not (e[0] <= 4 and len(e) == 4 + u) for e in c["vec"])
        if len(c["vec"]) > 256:
            continue
        pairs.append((("shorten", c["name"]), c["vec"], 1e-4, False, ALL_N, 1e-4, False, not lower_form_ok))
    # -- the shapes
    for n1 in UPDATE_SIZES:
        for n2 in UPDATE_SIZES:
            pairs.append((("shape_sizes", n1, n2), sized(ref, u, rng, n1, 1), 1e-4, bool(n1 % 2), sized(ref, u, rng, n2, 700), 2e-4, bool(n2 % 2), False))
    for want in UPDATE_MERGED + (449,):                            # a merged list of exactly `want` entries (>= for the last)
        n1 = want // 2
        a, b = sized(ref, u, rng, n1, 1), sized(ref, u, rng, want - n1 + 1, 700)   # (n1 - 1 sites, R, n2 - 2 sites, R)
        pairs.append((("shape_merged", want), a, 1e-4, False, b, 1e-4, False, False))
    for n_old in (512, 513):                                       # the old list at the staging limit and past it (inputs of 256 / 257)
        a, b = sized(ref, u, rng, 256, 1), sized(ref, u, rng, n_old - 255, 700)
        pairs.append((("shape_old", n_old), a, 1e-4, False, b, 1e-4, False, False))
    pairs.append((("shape_ties", 140), tied_runs(ref, u, 140, 10, False), 1e-4, False, tied_runs(ref, u, 140, 10, True), 2e-4, False, False))
    pairs.append((("shape_ties_updown", 140), tied_runs(ref, u, 140, 10, False), 1e-4, False, tied_runs(ref, u, 140, 10, True), 2e-4, False, True))
    b = Builder(ref, u)                                            # one run absorbed across three chunks of 64 entries
    for k in range(150):
        b.run(4, 2 * k + 1, 2 * k + 2, d0=2e-4, flag=False)
    pairs.append((("shape_absorb_three_chunks",), b.done(), 1e-4, False, ALL_N, 1e-4, False, False))
    for lead in (61, 62, 63):                                      # O entries whose aux doubles straddle entry 64
        b = prefix_sites(Builder(ref, u), rng, lead)
        for p in range(lead + 1, lead + 5):
            b.o(p, rng.dirichlet([1.0] * 4), d0=(1e-4 if p % 2 else None))
        pairs.append((("shape_O_straddle", lead), b.done(), 1e-4, False, ALL_N, 1e-4, False, False))
    # two lists that show different nucleotides at no distance: no merge (-1), at the first, a middle and the last step of the
    # walk, and at two steps of one chunk of lanes
    for name, ps in (("first", (1,)), ("middle", (700,)), ("last", (L_REF,)), ("two_in_a_chunk", (10, 20))):
        a, b = Builder(ref, u), Builder(ref, u)
        for p in ps:
            r = int(ref[p - 1])
            x = other(rng, r)
            a.nuc(p, x)
            b.nuc(p, other(rng, r, (x,)))
        pairs.append((("shape_none", name), a.done(), 0.0, False, b.done(), 0.0, False, False))
    lists, items = [], []

    def put(gl):
        lists.append([tuple(e) for e in gl])
        return len(lists) - 1

    for (name, pv1, b1, t1, pv2, b2, t2, ud) in pairs:
        try:
            m = o.mergeVectors(pv1, b1, t1, pv2, b2, t2, isUpDown=ud)
        except RuntimeError:
            continue                                               # (a state the reference raises on: not this family's)
        i1, i2 = put(pv1), put(pv2)
        s = None if m is None else o.shorten(m)
        olds = [("absent", False, None)]
        if m is not None:
            few = 3 if name[0] in ("shape_sizes", "skip", "shorten") else 8
            olds.append(("own", False, s))
            olds += [(("moved",) + (nm if isinstance(nm, tuple) else (nm,)), thr, gl) for nm, thr, gl in perturbed_copies(rng, s, u, few)]
            if m != s:
                olds.append(("own_unshortened", False, m))
                olds += [(("moved_unshortened",) + (nm if isinstance(nm, tuple) else (nm,)), thr, gl)
                         for nm, thr, gl in perturbed_copies(rng, m, u, 3)]
        for form, thr, old in olds:
            items.append(dict(i1=i1, b1=float(b1), t1=bool(t1), i2=i2, b2=float(b2), t2=bool(t2), ud=bool(ud), iold=-1 if old is None else put(old),
                              name=(name, form), threshold=thr, m=m, s=s))
    return lists, items


def update_item_expect(o, it, old, mode):
    """(list or None, outNone, verdict) of an item in a mode, from the oracle alone"""
    m, s = it["m"], it["s"]
    if m is None:
        return None, True, True
    if mode == 0:
        return s, False, (True if old is None else o.areVectorsDifferent(s, old))
    if mode == 1:
        return s, False, True
    flag = True if old is None else o.areVectorsDifferent(old, m)
    return (s if flag else None), False, flag


def scaled(gl, f):
    """the list with every double multiplied by f"""
    def mul(x):
        if isinstance(x, list):
            return [z * f for z in x]
        return x * f if isinstance(x, float) else x
    return [e[:2] + tuple(mul(x) for x in e[2:]) for e in gl]


def verdict_stable(o, it, old, mode, rel=1e-9):
    """the oracle's verdict of a compared item is the same when every double of the new list moves by +-rel"""
    new = it["s"] if mode == 0 else it["m"]
    want = o.areVectorsDifferent(new, old) if mode == 0 else o.areVectorsDifferent(old, new)
    for f in (1.0 + rel, 1.0 - rel):
        moved = scaled(new, f)
        got = o.areVectorsDifferent(moved, old) if mode == 0 else o.areVectorsDifferent(old, moved)
        if got != want:
            return False
    return True


# ---- the items of the branch-length sweep's fused estimate kernels (k_sweep_estimate / k_sweep_estimate_wave, blen_sweep.hip) ----------
# An item is (upper list, mutation list of the branch or none, lower list, fromTipC): the upper list is passed downwards through the
# mutations into per-item scratch, then estimateBranchLengthWithDerivative runs on the two lists.
SWEEP_SEAM = (255, 256, 257, 258, 300)                            # entries of a passed upper list around the 256 the wavefront form stages
SWEEP_STEPS = (63, 64, 65, 129)                                   # steps of the walk around a round of 64 lanes
_ZERO_PARTNER = {fr: to for fr, to in ZERO_RATES}
_ZERO_PARTNER.update({to: fr for fr, to in ZERO_RATES})


def walk_steps(a, b):
    """the steps the estimate's walk takes over two lists: one per distinct position at which an entry of either ends"""
    ends = set()
    for gl in (a, b):
        pos = 0
        for e in gl:
            pos = e[1] if e[0] in (4, 5) else pos + 1
            ends.add(pos)
    return len(ends)


def entry_at(gl, p):
    """(entry, first site, last site) of the entry that covers site p"""
    pos = 0
    for e in gl:
        end = e[1] if e[0] in (4, 5) else pos + 1
        if p <= end:
            return e, pos + 1, end
        pos = end


def fam_sweep_items(mode, o):
    """(lists, mutation lists, items) of a mode for the oracle o (set to that mode), in the order the ONE batch has: shuffled with a
    fixed seed, with a block of ten mutation-carrying items of very different sizes in a row.  items: dicts with iup, imut (-1: no
    mutation list), ilow (indices), tip, name, and where the item is built for a size want_passed / want_low / want_steps.
    The lower list of an item with mutations is in the frame below the branch: built over the mutated reference, or (the cases taken
    from other families) passed downwards by the oracle.
      arms     every blen_none (zero-rate modes) and blen_tenth case and every fourth append_d1_O case: bare; with a mutation list
               away from every single-site entry; with one mutation ON such a site (the kind of the upper list's entry there --
               inside an R run, which it splits, on a run's first or last site, on a nucleotide, on an O vector -- is in `on`); under
               an error model with both values of fromTipC.  `rich`: upper lists with every kind of entry, half of the mutations on
               their own entries, half of those turning the nucleotide into the reference (standard modes).
      exits    no term at all (False); 1 / t terms only (nA = 0, nZeros > 0).  The third early exit, minA < 0 (M:5309-5310), is out
               of reach: every a_i is a quotient of sums of products of probabilities, lengths and off-diagonal rates, all >= 0
               (the one subtraction, M:5140 / 5264, takes 1.33333 * errorRate < 1 of a term it has just added).
      seam     a stored upper list of at most 256 entries whose passed form has 255, 256, 257, 258 and 300 (each mutation splits a
               tail-less R run in three), against a short lower list; lower lists of 256 and 257 entries against a short passed
               list; both long
      shapes   walks of 63, 64, 65 and 129 steps; 100 a_i terms; the same nucleotide on both sides (two c1 terms in one step) at
               steps 64 and 128, the last lanes of two rounds"""
    ref = reference()
    u = bool(model(mode).get("usingErrorRate"))
    zero = mode.startswith("zeroq")
    rng = np.random.default_rng(600 + MODES.index(mode))
    corp = corpus(mode)
    lists, muts, items = [], [], []

    def put(gl):
        lists.append([tuple(e) for e in gl])
        return len(lists) - 1

    def new_nuc(p, avoid=()):
        r = int(ref[p - 1])
        return other(rng, r, tuple(avoid) + ((_ZERO_PARTNER[r],) if zero else ()))

    def mutated(ms):
        ref2 = ref.copy()
        for (p, fr, to) in ms:
            assert int(ref[p - 1]) == fr
            ref2[p - 1] = to
        return ref2

    def add(name, up, ms, low, tip, reframe=False, **extra):
        ms = sorted(tuple(int(x) for x in m) for m in ms)
        if ms and reframe:
            low = o.passGenomeListThroughBranch(low, ms, False)
        imut = -1
        if ms:
            muts.append(ms)
            imut = len(muts) - 1
        items.append(dict(name=name, iup=put(up), imut=imut, ilow=put(low), tip=bool(tip), **extra))

    def away_sites(a, b, k):
        busy = [p for p, _ in sites_of(a) + sites_of(b)]
        free = [p for p in range(15, L_REF - 15, 11) if all(abs(p - q) > 12 for q in busy)]
        return sorted(int(p) for p in rng.choice(free, size=k, replace=False))

    # -- arms of the estimate
    base = [(("blen_none", k), c["P"], c["C"], c["fromTipC"]) for k, c in enumerate(corp.get("blen_none", []))]
    base += [(("blen_tenth", k), c["P"], c["C"], c["fromTipC"]) for k, c in enumerate(corp.get("blen_tenth", []))]
    base += [(("append_d1_O", k), c["P"], c["C"], c["isTipC"]) for k, c in enumerate(corp.get("append_d1_O", [])) if k % 4 == 0]
    for j, (name, P, Cl, tip) in enumerate(base):
        tips = (False, True) if (u and name[0] != "blen_none") else (tip,)
        for tp in tips:
            add((name, "bare", tp), P, [], Cl, tp)
            add((name, "away", tp), P, [mutation(ref, p, False, new_nuc(p)) for p in away_sites(P, Cl, 2 + j % 4)], Cl, tp, reframe=True)
        sites = sorted({p for p, _ in sites_of(P) + sites_of(Cl)})
        for p in sites[: 3]:
            e, first, last = entry_at(P, p)
            kind = {6: "O", 5: "N", 4: "R_inside" if first < p < last else "R_edge"}.get(e[0], "nuc")
            x = e[0] if (kind == "nuc" and (j + p) % 2 and not (zero and _ZERO_PARTNER[int(ref[p - 1])] == e[0])) else new_nuc(p)
            add((name, "on", p), P, [mutation(ref, p, False, x)], Cl, tips[-1], reframe=True, on=kind if x != e[0] else "nuc_to_R")
            if kind == "R_inside" and e[0] == 4:
                add((name, "on_edge", first), P, [mutation(ref, first, False, new_nuc(first))], Cl, tips[-1], reframe=True, on="R_edge")
    if not zero:
        for k in range(8):
            P, Cl = rich_list(rng, ref, u, [6, 10, 25][k % 3]), rich_list(rng, ref, u, 15, d1=False)
            own = sites_of(P)
            ms = {}
            for j in rng.permutation(len(own))[: 6]:
                p, e = own[int(j)]
                x = e[0] if (e[0] < 4 and rng.random() < 0.5) else other(rng, int(ref[p - 1]))
                ms[p] = mutation(ref, p, False, x)
            for p in rng.integers(1, L_REF + 1, size=[1, 30, 4][k % 3]):
                ms.setdefault(int(p), mutation(ref, int(p), False, other(rng, int(ref[int(p) - 1]))))
            kinds = sorted({"O" if e[0] == 6 else ("nuc_to_R" if ms[p][2] == e[0] else "nuc") for p, e in own if p in ms})
            add(("rich", k), P, [ms[p] for p in sorted(ms)], Cl, bool(k % 2), reframe=True, on_kinds=kinds)
    # -- early exits
    one = Builder(ref, u).nuc(400, new_nuc(400)).done()
    add(("exit", "no_terms"), [(4, L_REF)], [], [(4, L_REF)], False)
    add(("exit", "zeros_only"), [(4, L_REF)], [], one, False)
    ms = [mutation(ref, p, False, new_nuc(p)) for p in (100, 900)]
    b = Builder(mutated(ms), u)                                    # (below the branch both sides show the old reference nucleotide)
    for (p, fr, to) in ms:
        b.nuc(p, fr)
    add(("exit", "no_terms_passed"), [(4, L_REF)], ms, b.done(), False)
    add(("exit", "zeros_only_passed"), [(4, L_REF)], ms, Builder(mutated(ms), u).nuc(400, new_nuc(400)).done(), False)

    # -- the 256 seam
    def short_low(ref2, k=3):
        b = Builder(ref2, u)
        for p in (1200, 1230, 1260)[:k]:
            b.nuc(p, other(rng, int(ref2[p - 1]), (int(ref[p - 1]),) + ((_ZERO_PARTNER[int(ref2[p - 1])],) if zero else ())), d0=2e-4)
        return b.done()

    def splitting(n0, m):
        """m mutations inside the trailing R run of sized(n0), three sites apart: the passed list has n0 + 2 m entries"""
        return [mutation(ref, p, False, new_nuc(p)) for p in range(n0 + 10, n0 + 10 + 3 * m, 3)]

    for want, n0, m in ((255, 205, 25), (256, 206, 25), (257, 207, 25), (300, 250, 25), (256, 254, 1), (258, 256, 1), (257, 1, 128)):
        ms = splitting(n0, m)
        upper, lower = sized(ref, u, rng, n0, 1), short_low(mutated(ms))
        for tp in ((False, True) if u else (False,)):
            add(("seam_upper", want, n0, tp), upper, ms, lower, tp, want_passed=want, want_low=7)
    for n_low in (256, 257):
        ms = [mutation(ref, p, False, new_nuc(p)) for p in (20, 40, 60)]
        add(("seam_lower", n_low), sized(ref, u, rng, 3, 1), ms, sized(mutated(ms), u, rng, n_low, 700), False, want_passed=9, want_low=n_low)
        add(("seam_lower_bare", n_low), sized(ref, u, rng, 3, 1), [], sized(ref, u, rng, n_low, 700), False, want_passed=3, want_low=n_low)
    ms = splitting(250, 25)
    add(("seam_both", 300, 257), sized(ref, u, rng, 250, 1), ms, sized(mutated(ms), u, rng, 257, 700), False, want_passed=300, want_low=257)
    # -- wave shapes
    for steps in SWEEP_STEPS:
        n1 = steps // 2
        add(("steps", steps), sized(ref, u, rng, n1, 1), [], sized(ref, u, rng, steps + 1 - n1, 700), False, want_steps=steps)
        ms = splitting(n1 - 4, 2)                                   # the same count with a pass in front
        add(("steps_passed", steps), sized(ref, u, rng, n1 - 4, 1), ms, sized(mutated(ms), u, rng, steps + 1 - n1, 700), False,
            want_steps=steps, want_passed=n1)
    b = Builder(ref, u)
    for p in range(300, 500, 2):
        b.nuc(p, new_nuc(p), d0=1e-4 * (1 + p % 7))
    add(("many_ais", 100), sized(ref, u, rng, 20, 1), [], b.done(), False, want_ais=100)
    P, Cb = Builder(ref, u), Builder(ref, u)
    for p in range(1, 129):
        x = new_nuc(p)
        P.nuc(p, x)
        if p in (64, 128):
            Cb.nuc(p, x)
    add(("two_c1_last_lane",), P.done(), [], Cb.done(), False, same_nuc_steps=(64, 128))
    # -- the batch's order: shuffled, then ten mutation-carrying items in a row, the largest scratch slices next to the smallest
    order = [int(k) for k in np.random.default_rng(7).permutation(len(items))]
    size = lambda it: len(lists[it["iup"]]) + 2 * len(muts[it["imut"]])                        # noqa: E731
    carrying = sorted((k for k in order if items[k]["imut"] >= 0), key=lambda k: size(items[k]))
    block = [k for pair in zip(carrying[-5:], carrying[:5]) for k in pair]
    rest = [k for k in order if k not in block]
    order = rest[: len(rest) // 2] + block + rest[len(rest) // 2:]
    return lists, muts, [items[k] for k in order]


def sweep_item_expect(o, lists, muts, it):
    """(passed upper list, the oracle's estimate: a length or False) of an item"""
    up = lists[it["iup"]]
    passed = o.passGenomeListThroughBranch(up, muts[it["imut"]], False) if it["imut"] >= 0 else up
    return passed, o.estimateBranchLengthWithDerivative(passed, lists[it["ilow"]], it["tip"])
