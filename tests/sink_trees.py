"""Small trees for the two tree-wide calls, maple_tree_log_lk and maple_tree_find_best_root, and an oracle twin of both calls.

A helper module like list_edges.py.  The twin works on tuple lists and calls nothing but the C oracle (oracle/oracle_py.py):

  oracle_tree_lk(o, tree)       calculateTreeLikelihood (M:9735-9779): (order, Lkcontribution per internal node of it, root term)
  oracle_root_scores(o, tree)   the scores of findBestRoot (M:7755-7848) for EVERY branch the search can reach: the recurrence
                                without the traversal's stop rules, without time trees and without the in-place shorten(upVect)
                                of M:7819 (shorten only follows a pass down through a mutation list, M:7844-7845).
                                {node: (score, (rootProbLK, lkRoot, lk, newLKtoRemove))}; a side whose upVect or whose new root's
                                merge is None or raises is absent, and nothing below it is visited (M:7838-7840).

Both read a node's STORED lower list (`tree.probVect`) and never recompute it, as the calls do.  `tree` is anything with the
columns root, up, children, dist, mutations, n_minor, probVect (a HostTree, or Columns below).  The children's merge of a visited
node (M:7797) and the root's own merge (M:7760) stand outside the reference's `try`: the twin asserts that they succeed.

The builders turn cases of the corpus (list_edges.corpus) into such trees:

  cherry_comb(o, pairs)         a caterpillar whose k-th backbone node carries a cherry (A_k, B_k) with the pair's two lists
  root_gadget(o, case, k0)      root -> (c1 -> (k0, k1), c2): lower[k1], lower[c2] = the case's pair, dist[c1] + dist[c2] its b2
                                exactly, so rooting above k0 makes the case's own merge (M:7804)
  caterpillar(o, sides)         the same shape with any number of leaves: upVect is handed down level after level
  grove(o, trees)               several trees under one balanced backbone: many items on one level

A side that is to be a non-tip is an internal node with two trivial leaves below it and its lower list assigned directly.  Lower
lists a case does not determine (c1, backbone nodes, the root) are what the oracle's mergeVectors gives for the children; where a
merge that the calls never make has none, the list is all N.
"""
import list_edges as le

L = le.L_REF
ALL_R = [(4, L)]
ALL_N = [(5, L)]


class Columns:
    """A tree as plain columns, built bottom up: add() takes the children that exist already."""

    def __init__(self):
        self.root = None
        self.up, self.children, self.dist, self.mutations, self.n_minor, self.probVect = [], [], [], [], [], []
        self.mark = {}

    @property
    def n(self):
        return len(self.up)

    def add(self, lower, dist=0.0, kids=(), n_minor=0):
        v = len(self.up)
        self.up.append(None)
        self.children.append(list(kids))
        self.dist.append(float(dist))
        self.mutations.append([])
        self.n_minor.append(int(n_minor))
        self.probVect.append([tuple(e) for e in lower])
        for c in kids:
            self.up[c] = v
        return v

    def side(self, lower, dist, tip, n_minor=0):
        """A leaf; as a non-tip a leaf with minor sequences (the reference's rule), or an internal node over two trivial leaves."""
        if tip or n_minor:
            return self.add(lower, dist, n_minor=0 if tip else n_minor)
        a, b = self.add(ALL_R, 1e-4), self.add(ALL_R, 2e-4)
        return self.add(lower, dist, kids=(a, b))

    def tips(self):
        return default_tip(self)

    def graft(self, other, dist):
        """other's nodes appended; returns the new id of its root, now hanging on a branch of length dist"""
        off = self.n
        for v in range(other.n):
            self.up.append(None if other.up[v] is None else other.up[v] + off)
            self.children.append([c + off for c in other.children[v]])
            self.dist.append(other.dist[v])
            self.mutations.append(list(other.mutations[v]))
            self.n_minor.append(other.n_minor[v])
            self.probVect.append(other.probVect[v])
        self.dist[other.root + off] = float(dist)
        return other.root + off

    def host_tree(self):
        from maple_amd.tree_host import HostTree
        none = [None] * self.n
        return HostTree(self.root, self.up, self.children, self.dist, self.mutations, self.n_minor, self.probVect, none, none, none)


def fixture_columns(f):
    """the tree of a search_* fixture"""
    t = f["tree"]
    c = Columns()
    c.root, c.up, c.children = t["root"], list(t["up"]), [list(x or []) for x in t["children"]]
    c.dist = [float(x or 0.0) for x in t["dist"]]
    c.mutations = [[tuple(m) for m in (ml or [])] for ml in t["mutations"]]
    c.n_minor = list(t["nMinor"])
    c.probVect = [None if gl is None else [tuple(e) for e in gl] for gl in t["probVect"]]
    return c


def default_tip(tree):
    """the reference's rule: no children and no minor sequences"""
    return [(not c) and (m == 0) for c, m in zip(tree.children, tree.n_minor)]


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
def _lower(tree, v):
    return [tuple(e) for e in tree.probVect[v]]


def _lower_up(o, tree, v):
    """the lower list as the parent reads it: through the node's own mutation list where it has one"""
    pv = _lower(tree, v)
    return o.passGenomeListThroughBranch(pv, tree.mutations[v], True) if tree.mutations[v] else pv


def _merge(o, a, da, ta, b, db, tb, na=0, nb=0):
    """mergeVectors(returnLK=True): (list, Lkcontribution), None, or RuntimeError where the reference raises"""
    return o.mergeVectors(a, float(da), bool(ta), b, float(db), bool(tb), returnLK=True, numMinor1=int(na), numMinor2=int(nb))


def _failure(o, a, da, ta, b, db, tb, na, nb):
    """Why a merge with returnLK gave nothing: "none" where the lists have no merge at all (different nucleotides at no distance,
    M:4753-4758: with returnLK the reference raises there too), "underflow" where only the running factor failed (M:4830-4837)."""
    res = o.mergeVectors(a, float(da), bool(ta), b, float(db), bool(tb), returnLK=False, numMinor1=int(na), numMinor2=int(nb))
    return "none" if res is None else "underflow"


def lk_order(tree):
    """internal nodes reachable from the root in the order the reference adds their contribution (M:9735-9770)"""
    order, stack = [], [(tree.root, False)]
    while stack:
        v, done = stack.pop()
        if not tree.children[v]:
            continue
        if done:
            order.append(v)
        else:
            stack += [(v, True), (tree.children[v][1], False), (tree.children[v][0], False)]
    return order


def oracle_tree_lk(o, tree, tip=None, known=None):
    """known: {node: Lkcontribution} the oracle has computed already from the same two lists, lengths, tip flags and counts"""
    tip = default_tip(tree) if tip is None else tip
    order = lk_order(tree)
    contrib = []
    for v in order:
        if known is not None and v in known:
            contrib.append(known[v])
            continue
        a, b = tree.children[v]
        res = _merge(o, _lower_up(o, tree, a), tree.dist[a], tip[a], _lower_up(o, tree, b), tree.dist[b], tip[b],
                     tree.n_minor[a], tree.n_minor[b])
        assert res is not None, f"node {v}: no merge of the children's lower lists (M:9762)"
        contrib.append(res[1])
    root = tree.root
    root_term = o.findProbRoot(_lower(tree, root), [tree.mutations[root]] if tree.mutations[root] else [])
    return order, contrib, root_term


def oracle_root_scores(o, tree, tip=None, why=None):
    """why: a dict that receives {node: "up_underflow" | "up_none" | "new_underflow" | "new_none"} for every abandoned side"""
    tip = default_tip(tree) if tip is None else tip
    ch, dist, mut, nm, up, root = tree.children, tree.dist, tree.mutations, tree.n_minor, tree.up, tree.root
    out = {}
    if not ch[root]:
        return out

    def path(v):
        p = []
        while v is not None:
            if mut[v]:
                p.append(mut[v])
            v = up[v]
        return p

    def given_up(v, reason):
        if why is not None:
            why[v] = reason

    c1, c2 = ch[root]
    v1, v2 = _lower_up(o, tree, c2), _lower_up(o, tree, c1)                # what child 1 sees from above is child 2's lower list
    original = o.findProbRoot(_lower(tree, root), path(root))
    res = _merge(o, v1, dist[c2], tip[c2], v2, dist[c1], tip[c1], nm[c2], nm[c1])
    assert res is not None, "the root's own merge has no result (M:7760)"
    original += res[1]
    if mut[c1]:
        v1 = o.passGenomeListThroughBranch(v1, mut[c1], False)
    if mut[c2]:
        v2 = o.passGenomeListThroughBranch(v2, mut[c2], False)
    stack = []
    if ch[c1]:
        stack.append((c1, v1, dist[c1] + dist[c2], tip[c2], nm[c2], original))
    if ch[c2]:
        stack.append((c2, v2, dist[c2] + dist[c1], tip[c1], nm[c1], original))
    while stack:
        t1, passed, distance, is_tip, n_min, rem = stack.pop()
        kids = ch[t1]
        pv = [_lower_up(o, tree, k) for k in kids]
        d, tp, nms = [dist[k] for k in kids], [tip[k] for k in kids], [nm[k] for k in kids]
        res = _merge(o, pv[0], d[0], tp[0], pv[1], d[1], tp[1], nms[0], nms[1])
        assert res is not None, f"node {t1}: no merge of the children's lower lists (M:7797)"
        new_rem = rem + res[1]
        for i in (0, 1):
            args = (pv[1 - i], d[1 - i], tp[1 - i], passed, distance, is_tip, nms[1 - i], n_min)
            try:
                res = _merge(o, *args)
            except RuntimeError:
                res = None
            if res is None:
                given_up(kids[i], "up_" + _failure(o, *args))
                continue
            up_vect, lk = res
            args = (up_vect, d[i] / 2, False, pv[i], d[i] / 2, tp[i], 0, nms[i])
            try:
                res = _merge(o, *args)
            except RuntimeError:
                res = None
            if res is None:
                given_up(kids[i], "new_" + _failure(o, *args))
                continue
            new_root, lk_root = res
            rp = o.findProbRoot(new_root, path(t1))
            score = rp + lk_root + lk - new_rem
            out[kids[i]] = (score, (rp, lk_root, lk, new_rem))
            if ch[kids[i]]:
                vect = up_vect
                if mut[kids[i]]:
                    vect = o.shorten(o.passGenomeListThroughBranch(up_vect, mut[kids[i]], False))
                stack.append((kids[i], vect, d[i], False, 0, new_rem - lk))
    return out


# ---- the builders -----------------------------------------------------------------------------------------------------------------
def merged_lk(o, a, da, ta, b, db, tb, na=0, nb=0):
    """(the merged list, its Lkcontribution), or None where the merge has none or raises"""
    try:
        return _merge(o, a, da, ta, b, db, tb, na, nb)
    except RuntimeError:
        return None


def merged(o, a, da, ta, b, db, tb, na=0, nb=0):
    res = merged_lk(o, a, da, ta, b, db, tb, na, nb)
    return None if res is None else res[0]


def as_pair(c):
    """A case of a merge family, of an appendProbNode family (the parent's list over 1e-4 as a non-tip against the child) or of
    sink_flag (the tip k0 against k1: the merge that makes the flags) as one pair of sides."""
    if "k0" in c:
        return dict(pv1=c["k0"], b1=c["bk0"], tip1=c["tipk0"], pv2=c["pv1"], b2=c["b1"], tip2=c["tip1"])
    if "P" in c:
        return dict(pv1=c["P"], b1=1e-4, tip1=False, pv2=c["C"], b2=c["bLen"], tip2=c["isTipC"])
    return dict(pv1=c["pv1"], b1=c["b1"], tip1=c["tip1"], pv2=c["pv2"], b2=c["b2"], tip2=c["tip2"])


def cherry_comb(o, pairs, minor=(), underflow=()):
    """Backbone node k has the children (cherry k, backbone node k + 1), the last one (cherry, a trivial leaf): the reference adds
    the cherries' contributions in the order of `pairs`, and the ids run the other way (the comb is built from its far end).
    minor: cherries whose non-tip sides are leaves with 2 and 1 minor sequences instead of internal nodes.  underflow: cherries
    whose own merge is expected to raise (their lower list is all R); every other merge of the comb must succeed.
    mark["cherry"][k] = (cherry, A_k, B_k); mark["contrib"] = {node: the Lkcontribution of the merge that made its list}, which is
    what oracle_tree_lk computes for it again (it takes them as `known`)."""
    t = Columns()
    cherries = [None] * len(pairs)
    contrib = {}
    below = None
    for k in reversed(range(len(pairs))):
        p = pairs[k]
        nm = (2, 1) if k in minor else (0, 0)
        a = t.side(p["pv1"], p["b1"], p["tip1"], nm[0])
        b = t.side(p["pv2"], p["b2"], p["tip2"], nm[1])
        tip = t.tips()
        m = merged_lk(o, p["pv1"], p["b1"], tip[a], p["pv2"], p["b2"], tip[b], t.n_minor[a], t.n_minor[b])
        assert (m is None) == (k in underflow), k
        ch = t.add(m[0] if m else ALL_R, 1e-4 * (1 + k % 3), kids=(a, b))
        cherries[k] = (ch, a, b)
        other = t.add(ALL_R, 2e-4) if below is None else below
        low = merged_lk(o, t.probVect[ch], t.dist[ch], False, t.probVect[other], t.dist[other], not t.children[other])
        assert low is not None, k
        below = t.add(low[0], 1e-4, kids=(ch, other))
        contrib[below] = low[1]
        if m:
            contrib[ch] = m[1]
    t.dist[below] = 0.0
    t.root = below
    t.mark.update(cherry=cherries, contrib=contrib)
    return t


def caterpillar(o, sides, minor=()):
    """sides = [(list, dist, tip)]: root -> (X1, sides[0]), X1 -> (sides[1], X2), ..., the last X -> (sides[-2], sides[-1]).
    sides[0]'s dist is the whole distance between sides[0] and X1: half of it goes on either branch if the halves add up to it
    exactly, else all of it on sides[0].  The X's lower lists are their children's merges, which must exist; X1's is all N where
    the root's own merge would have no result with it.  mark: "sides" (node per side), "inner" (X1, X2, ...)."""
    assert len(sides) >= 3
    t = Columns()
    dis = float(sides[0][1])
    d1 = dis / 2
    d2 = dis - d1
    if d1 + d2 != dis:
        d1, d2 = 0.0, dis
    ids = [None] * len(sides)
    ids[-1] = t.side(*sides[-1], n_minor=2 if len(sides) - 1 in minor else 0)
    below = ids[-1]
    inner = []
    for k in range(len(sides) - 2, 0, -1):
        ids[k] = t.side(*sides[k], n_minor=2 if k in minor else 0)
        tip = t.tips()
        m = merged(o, t.probVect[ids[k]], t.dist[ids[k]], tip[ids[k]], t.probVect[below], t.dist[below], tip[below],
                   t.n_minor[ids[k]], t.n_minor[below])
        assert m is not None, f"the children of X{k} have no merge (M:7797)"
        below = t.add(m, d1 if k == 1 else 1e-4 * (1 + k % 2), kids=(ids[k], below))
        inner.append(below)
    ids[0] = t.side(sides[0][0], d2, sides[0][2], n_minor=2 if 0 in minor else 0)
    tip = t.tips()
    for cand in (t.probVect[below], ALL_N):
        low = merged(o, cand, d1, False, t.probVect[ids[0]], d2, tip[ids[0]], 0, t.n_minor[ids[0]])
        if low is not None:
            break
    assert low is not None
    t.probVect[below] = [tuple(e) for e in cand]
    t.root = t.add(low, 0.0, kids=(below, ids[0]))
    assert t.dist[below] + t.dist[ids[0]] == dis
    t.mark.update(sides=ids, inner=inner[::-1])
    return t


def root_gadget(o, case, k0=None, minor=()):
    """case: a pair (as_pair) or a sink_flag / sink_abandon case, which brings its own k0; k0 = (list, dist, tip) otherwise.
    mark: k0, k1, c1, c2."""
    if "k0" in case:
        k0 = (case["k0"], case["bk0"], case["tipk0"])
        p = case
    else:
        p = as_pair(case)
    t = caterpillar(o, [(p["pv2"], p["b2"], p["tip2"]), k0, (p["pv1"], p["b1"], p["tip1"])], minor)
    s = t.mark["sides"]
    t.mark.update(c2=s[0], k0=s[1], k1=s[2], c1=t.mark["inner"][0])
    return t


def partner(cases, k):
    """lower[k0] of the k-th gadget of a family: a list of the next case, over a real branch length"""
    p = as_pair(cases[(k + 1) % len(cases)])
    return (p["pv1"], p["b1"] if p["b1"] >= 1e-100 else 1e-4, p["tip1"])


def family_gadgets(o, corp, fam, minor=()):
    """the five-node trees of a family of the corpus of one mode; minor: of c2, k0, k1 (0, 1, 2) those that are leaves with two
    minor sequences where the case wants a non-tip"""
    cases = corp[fam]
    if fam.startswith("sink"):
        return [root_gadget(o, c, minor=minor) for c in cases]
    return [root_gadget(o, c, partner(cases, k), minor) for k, c in enumerate(cases)]


def grove(o, trees, dist=1e-3):
    """The trees under one balanced backbone: neighbours are joined pair by pair, level by level, every join's lower list the
    merge of its two children's (which must exist).  mark["roots"][k] = the node that was the root of trees[k]."""
    t = Columns()
    cur = [t.graft(x, dist * (1 + k % 2)) for k, x in enumerate(trees)]
    t.mark["roots"] = list(cur)
    while len(cur) > 1:
        nxt = []
        for k in range(0, len(cur) - 1, 2):
            a, b = cur[k], cur[k + 1]
            low = merged(o, t.probVect[a], t.dist[a], False, t.probVect[b], t.dist[b], False)
            assert low is not None
            nxt.append(t.add(low, dist, kids=(a, b)))
        if len(cur) % 2:
            nxt.append(cur[-1])
        cur = nxt
    t.root = cur[0]
    t.dist[t.root] = 0.0
    return t


def gadget_sides(t):
    """the two branches whose rootings a five-node gadget is about"""
    return [t.mark["k0"], t.mark["k1"]]


# ---- the trees the tests of both kinds use (tests/test_sink_trees.py on the oracle, tests/test_hip_sink_edges.py on the GPU) ---------
_SE = le.model("siteerr")
# name -> (the mode whose corpus it uses, the model): the five standard modes and two more (global error + rate variation,
# site-specific error without rate variation), so that all six template instances <rate variation, error model, site-specific
# error> of the kernels run.  They are not in le.MODES: that would re-parametrise the tests on the other families.
MODELS = {m: (m, le.model(m)) for m in le.MODES[:5]}
MODELS["gerr_ratevar"] = ("siteerr", {k: v for k, v in _SE.items() if k != "errorRates"})
MODELS["siteerr_flat"] = ("siteerr", {k: v for k, v in _SE.items() if k != "siteRates"})
CARRY_FAMS = ("merge_carry", "long", "append_carry")
GADGET_FAMS = CARRY_FAMS + ("merge_underflow", "sink_flag", "sink_abandon")
N_COMB = 305                                                      # cherries: more than a block of 256 lanes, a ragged last wavefront


def standard_comb(o, corp):
    """N_COMB cherries of the carry families (and of sink_flag under an error model), repeated to size; every seventh one has
    leaves with minor sequences for its non-tip sides"""
    pairs = [as_pair(c) for fam in CARRY_FAMS + ("sink_flag",) if fam in corp for c in corp[fam]]
    return cherry_comb(o, [pairs[k % len(pairs)] for k in range(N_COMB)], minor=set(range(0, N_COMB, 7)))


UNDERFLOW_AT = (3, 8)


def underflow_comb(o, corp):
    """twelve cherries, the two at UNDERFLOW_AT from merge_underflow: the first in summation order has the larger node id"""
    pairs = [as_pair(c) for c in corp["merge_carry"][:6] + corp["long"][:6]]
    for k, at in enumerate(UNDERFLOW_AT):
        pairs[at] = as_pair(corp["merge_underflow"][k])
    return cherry_comb(o, pairs, underflow=set(UNDERFLOW_AT))


def deep_gadget(o, corp):
    """six heavy lists on a caterpillar: what X1 is handed from above goes down three more levels, merged with a long list each"""
    lo, ac = corp["long"], corp["append_carry"]
    sides = [(lo[0]["C"], 1e-4, True), (lo[0]["P"], 2e-4, False), (ac[0]["P"], 1e-4, False), (ac[0]["C"], 1e-5, True),
             (lo[3]["P"], 1e-4, False), (lo[3]["C"], 3e-4, True), (ac[1]["C"], 1e-4, True)]
    return caterpillar(o, sides)


def gadget_grove(o, corp):
    """every merge_carry gadget five times, with five different k0, and those of sink_flag, under one balanced backbone"""
    cases = corp["merge_carry"]
    trees = []
    for shift in (1, 2, 3, 4, 5):
        for k, c in enumerate(cases):
            p = as_pair(cases[(k + shift) % len(cases)])
            trees.append(root_gadget(o, c, (p["pv1"], p["b1"], p["tip1"])))
    trees += [root_gadget(o, c) for c in corp.get("sink_flag", [])]
    return grove(o, trees)


def with_root_mutations(t, rng):
    """the tree with a mutation list on the root: every list below it is in that frame already, the root probability is taken
    after the pass through it"""
    t.mutations[t.root] = [tuple(m) for m in le.path_mutations(rng, le.reference(), 1, 5)[0]]
    return t


def level_sizes(t):
    """internal nodes below the root per depth: the items of one level of the root search"""
    sizes, cur = [], [c for c in t.children[t.root] if t.children[c]]
    while cur:
        sizes.append(len(cur))
        cur = [c for v in cur for c in t.children[v] if t.children[c]]
    return sizes
