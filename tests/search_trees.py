"""Small trees for the SPR regraft search (maple_spr_search_batch; findBestParentTopology M:6817-7724 and the worker's accept
rule M:9681-9700): gadgets whose four list columns are set by hand so that a given search meets a given arm of the search.

A helper module like sink_trees.py, whose Columns and tuple lists it reuses.  Only the oracle (Oracle.spr_worker on
SearchColumns.oracle_tree) decides what the right answer of a search is; tests/test_search_trees.py gates, with the counting
build of the oracle, that every gadget reaches the arm it is named for, and tests/test_hip_search_edges.py runs the same
searches on the GPU in every form of the library.

Every gadget but one (five nodes, for the search seeded at the root beside a leaf) is the frame() below, thirteen nodes:

                R                   children in this order: R = (G, w), G = (P, u), P = (v, s), s = (a, b),
              /   \\                 u = (u1, u2), w = (w1, w2); the leaves are tips
             G     w
            / \\   / \\              pruning v: the search starts going up at G (handed lower[s]) and down at s (handed G's upper
           P   u  w1 w2             list); pruning a: it starts going up at P and down at b
          / \\ / \\
         v  s u1 u2
           / \\
          a   b

consistent(o, t) gives every node the lists the reference itself would compute from the leaves' lower lists (the recurrences of
reCalculateAllGenomeLists, M:6013-6347, by the oracle's operators).  A gadget then replaces single lists and branch lengths.
The recurring devices:

  stop here       probVectTotUp of a node is the oracle's own merge of what the search hands it with its lower list: the stop
                  rule (areVectorsDifferent false) fires there and everything behind it is in the cached regime, where the
                  lists the search reads (the parent's upper list, lower and probVectTotUp of the node) are free to be anything
  contradiction   two lists with different nucleotides at one site and no branch length between them: mergeVectors returns None
                  (M:4753-4758).  Next to the root a branch is scored whatever its length (M:6987, 7166)
  N but one site  lists that are N everywhere but at one or two sites: estimateBranchLengthWithDerivative finds no coefficient and,
                  the genome's total rate being above lRef, returns 0 (the evalplace_fallback family of list_edges.py)

gadgets(o, mode, mat) -> [Gadget]: name, tree, the pruned nodes to search, the search parameters, the counters (of
OMO_BC_SEARCH_LIST, without the search_ prefix) the searches must reach, and whether the frontier tier is expected to hand the
search to the one-lane kernel, and why.
"""
import numpy as np

import list_edges as le
from sink_trees import ALL_N, ALL_R, Columns

L = le.L_REF
EFF = 1.0 / (10 * L)                                               # effectivelyNon0BLen of every gadget search
NAMES = ("R", "G", "w", "P", "u", "w1", "w2", "v", "s", "u1", "u2", "a", "b")
LEAVES = ("v", "a", "b", "u1", "u2", "w1", "w2")


class SearchColumns(Columns):
    """Columns with the three upper list columns; mark[name] = node id of the frame's nodes"""

    def __init__(self):
        super().__init__()
        self.upRight, self.upLeft, self.totUp = [], [], []

    def add(self, lower, dist=0.0, kids=(), n_minor=0):
        v = super().add(lower, dist, kids, n_minor)
        for col in (self.upRight, self.upLeft, self.totUp):
            col.append(None)
        return v

    def up_list(self, parent, child):
        """the column and index of the upper list of `parent` that its child `child` is handed"""
        return (self.upRight if self.children[parent][0] == child else self.upLeft), parent

    def host_tree(self):
        from maple_amd.tree_host import HostTree
        return HostTree(self.root, self.up, self.children, self.dist, self.mutations, self.n_minor, self.probVect, self.upRight,
                        self.upLeft, self.totUp)

    def oracle_tree(self, o):
        from oracle.oracle_py import OracleTree
        return OracleTree(o, self.root, self.up, self.children, self.dist, self.mutations, self.n_minor,
                          [self.probVect, self.upRight, self.upLeft, self.totUp])

    def lists(self):
        return [gl for col in (self.probVect, self.upRight, self.upLeft, self.totUp) for gl in col if gl]


def _up(o, t, v):
    """lower[v] as its parent reads it"""
    pv = t.probVect[v]
    return o.passGenomeListThroughBranch(pv, t.mutations[v], True) if t.mutations[v] else pv


def consistent(o, t):
    """Lower lists of the internal nodes from their children's, then the upper lists and probVectTotUp from the root down.  A
    merge without a result (lists that disagree over no length) gives an all-N list: no list is absent but by a gadget's own
    doing; probVectTotUp only over a branch longer than EFF, as the reference keeps it."""
    tip = t.tips()
    order = []
    stack = [t.root]
    while stack:
        v = stack.pop()
        order.append(v)
        stack += t.children[v]
    for v in reversed(order):
        if t.children[v]:
            a, b = t.children[v]
            t.probVect[v] = o.mergeVectors(_up(o, t, a), t.dist[a], tip[a], _up(o, t, b), t.dist[b], tip[b]) or ALL_N
    for v in order:
        if not t.children[v]:
            continue
        a, b = t.children[v]
        if v == t.root:
            path = [t.mutations[v]] if t.mutations[v] else []
            t.upRight[v] = o.rootVector(_up(o, t, b), t.dist[b], tip[b], path)
            t.upLeft[v] = o.rootVector(_up(o, t, a), t.dist[a], tip[a], path)
            continue
        col, p = t.up_list(t.up[v], v)
        above = col[p]
        if t.mutations[v]:
            above = o.passGenomeListThroughBranch(above, t.mutations[v], False)
        t.upRight[v] = o.mergeVectors(above, t.dist[v], False, _up(o, t, b), t.dist[b], tip[b], isUpDown=True) or ALL_N
        t.upLeft[v] = o.mergeVectors(above, t.dist[v], False, _up(o, t, a), t.dist[a], tip[a], isUpDown=True) or ALL_N
    for v in order:
        if v == t.root or not t.dist[v] > EFF:
            continue
        col, p = t.up_list(t.up[v], v)
        above = col[p]
        if t.mutations[v]:
            above = o.passGenomeListThroughBranch(above, t.mutations[v], False)
        t.totUp[v] = o.mergeVectors(above, t.dist[v] / 2, False, t.probVect[v], t.dist[v] / 2, tip[v], isUpDown=True) or ALL_N
    return t


def leaf_lists(u, seed=0, sites=4):
    """seven tip lists with `sites` nucleotides each, at sites of their own"""
    ref = le.reference()
    rng = np.random.default_rng(1000 + seed)
    pos = rng.choice(np.arange(40, L - 40), size=7 * sites + 3, replace=False)
    out = {}
    for k, name in enumerate(LEAVES):
        mine = sorted(int(p) for p in pos[k * sites:(k + 1) * sites])
        b = le.Builder(ref, u)
        for p in mine:
            b.nuc(p, le.other(rng, int(ref[p - 1])))
        out[name] = b.done()
    return out


def clade_lists(u, seed=0):
    """seven tip lists that support the frame's own shape: a nucleotide shared by every clade of it and two of each leaf's own"""
    ref = le.reference()
    rng = np.random.default_rng(2000 + seed)
    clades = [("a", "b"), ("v", "a", "b"), ("u1", "u2"), ("v", "a", "b", "u1", "u2"), ("w1", "w2")] + [(n,) for n in LEAVES] * 2
    pos = rng.choice(np.arange(40, L - 40), size=len(clades), replace=False)
    sites = {n: {} for n in LEAVES}
    for p, members in zip(pos, clades):
        nuc = le.other(rng, int(ref[int(p) - 1]))
        for n in members:
            sites[n][int(p)] = nuc
    out = {}
    for n in LEAVES:
        b = le.Builder(ref, u)
        for p in sorted(sites[n]):
            b.nuc(p, sites[n][p])
        out[n] = b.done()
    return out


def frame(o, leaves, dist=None, mutations=None):
    """the thirteen-node tree over the leaves' lists (a dict by LEAVES), branch lengths from `dist` (by NAMES; 1e-4 .. 4e-4 else)
    and mutation lists from `mutations` (by NAMES), every other list consistent"""
    d = {n: 1e-4 * (1 + k % 4) for k, n in enumerate(NAMES)}
    d.update(dist or {})
    t = SearchColumns()
    m = t.mark
    for n in LEAVES:
        m[n] = t.add(leaves[n], d[n])
    m["s"] = t.add(ALL_N, d["s"], kids=(m["a"], m["b"]))
    m["P"] = t.add(ALL_N, d["P"], kids=(m["v"], m["s"]))
    m["u"] = t.add(ALL_N, d["u"], kids=(m["u1"], m["u2"]))
    m["G"] = t.add(ALL_N, d["G"], kids=(m["P"], m["u"]))
    m["w"] = t.add(ALL_N, d["w"], kids=(m["w1"], m["w2"]))
    m["R"] = t.root = t.add(ALL_N, 0.0, kids=(m["G"], m["w"]))
    for name, ml in (mutations or {}).items():
        t.mutations[m[name]] = [tuple(x) for x in ml]
    return consistent(o, t)


PARAMS = dict(strict=False, allowedFails=5, thresholdLogLKtopology=1e9, thresholdTopologyPlacement=-0.1,
              thresholdLogLKoptimizationTopology=1e9, thresholdLogLKconsecutivePlacement=1.0, effectivelyNon0BLen=EFF)


# ---- what a search that never stops updating hands every node: the lists a "stop here" is made of ---------------------------------
def handed(o, t, pruned):
    """{("down" | "up", node): dict(passed, distance, mid, bottom, vect_up)} of findBestParentTopology from `pruned`, as long as it
    updates lists and whatever it scores (M:6982-7434 without the stop and score rules): mid = the midTot the node is scored
    with, bottom / vect_up = an upward item's midBottom and the upper list it reads.  None where a merge has no result."""
    tip = t.tips()
    ch, up, dist, mut = t.children, t.up, t.dist, t.mutations

    def down_(gl, v):
        return o.passGenomeListThroughBranch(gl, mut[v], False) if gl is not None and mut[v] else gl

    def merge(a, da, ta, b, db, tb, upd):
        if a is None or b is None:
            return None
        return o.mergeVectors(a, float(da), bool(ta), b, float(db), bool(tb), isUpDown=upd)

    def path(v):
        p = []
        while v is not None:
            if mut[v]:
                p.append(mut[v])
            v = up[v]
        return p

    node = up[pruned]
    sib = [c for c in ch[node] if c != pruned][0]
    out, stack = {}, []
    if up[node] is not None:
        parent = up[node]
        col, i = t.up_list(parent, node)
        d = dist[sib] + dist[node]
        pv1 = _up(o, t, sib)
        if mut[node]:
            pv1 = o.passGenomeListThroughBranch(pv1, mut[node], True)
        stack.append((parent, 1 if ch[parent][0] == node else 2, pv1, d))
        stack.append((sib, 0, down_(down_(col[i], node), sib), d))
    elif ch[sib]:
        c1, c2 = ch[sib]
        stack.append((c1, 0, down_(o.rootVector(_up(o, t, c2), dist[c2], tip[c2], path(node)), c1), dist[c1]))
        stack.append((c2, 0, down_(o.rootVector(_up(o, t, c1), dist[c1], tip[c1], path(node)), c2), dist[c2]))
    while stack:
        t1, direction, passed, distance = stack.pop()
        if direction == 0:
            rec = dict(passed=passed, distance=distance, mid=None)
            out[("down", t1)] = rec
            if not (up[t1] == node or up[t1] is None):
                rec["mid"] = merge(passed, distance / 2, False, t.probVect[t1], distance / 2, tip[t1], True)
            for k in (0, 1) if ch[t1] else ():
                c, other = ch[t1][k], ch[t1][1 - k]
                v_up = merge(passed, distance, False, _up(o, t, other), dist[other], tip[other], True)
                if v_up is not None:
                    stack.append((c, 0, down_(v_up, c), dist[c]))
            continue
        other = ch[t1][1] if direction == 1 else ch[t1][0]
        rec = dict(passed=passed, distance=distance, mid=None, bottom=None, vect_up=None)
        out[("up", t1)] = rec
        rec["bottom"] = merge(passed, distance, False, _up(o, t, other), dist[other], tip[other], False)
        if up[t1] is None:
            stack.append((other, 0, down_(o.rootVector(passed, distance, False, path(t1)), other), dist[other]))
            continue
        col, i = t.up_list(up[t1], t1)
        rec["vect_up"] = down_(col[i], t1)
        rec["mid"] = merge(rec["vect_up"], dist[t1] / 2, False, rec["bottom"], dist[t1] / 2, False, True)
        v_up = merge(rec["vect_up"], dist[t1], False, passed, distance, False, True)
        if v_up is None:
            continue
        stack.append((other, 0, down_(v_up, other), dist[other]))
        if rec["bottom"] is not None:
            bottom = o.passGenomeListThroughBranch(rec["bottom"], mut[t1], True) if mut[t1] else rec["bottom"]
            stack.append((up[t1], 1 if ch[up[t1]][0] == t1 else 2, bottom, dist[t1]))
    return out


def stop_at(o, t, pruned, direction, name):
    """probVectTotUp of the node := the midTot the search from `pruned` scores it with: the stop rule fires there"""
    mid = handed(o, t, t.mark[pruned])[(direction, t.mark[name])]["mid"]
    assert mid is not None, (pruned, direction, name)
    t.totUp[t.mark[name]] = mid
    return t


# ---- the gadgets ----------------------------------------------------------------------------------------------------------------
K1, K2 = 700, 900                                                  # the sites the hand-made lists differ at


class Gadget:
    def __init__(self, name, tree, prune, reach, params=None, handback=None, whole_tree=False):
        """prune: names of the pruned nodes; reach: the counters every mode must reach; handback: None, or the reasons
        (Device.HANDBACK_REASONS, or None) for which the frontier tier hands a search to the one-lane kernel in a batch of at
        most 64 searches (k_fr_replay walks without a layout) and in a larger one (the walk over the laid-out items); whole_tree:
        the library takes the search for a whole-tree search at once (a pruned branch of length 0 without an error model) and
        scores it from the dense table: the frontier tier then has no list-updating item unless wide_search_budget < 0"""
        self.name, self.tree, self.reach, self.handback = name, tree, tuple(reach), handback or (None, None)
        self.prune, self.whole_tree = tuple(prune), whole_tree
        self.nodes = [tree.mark[p] for p in self.prune]
        self.params = dict(PARAMS)
        self.params.update(params or {})


def one_site(u, at, fill=4):
    """a list that is R (fill 4) or N (fill 5) everywhere but for the nucleotides {site: which non-reference one, 0..2} of `at`"""
    ref = le.reference()
    b = le.Builder(ref, u)
    cur = 1
    for p in sorted(at):
        if fill == 5 and p > cur:
            b.run(5, cur, p - 1)
        b.nuc(p, [x for x in range(4) if x != int(ref[p - 1])][at[p]])
        cur = p + 1
    if fill == 5 and cur <= L:
        b.run(5, cur, L)
    return b.done()


def set_list(t, kind, name, gl, child=None):
    """kind: lower, totUp, or up (the upper list of `name` that its child `child` reads)"""
    v = t.mark[name]
    if kind == "up":
        col, v = t.up_list(v, t.mark[child])
    else:
        col = t.probVect if kind == "lower" else t.totUp
    col[v] = None if gl is None else [tuple(e) for e in gl]


def non_tip(t, name):
    """a leaf with one minor sequence is no tip (M:4489): an error model does not flag its entries"""
    t.n_minor[t.mark[name]] = 1


def _frame(o, u, dist=None, seed=0, mutations=None, leaves=None):
    lv = leaf_lists(u, seed)
    lv.update(leaves or {})
    return frame(o, lv, dist, mutations)


def gadgets(o, mode, mat=False):
    """The gadgets of a mode (o is set to its model).  mat: each with a mutation list on the root, which every list of the tree
    is below: the lists stay what they are, the root's two upper lists and every rootVector of a search pass through it, and
    the library runs the instantiations for trees with local references."""
    u = bool(le.model(mode).get("usingErrorRate"))
    corp = le.corpus(mode)
    mut = None
    if mat:
        mut = {"R": [tuple(m) for m in le.path_mutations(np.random.default_rng(11), le.reference(), 1, 5)[0]]}
    X, Y = one_site(u, {K1: 0}), one_site(u, {K1: 1})
    XN, YN, ZN = one_site(u, {K1: 0}, 5), one_site(u, {K1: 1}, 5), one_site(u, {K2: 2}, 5)
    out = []

    def add(name, t, prune, reach, params=None, handback=None, whole_tree=False):
        out.append(Gadget(name, t, prune, reach, params, handback, whole_tree))

    # the two stop-rule arms, and the regimes behind them
    t = _frame(o, u, mutations=mut)
    stop_at(o, t, "v", "down", "a")
    stop_at(o, t, "v", "up", "G")
    add("stop_rules", t, ["v"], ["down_stop", "up_stop", "root_cross_cached"])
    t = _frame(o, u, mutations=mut)
    add("plain", t, ["v", "a", "u1", "w", "s"], ["root_cross_updating", "seed_root_sibling_inner", "veto_below_sibling"])
    # a node without probVectTotUp over a real branch
    t = _frame(o, u, mutations=mut)
    set_list(t, "totUp", "G", None)
    add("totup_on_the_spot", t, ["v"], ["up_totup_on_the_spot"])
    # going down, M:7037-7044: over the root (lengths of 0 up to there), w is handed X and holds Y
    t = _frame(o, u, dict(s=0.0, P=0.0, G=0.0, u=0.0, w=0.0), mutations=mut)
    for name in ("s", "u"):
        set_list(t, "lower", name, X)
    set_list(t, "up", "R", X, "G")
    set_list(t, "lower", "w", Y)
    add("down_mid_none", t, ["v"], ["down_mid_none", "root_cross_updating"])
    # going down: the vectUp of s's child a, from G's upper list X and lower[b] = Y, b no tip
    t = _frame(o, u, dict(s=0.0, P=0.0, b=0.0), mutations=mut)
    set_list(t, "up", "G", X, "P")
    set_list(t, "lower", "b", Y)
    non_tip(t, "b")
    add("down_vup_none", t, ["v"], ["down_vup_none"])
    # crawling up, M:7170-7178: lower[s] = X handed to G, whose other child u holds Y
    t = _frame(o, u, dict(s=0.0, P=0.0, u=0.0), mutations=mut)
    set_list(t, "lower", "s", X)
    set_list(t, "lower", "u", Y)
    add("up_bottom_none", t, ["v"], ["up_bottom_none"])
    # ... midBottom is X, the root's upper list Y
    t = _frame(o, u, dict(s=0.0, P=0.0, u=0.0, G=0.0), mutations=mut)
    set_list(t, "lower", "s", X)
    set_list(t, "lower", "u", X)
    set_list(t, "up", "R", Y, "G")
    add("up_mid_none", t, ["v"], ["up_mid_none"])
    # ... pruning a: P over no length is not scored, G's upper list Y meets lower[b] = X
    t = _frame(o, u, dict(s=0.0, P=0.0, b=0.0), mutations=mut)
    set_list(t, "lower", "b", X)
    set_list(t, "up", "G", Y, "P")
    add("up_vup_none", t, ["a"], ["up_vup_none"])
    # ... the late midBottom: lower[b] = X against lower[v] = Y, v no tip
    t = _frame(o, u, dict(s=0.0, P=0.0, b=0.0, v=0.0), mutations=mut)
    set_list(t, "lower", "b", X)
    set_list(t, "lower", "v", Y)
    set_list(t, "up", "G", X, "P")
    non_tip(t, "v")
    add("up_bottom_late_none", t, ["a"], ["up_bottom_late_none"])

    # ---- the refinement, M:7460-7639.  Pruning u: the search stops updating at s, whose children a and b are then scored and
    # refined from the tree's own lists: upV = s's upper list, downV = lower[a], midTot = probVectTotUp[a], removed = lower[u]
    def below_s(case_lists, dist_a, tip_a=True):
        t = _frame(o, u, dict(a=dist_a), mutations=mut)
        up_v, down_v, mid, rem = case_lists
        set_list(t, "lower", "u", rem)
        stop_at(o, t, "u", "down", "s")
        set_list(t, "up", "s", up_v, "a")
        set_list(t, "lower", "a", down_v)
        set_list(t, "totUp", "a", mid)
        if not tip_a:
            non_tip(t, "a")
        return t
    for k, c in enumerate(corp["evalplace_fallback"][:2]):                # midTop None, then not None over defaultBLen * 0.1
        t = below_s((c["up"], c["down"], c["midTot"], c["rem"]), c["distance"], c["fromTip1"])
        add(f"refine_top_retry_{k}", t, ["u"], ["refine_top_retry"])
    # newMid None: upV and downV disagree at K1, the removed list is N there: every estimated length is 0
    t = below_s((YN, XN, ZN, ZN), 2e-4, False)
    add("refine_newmid_none", t, ["u"], ["refine_newmid_none", "status_minus_1"])
    # midLower None: over no length (G hangs on the root, reached in the cached regime: pruning a, the search stops at P),
    # lower[G] and the removed list disagree at K1
    t = _frame(o, u, dict(G=0.0), mutations=mut)
    set_list(t, "lower", "a", XN)
    non_tip(t, "a")
    stop_at(o, t, "a", "up", "P")
    set_list(t, "lower", "G", YN)
    set_list(t, "totUp", "G", XN)
    set_list(t, "up", "R", ALL_N, "G")
    add("refine_lower_none", t, ["a"], ["refine_lower_none", "status_minus_1"])
    # a record without its upper list: the same search, the root's upper list towards G absent
    t = _frame(o, u, mutations=mut)
    stop_at(o, t, "a", "up", "P")
    set_list(t, "up", "R", None, "G")
    add("refine_no_list", t, ["a"], ["refine_no_list", "status_minus_1"])

    # ---- the worker: status 2, a score of -inf, the vetoes of the accept rule (M:9681-9700)
    t = _frame(o, u, dict(v=0.0), mutations=mut, leaves=dict(v=ALL_R))
    add("status_2", t, ["v"], ["status_2"], dict(thresholdTopologyPlacement=-1e9))
    t = _frame(o, u, dict(v=0.0), mutations=mut)
    non_tip(t, "v")
    add("score_minus_inf", t, ["v"], ["score_minus_inf"], whole_tree=not u)
    # a tree whose tips support its shape: nothing scores above the present placement, the sibling stays the best node
    t = frame(o, clade_lists(u), None, mut)
    add("veto_sibling", t, ["v", "u1", "w1"], ["veto_sibling"],
        dict(thresholdTopologyPlacement=1.0, thresholdLogLKoptimizationTopology=0.0))
    # ... P at no distance below G; under strict rules without any tolerance G's branch is the only one scored, and it is
    # refined to a bottom length of 0: where v hangs already
    t = frame(o, clade_lists(u), dict(P=0.0), mut)
    add("veto_chain_top", t, ["v"], ["chain_step", "veto_chain_top"],
        dict(thresholdTopologyPlacement=1.0, strict=True, thresholdLogLKtopology=0.0))
    t = _frame(o, u, dict(P=0.0, G=0.0), mutations=mut)
    add("chain_to_the_root", t, ["v", "a"], ["chain_step"], dict(thresholdTopologyPlacement=1.0))

    # ---- the in-place shorten of the removed list, M:7087: the pruned tip carries the nucleotides of another tip, so that a
    # branch on the way down beats the present placement, and two adjacent R entries with one and the same tail
    def tailed(name):
        ref = le.reference()
        b = le.Builder(ref, u).run(4, 1, 10, d0=1e-4).run(4, 11, 20, d0=1e-4)
        pos = 0
        for e in clade_lists(u)[name]:
            pos = e[1] if e[0] in (4, 5) else pos + 1
            if e[0] < 4:
                b.nuc(pos, e[0])
        return b.done()
    def branch(p):
        ref = le.reference()
        return [le.mutation(ref, p, False, le.other(np.random.default_rng(p), int(ref[p - 1])))]
    # ... the search's own first list: b's branch beats v's placement while the list is still the one the search began with
    t = frame(o, dict(clade_lists(u), v=tailed("b")), None, mut)
    add("shorten_own", t, ["v"], ["shorten_own"], handback=("marked_without_layout", "own_list_shortened"))
    # ... its copy in the sibling's frame (a mutation on s's branch), which is the list the search returns if nothing is better
    t = frame(o, dict(clade_lists(u), v=tailed("b")), None, dict(mut or {}, s=branch(30)))
    add("shorten_passed", t, ["v"], ["shorten_passed"], handback=("marked_without_layout", "own_list_shortened"))
    # ... P's branch (the copy in P's frame) beats u1's placement, then the copy is re-expressed again into s's frame
    t = frame(o, dict(clade_lists(u), u1=tailed("v")), None, dict(mut or {}, P=branch(30), s=branch(35)))
    add("shorten_passed_on", t, ["u1"], ["shorten_passed"], handback=("marked_without_layout", "passed_from_shortened"))
    add("seed_root_sibling_leaf", _leaf_sibling(o, u, mut), ["s", "v"], ["seed_root_sibling_leaf", "seed_root_sibling_inner"])
    return out


def _leaf_sibling(o, u, mut):
    """five nodes, root = (s, v) with v a leaf: pruning s leaves a search from the root with nothing to visit"""
    lv = leaf_lists(u, 3)
    t = SearchColumns()
    m = t.mark
    m["v"] = t.add(lv["v"], 2e-4)
    m["a"], m["b"] = t.add(lv["a"], 1e-4), t.add(lv["b"], 3e-4)
    m["s"] = t.add(ALL_N, 1e-4, kids=(m["a"], m["b"]))
    m["R"] = t.root = t.add(ALL_N, 0.0, kids=(m["s"], m["v"]))
    for name, ml in (mut or {}).items():
        t.mutations[m[name]] = [tuple(x) for x in ml]
    return consistent(o, t)
