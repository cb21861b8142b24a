"""An oracle twin of the repair of the genome lists around one change (updatePartials with updateBLen, M:5385-5414, 5479-5815) and
small trees that send the repair into its rarely taken arms.

A helper module like sink_trees.py.  The twin works on tuple lists and calls nothing but the C oracle (oracle/oracle_py.py):

  oracle_update_partials(o, tree, nodeList, counts)   the reference's LIFO work list of (node, direction) items -- direction 2: the
                                change comes from the parent, 0 / 1: from that child -- without time trees and HnZ.  It keeps the
                                reference's order of work, its madeChange / updatedBLen rules and its quirks: a list made again
                                after updateBLen in a None arm is stored as mergeVectors gave it, NOT shortened (M:5577, 5593,
                                5692, 5711-5713, 5735); the verdict of the upper lists is areVectorsDifferent(old, unshortened
                                new) (M:5646, 5799), that of the lower list areVectorsDifferent(shortened new, old) (M:5808).
                                Where the reference raises ("Strange: None vector from non-zero distances", M:5583 / 5600 / 5697 /
                                5741) or would fail on a None list, the twin raises RepairError.  counts: a dict that receives
                                one counter per place the reference can go (ARMS).  Returns what the call looked at: the nodes it
                                popped, the nodes it marked dirty, the nodes whose length updateBLen set.

`tree` is a Lists tree: the columns of sink_trees.Columns plus probVectUpRight, probVectUpLeft, probVectTotUp (None: no list).
`consistent(o, t)` makes every list of a tree from the tips' lower lists with the oracle's operators in the order of
reCalculateAllGenomeLists (M:6013-6347); `fixture_lists(f)` is the tree of a search_* fixture.

The gadgets are five-node trees root -> (inner, C), inner -> (A, B) (tests/test_hip_struct_edges.py) over lRef = le.L_REF: all
lists consistent, then ONE change at a tip (its lower list and / or its length) with the zero lengths and the few hand-set sites
that send the repair into one arm.  Every hand-set site differs materially (another nucleotide) or not at all, far from
thresholdProb / thresholdDiffForUpdate: the verdicts of areVectorsDifferent do not hang on rounding, so the visiting order -- LIFO
in the twin, level by level in the library -- cannot change the outcome.  gadgets(o, mode) -> {name: Gadget}; zero_gadgets(o, mode)
for the two zero-rate modes.  run_twin(o, gadget) is the twin on a gadget; compare_with_twin holds a library's repair to it.
"""
import numpy as np

import list_edges as le
import sink_trees as st

L = le.L_REF

ARMS = ("from_parent_totup_none", "from_parent_totup_zero_len",
        "from_parent_upright_none_node_lengthened", "from_parent_upright_none_child_lengthened",
        "from_parent_upleft_none_node_lengthened", "from_parent_upleft_none_child_lengthened", "from_parent_raise",
        "from_child_lower_none_child_lengthened", "from_child_lower_none_other_lengthened", "from_child_lower_raise",
        "from_child_totup_none",
        "from_child_upvect_none_node_lengthened", "from_child_upvect_none_child_lengthened", "from_child_upvect_raise",
        "from_child_at_root", "stop_upper_same", "stop_lower_same", "other_upper_absent", "old_lower_absent")
KEYS = ("probVect", "probVectUpRight", "probVectUpLeft", "probVectTotUp")


class RepairError(RuntimeError):
    """where the reference's updatePartials raises, or fails on a list that is None"""


class Lists(st.Columns):
    """sink_trees.Columns with the three upper lists of every node"""

    def __init__(self):
        super().__init__()
        self.probVectUpRight, self.probVectUpLeft, self.probVectTotUp = [], [], []

    def add(self, lower, dist=0.0, kids=(), n_minor=0):
        v = super().add(lower if lower is not None else [], dist, kids, n_minor)
        if lower is None:
            self.probVect[v] = None
        for col in (self.probVectUpRight, self.probVectUpLeft, self.probVectTotUp):
            col.append(None)
        return v

    def copy(self):
        c = Lists()
        c.root, c.mark = self.root, dict(self.mark)
        c.up, c.dist, c.n_minor = list(self.up), list(self.dist), list(self.n_minor)
        c.children, c.mutations = [list(x) for x in self.children], [list(x) for x in self.mutations]
        for k in KEYS:
            setattr(c, k, [None if gl is None else list(gl) for gl in getattr(self, k)])
        return c

    def host_tree(self):
        from maple_amd.tree_host import HostTree
        return HostTree(self.root, self.up, self.children, self.dist, self.mutations, self.n_minor, self.probVect, self.probVectUpRight,
                        self.probVectUpLeft, self.probVectTotUp)

    def reachable(self):
        out, stack = [], [self.root]
        while stack:
            v = stack.pop()
            out.append(v)
            stack.extend(self.children[v])
        return out


def _tl(gl):
    return None if not gl else [tuple(e) for e in gl]


def fixture_lists(f):
    """the tree of a search_* fixture with its four lists per node"""
    t = f["tree"]
    c = Lists()
    c.root, c.up, c.children = t["root"], list(t["up"]), [list(x or []) for x in t["children"]]
    c.dist = [float(x or 0.0) for x in t["dist"]]
    c.mutations = [[tuple(m) for m in (ml or [])] for ml in t["mutations"]]
    c.n_minor = list(t["nMinor"])
    for k in KEYS:
        setattr(c, k, [_tl(gl) for gl in t[k]])
    return c


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
def oracle_update_partials(o, tree, nodeList, counts, log=None):
    """log: a list that receives (arm, node) in the order the arms are taken"""
    ch, up, dist, mut = tree.children, tree.up, tree.dist, tree.mutations
    low, ur, ul, tu = tree.probVect, tree.probVectUpRight, tree.probVectUpLeft, tree.probVectTotUp
    tip = st.default_tip(tree)
    work = [tuple(x) for x in nodeList]
    popped, dirty, lengths = [], set(), set()

    def arm(name):
        assert name in ARMS
        counts[name] = counts.get(name, 0) + 1
        if log is not None:
            log.append((name, v))

    def merge(a, da, ta, b, db, tb, up_down=False):
        if a is None or b is None:
            raise RepairError("mergeVectors of a list that is None")
        return o.mergeVectors(a, float(da), bool(ta), b, float(db), bool(tb), isUpDown=up_down)

    def shorten(gl, v):
        if gl is None:                                                  # (shorten(None), M:5542 / 5648 / 5652 / 5704: a TypeError there)
            raise RepairError(f"None vector after updateBLen at node {v}")
        return o.shorten(gl)

    def lower_up(k):
        return o.passGenomeListThroughBranch(low[k], mut[k], True) if mut[k] else low[k]

    def upper_seen_by(c):                                               # M:5396-5403 / 5503-5514
        p = up[c]
        vect = ur[p] if ch[p][0] == c else ul[p]
        if mut[c] and vect is not None:
            vect = o.passGenomeListThroughBranch(vect, mut[c], False)
        return vect

    def update_blen(c, push):                                           # updateBLen, M:5385-5414
        p = up[c]
        if p is None:
            raise RepairError(f"updateBLen of the root {c}")
        vect = upper_seen_by(c)
        if vect is None:
            raise RepairError(f"updateBLen of node {c} without an upper list")
        best = o.estimateBranchLengthWithDerivative(vect, low[c], tip[c])
        dist[c] = 0.0 if best is False else float(best)                 # (the reference stores False: the same number everywhere)
        lengths.add(c)
        dirty.update((p, c))
        if push:
            work.append((c, 2))
            work.append((p, 0 if ch[p][0] == c else 1))

    while work:
        updated = made = False                                          # updatedBLen, madeChange (M:5496-5497)
        v, direction = work.pop()
        popped.append(v)
        dirty.add(v)
        p = up[v]
        if p is not None:
            num_up = 0 if ch[p][0] == v else 1
            seen = upper_seen_by(v)                                     # vectUpUp
        if direction == 2:                                              # ---- from the parent, M:5519-5658
            if dist[v]:
                new = merge(seen, dist[v] / 2, False, low[v], dist[v] / 2, tip[v], True)
                if new is None:                                         # M:5523-5529
                    arm("from_parent_totup_none")
                    update_blen(v, False)
                    work.append((p, num_up))
                    new = merge(seen, dist[v] / 2, False, low[v], dist[v] / 2, tip[v], True)
                    made = True
                tu[v] = shorten(new, v)
            else:
                arm("from_parent_totup_zero_len")
                tu[v] = None
            if ch[v]:
                k0, k1 = ch[v]
                v0, v1 = lower_up(k0), lower_up(k1)
                new_r = merge(seen, dist[v], False, v1, dist[k1], tip[k1], True)
                new_l = None
                for which, kid in ((1, k1), (0, k0)):                   # upRight from child 1 (M:5569-5583), upLeft from child 0 (M:5585-5600)
                    if which == 0:
                        if updated:
                            break
                        new_l = merge(seen, dist[v], False, v0, dist[k0], tip[k0], True)
                    if (new_r if which else new_l) is not None:
                        continue
                    side = "upright" if which else "upleft"
                    if dist[v] or dist[kid]:
                        arm("from_parent_raise")
                        raise RepairError(f"None upper vector from non-zero distances at node {v}")
                    update_blen(v, False)
                    if not dist[v]:
                        arm(f"from_parent_{side}_none_child_lengthened")
                        update_blen(kid, True)
                        updated = True
                    else:
                        arm(f"from_parent_{side}_none_node_lengthened")
                        tu[v] = merge(seen, dist[v] / 2, False, low[v], dist[v] / 2, tip[v], True)     # (not shortened)
                        new_r = merge(seen, dist[v], False, v1, dist[k1], tip[k1], True)
                        if which == 0:
                            new_l = merge(seen, dist[v], False, v0, dist[k0], tip[k0], True)
                        work.append((p, num_up))
                        made = True
                if not updated:                                         # M:5645-5658
                    for col, new, kid in ((ur, new_r, k0), (ul, new_l, k1)):
                        if not made and col[v] is None:
                            raise RepairError(f"node {v} has no upper list to compare with")
                        if made or o.areVectorsDifferent(col[v], new):
                            col[v] = shorten(new, v)
                            work.append((kid, 2))
                        else:
                            arm("stop_upper_same")
            continue
        # ---- from child number `direction`, M:5660-5814
        kc, ko = ch[v][direction], ch[v][1 - direction]
        cd, od = dist[kc], dist[ko]
        v_other, v_down = lower_up(ko), lower_up(kc)
        other_up = ur[v] if direction else ul[v]
        old = None
        new = merge(v_other, od, tip[ko], v_down, cd, tip[kc])
        if new is None:                                                 # M:5684-5697
            if cd or od:
                arm("from_child_lower_raise")
                raise RepairError(f"None vector from non-zero distances in the lower merge at node {v}")
            update_blen(kc, False)
            if not dist[kc]:
                arm("from_child_lower_none_other_lengthened")
                update_blen(ko, True)
                updated = True
            else:
                arm("from_child_lower_none_child_lengthened")
                cd = dist[kc]
                low[v] = merge(v_other, od, tip[ko], v_down, cd, tip[kc])                              # (not shortened)
                work.append((kc, 2))
                made = True
        else:
            old = low[v]
            if old is None:
                arm("old_lower_absent")
            low[v] = shorten(new, v)
        if not updated and dist[v] and p is not None and seen is not None:                             # M:5707-5718
            tot = merge(seen, dist[v] / 2, False, low[v], dist[v] / 2, False, True)
            if tot is None:
                arm("from_child_totup_none")
                update_blen(v, False)
                low[v] = merge(v_other, od, tip[ko], v_down, cd, tip[kc])                              # (not shortened)
                work.append((kc, 2))
                tu[v] = merge(seen, dist[v] / 2, False, low[v], dist[v] / 2, False, True)              # (not shortened)
                made = True
            else:
                tu[v] = shorten(tot, v)
        elif not dist[v]:
            tu[v] = None
        new_up = None
        if not updated and other_up is None:
            arm("other_upper_absent")
        if not updated and other_up is not None:                        # M:5722-5741
            if p is not None:
                new_up = merge(seen, dist[v], False, v_down, cd, tip[kc], True)
            else:
                arm("from_child_at_root")
                new_up = o.rootVector(v_down, float(cd), bool(tip[kc]), [mut[v]] if mut[v] else [])
            if new_up is None:
                if dist[v] or cd:
                    arm("from_child_upvect_raise")
                    raise RepairError(f"None upper vector from non-zero distances at node {v}")
                update_blen(v, False)
                if not dist[v]:
                    arm("from_child_upvect_none_child_lengthened")
                    update_blen(kc, True)
                    updated = True
                else:
                    arm("from_child_upvect_none_node_lengthened")
                    tu[v] = merge(seen, dist[v] / 2, False, low[v], dist[v] / 2, False, True)          # (not shortened)
                    work.append((kc, 2))
                    made = True
                    new_up = merge(seen, dist[v], False, v_down, cd, tip[kc], True)
        if updated:
            continue
        up_changed = down_changed = False                               # M:5795-5814
        if other_up is not None:
            if made or o.areVectorsDifferent(other_up, new_up):
                up_changed = True
                (ur if direction else ul)[v] = shorten(new_up, v)
            else:
                arm("stop_upper_same")
        if made or o.areVectorsDifferent(low[v], old):
            down_changed = True
        else:
            arm("stop_lower_same")
        if p is not None and down_changed:
            work.append((p, num_up))
        if up_changed:
            work.append((ko, 2))
    return dict(popped=popped, dirty=dirty, lengths=lengths)


def changed_node_list(tree, v):
    """the pair updateBLen(addToList=True) pushes for a change at v (M:5412-5414): what the recorded repairs started from"""
    p = tree.up[v]
    return [(v, 2), (p, 0 if tree.children[p][0] == v else 1)]


# ---- consistent lists ---------------------------------------------------------------------------------------------------------------
def consistent(o, t, bump=None):
    """Every list of t from the tips' lower lists, in the order of reCalculateAllGenomeLists (M:6013-6347): lower lists from the
    deepest level up, then the upper lists from the root down, every merge shortened.  A None between two zero-length branches
    raises (bump: lengthen both to it and merge again, as maple_tree_rebuild_lists does with bumpLen).  Returns t."""
    tip = st.default_tip(t)
    order = t.reachable()                                               # (a parent before its children)

    def lower_up(k):
        return o.passGenomeListThroughBranch(t.probVect[k], t.mutations[k], True) if t.mutations[k] else t.probVect[k]

    for v in reversed(order):
        if not t.children[v]:
            continue
        a, b = t.children[v]
        m = o.mergeVectors(lower_up(a), t.dist[a], tip[a], lower_up(b), t.dist[b], tip[b])
        if m is None and bump:
            t.dist[a], t.dist[b] = max(t.dist[a], bump), max(t.dist[b], bump)
            m = o.mergeVectors(lower_up(a), t.dist[a], tip[a], lower_up(b), t.dist[b], tip[b])
        if m is None:
            raise RepairError(f"inconsistent lower lists at node {v}")
        t.probVect[v] = o.shorten(m)
    for v in order:
        t.probVectUpRight[v] = t.probVectUpLeft[v] = t.probVectTotUp[v] = None
        if v == t.root:
            if t.children[v]:
                a, b = t.children[v]
                path = [t.mutations[v]] if t.mutations[v] else []
                t.probVectUpRight[v] = o.rootVector(lower_up(b), t.dist[b], tip[b], path)
                t.probVectUpLeft[v] = o.rootVector(lower_up(a), t.dist[a], tip[a], path)
            continue
        p = t.up[v]
        seen = t.probVectUpRight[p] if t.children[p][0] == v else t.probVectUpLeft[p]
        if t.mutations[v]:
            seen = o.passGenomeListThroughBranch(seen, t.mutations[v], False)
        if t.dist[v]:
            m = o.mergeVectors(seen, t.dist[v] / 2, False, t.probVect[v], t.dist[v] / 2, tip[v], isUpDown=True)
            t.probVectTotUp[v] = None if m is None else o.shorten(m)    # (a None probVectTotUp stays None, M:6270)
        if t.children[v]:
            a, b = t.children[v]
            r = o.mergeVectors(seen, t.dist[v], False, lower_up(b), t.dist[b], tip[b], isUpDown=True)
            l = o.mergeVectors(seen, t.dist[v], False, lower_up(a), t.dist[a], tip[a], isUpDown=True)
            if r is None or l is None:
                raise RepairError(f"inconsistent upper lists at node {v}")
            t.probVectUpRight[v], t.probVectUpLeft[v] = o.shorten(r), o.shorten(l)
    return t


# ---- the gadgets ----------------------------------------------------------------------------------------------------------------------
TA, TB, INNER, TC, ROOT = 0, 1, 2, 3, 4                               # ids of five(): children are added before their parent
S = 720                                                               # the hand-set site


class Gadget:
    """before: the consistent tree with the change applied (the lists of the other nodes as they were); changed: the node the repair
    starts from; arms: the twin's counters the gadget is named for; stats: lower bounds on what maple_debug_update_partials_stats
    must show; raises: a piece of the message where the twin raises and the library returns MAPLE_ERR_FATAL; python_loop_raises:
    the Python level loop (update_genome_lists(native=False)) stops in the upper pass with "updateBLen" in its message; again:
    the reference leaves a list as it was made with the old length of a branch that updateBLen lengthened without addToList (see
    gadgets()), so the twin is called once more for every such branch, as the reference's callers do for a changed length; after:
    after(o, tree) finishes what the reference leaves undone where a list is absent (see gadgets(), upper_absent); redo: items
    the reference abandons (updatedBLen) and never takes up again, run once the twin is through (see gadgets(), *_none_child);
    complete: the finished twin is the tree rebuilt from its leaves (not where a hand-set child was never announced as changed and
    its parent's lower list is not made again); never: counters of the library that must stay 0."""

    def __init__(self, name, before, changed, arms=(), stats=(), raises=None, python_loop_raises=False, again=False, after=None, redo=(),
                 complete=True, never=()):
        self.name, self.before, self.changed, self.arms, self.stats, self.raises = name, before, changed, tuple(arms), dict(stats), raises
        self.python_loop_raises, self.again, self.after, self.redo, self.complete = python_loop_raises, again, after, tuple(redo), complete
        self.never = tuple(never)


def run_twin(o, g, counts=None, log=None):
    """the twin on a copy of the gadget's tree: (tree after, what oracle_update_partials returned); raises RepairError"""
    t = g.before.copy()
    counts = {} if counts is None else counts
    res = oracle_update_partials(o, t, changed_node_list(t, g.changed), counts, log)
    if g.again:
        for w in sorted(res["lengths"]):
            more = oracle_update_partials(o, t, changed_node_list(t, w), {})
            res["popped"] += more["popped"]
            res["dirty"] |= more["dirty"]
            res["lengths"] |= more["lengths"]
    if g.redo:
        more = oracle_update_partials(o, t, list(g.redo), {})
        res["popped"] += more["popped"]
        res["dirty"] |= more["dirty"]
    if g.after:
        g.after(o, t, res)
    return t, res


def make_absent_upper(o, t, v, which, res):
    """probVectUpRight (which = 1: from child 1, for child 0) or probVectUpLeft of v from the lists around it, then the child that
    sees it visited from above: what a caller of the reference does for a node that lacks the list"""
    tip = st.default_tip(t)
    p = t.up[v]
    seen = t.probVectUpRight[p] if t.children[p][0] == v else t.probVectUpLeft[p]
    if t.mutations[v]:
        seen = o.passGenomeListThroughBranch(seen, t.mutations[v], False)
    k = t.children[v][which]
    low = o.passGenomeListThroughBranch(t.probVect[k], t.mutations[k], True) if t.mutations[k] else t.probVect[k]
    new = o.shorten(o.mergeVectors(seen, t.dist[v], False, low, t.dist[k], tip[k], isUpDown=True))
    (t.probVectUpRight if which == 1 else t.probVectUpLeft)[v] = new
    more = oracle_update_partials(o, t, [(t.children[v][1 - which], 2)], {})
    res["popped"] += more["popped"]
    res["dirty"] |= more["dirty"]


def five(a, b, c, da=1e-4, db=1e-4, dc=1e-4, di=1e-4, minor=(0, 0, 0)):
    """root -> (inner, C), inner -> (A, B) with the tips' lower lists; ids TA, TB, INNER, TC, ROOT.  minor: minor sequences of A,
    B, C (a leaf with some is no tip for the merges)"""
    t = Lists()
    ta = t.add(a, da, n_minor=minor[0])
    tb = t.add(b, db, n_minor=minor[1])
    inner = t.add(None, di, kids=(ta, tb))
    tc = t.add(c, dc, n_minor=minor[2])
    t.root = t.add(None, 0.0, kids=(inner, tc))
    assert (ta, tb, inner, tc, t.root) == (TA, TB, INNER, TC, ROOT)
    return t


def thirteen(leaves, dists):
    """The thirteen-node frame of tests/search_trees.py: R -> (G, w), G -> (P, u), P -> (v, s), s -> (a, b), two leaves below u and
    below w.  leaves: the lower lists of a, b, v, u1, u2, w1, w2; dists: a length per node name.  mark: node per name.  Phase B's
    levels hold two internal nodes here (G and w, then P and u) and phase A's frontier climbs four levels."""
    t = Lists()
    m = {}
    for k, name in enumerate(("a", "b", "v", "u1", "u2", "w1", "w2")):
        m[name] = t.add(leaves[k], dists[name])
    m["s"] = t.add(None, dists["s"], kids=(m["a"], m["b"]))
    m["P"] = t.add(None, dists["P"], kids=(m["v"], m["s"]))
    m["u"] = t.add(None, dists["u"], kids=(m["u1"], m["u2"]))
    m["G"] = t.add(None, dists["G"], kids=(m["P"], m["u"]))
    m["w"] = t.add(None, dists["w"], kids=(m["w1"], m["w2"]))
    m["R"] = t.root = t.add(None, 0.0, kids=(m["G"], m["w"]))
    t.mark.update(m)
    assert t.n == 13
    return t


def _sites(ref, u, spec, n_runs=()):
    """a tip's list: {position: nucleotide} and N runs [(first, last)]"""
    b = le.Builder(ref, u)
    items = [(p, ("nuc", x)) for p, x in spec.items()] + [(s, ("n", e)) for s, e in n_runs]
    for p, (kind, x) in sorted(items):
        if kind == "nuc":
            b.nuc(p, x)
        else:
            b.run(5, p, x)
    return b.done()


def _background(rng, ref, n, taken):
    """n sites away from the hand-set one and from those taken already"""
    free = [p for p in range(20, L - 20, 7) if p not in taken and not S - 40 <= p <= S + 40]
    ps = [int(p) for p in rng.choice(free, size=n, replace=False)]
    taken.update(ps)
    return {p: le.other(rng, int(ref[p - 1])) for p in ps}


N_AT_S = [(S - 3, S + 3)]


def gadgets(o, mode, mutations=False):
    """{name: Gadget} of a model mode (the oracle must be set to it).  mutations: the same trees with a mutation list on the
    branch above INNER -- the branch above the changed node's parent, so that the lists INNER sees and hands up go through it; where
    that branch has length 0, on a leaf's -- and on the root (rootVector with the root's own list), at sites none of the leaves names.  At the hand-set site S the reference has nucleotide r and x, y
    are two others; a leaf shows x, y, r (nothing) or N there.  Two nodes that show different nucleotides at no distance have no
    merge (M:4753-4762); under an error model that holds only for leaves that are no tips (a tip's nucleotide may be an error), so
    the None gadgets give their leaves minor sequences there.

    Arms out of reach of CONSISTENT lists in the standard modes, and how the gadgets reach them all the same:
      from_parent_up{right,left}_none_*   the change comes down to INNER from the root with INNER and the merged child at length 0:
            what INNER sees from above shows a nucleotide without any length only if C is at length 0 too, and then INNER, the child
            and C are one point of the tree: if the child's list contradicted the new C, so would INNER's lower list, and the ROOT's
            lower merge -- made first, from C's side -- would be the one that comes out None (from_child_lower_none_*).  The
            recorded repairs reach these arms twice, through vectors at the thresholds.  The gadgets hand-set the child's list at
            S AFTER the lists were made (INNER's lower list is N or carries a length at S), as after a tree edit that was not
            announced; the library reads the same stale lists, so the outcome is still the same.
      from_*_raise, *_totup_none          a None over a positive length needs a substitution that cannot happen: a zero rate of Q.
            The zero-rate gadgets (zero_gadgets) reach from_child_lower_raise; in the standard modes these counters stay 0.
      from_child_lower_none_other_lengthened, from_child_upvect_none_child_lengthened     the first estimate must come back 0
            although the two lists contradict each other: a zero rate of Q again (fam_blen_none).
    from_child_upvect_none_node_lengthened lengthens INNER without addToList and remakes only probVectTotUp[INNER] and the list
    the OTHER child sees: probVectUpRight[INNER], which depends on that length too, stays as it was (M:5729-5738).  The library
    remakes it.  That gadget runs the twin again for the lengthened branch (Gadget.again).
    from_parent_*_none_child_lengthened abandons the item (INNER, from the parent) once the child is lengthened (updatedBLen,
    M:5574-5575, 5584, 5602) and what follows -- the child from above, INNER from that child -- makes the list the OTHER child sees
    only: the list the lengthened child sees keeps what it was before C changed.  The library takes INNER up again in its next round.
    Those gadgets run the abandoned item once more at the end (Gadget.redo).
    tests/test_update_trees.py checks that every gadget's finished twin is the tree rebuilt from its leaves.
    The last two gadgets stand on the thirteen-node frame (thirteen())."""
    ref = le.reference()
    u = bool(le.model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(400 + le.MODES.index(mode))
    x, y = [n for n in range(4) if n != int(ref[S - 1])][:2]
    taken = set()
    base = _background(rng, ref, 10, taken)
    own = {k: _background(rng, ref, 4, taken) for k in "abc"}
    hard = (1, 1, 1) if u else (0, 0, 0)
    out = {}

    def leaf(k, s=None, n=(), own_sites=True):
        return _sites(ref, u, {**base, **(own[k] if own_sites else {}), **({S: s} if s is not None else {})}, n)

    def bare(k, s=None, n=()):                                          # (leaves at no distance from each other share every other site)
        return leaf(k, s, n, own_sites=False)

    muts = [[], []]
    if mutations:                                                       # (below such a branch the frame is the genome's own reference)
        ps = [int(p) for p in rng.choice([p for p in range(30, L - 30, 13) if not S - 40 <= p <= S + 40], size=6, replace=False)]
        muts = [sorted(le.mutation(ref, p, True, le.other(rng, int(ref[p - 1]))) for p in ps[k::2]) for k in (0, 1)]

    def tree(*args, mut_on=INNER, **kw):                                 # (mut_on: a branch that is not of length 0; None: the root only)
        t = five(*args, **kw)
        if mut_on is not None:
            assert t.dist[mut_on] > 0.0
            t.mutations[mut_on] = [tuple(m) for m in muts[0]]
        t.mutations[ROOT] = [tuple(m) for m in muts[1]]
        return consistent(o, t)

    def changed(t, node=TA, new=None, dist=None):
        g = t.copy()
        if new is not None:
            g.probVect[node] = [tuple(e) for e in new]
        if dist is not None:
            g.dist[node] = float(dist)
        return g

    def add(name, *args, **kw):
        out[name] = Gadget(name, *args, **kw)

    # -- the plain repair: a tip's list changes at a site nobody else names; the change travels to the root (rootVector) and down
    t = tree(leaf("a"), leaf("b"), leaf("c"))
    add("plain_tip", changed(t, new=leaf("a", x)), TA, arms=("from_child_at_root",), stats=dict(root_left_made=1, items_mode0=2, items_mode2=1))
    add("plain_dist", changed(t, dist=3e-4), TA, arms=("from_child_at_root",), stats=dict(items_mode0=2))
    # -- nothing changed: the repair stops at INNER, whose lower list and whose list for B come out as they were
    add("no_change", changed(t), TA, arms=("stop_lower_same", "stop_upper_same"), stats=dict(items_mode0=1, items_mode2=1))
    # -- nothing changed at C, the root's own child: the root's lower list and rootVector of C come out as they were, the root's
    #    upper list is kept (rootLevel with one of its two children marked and "same")
    add("no_change_at_root", changed(t), TC, arms=("stop_lower_same", "stop_upper_same", "from_child_at_root"), stats=dict(root_kept=1),
        never=("root_right_made", "root_left_made"))
    # -- the change comes from C: ROOT hands it down to INNER, which hands it on to A and B (the from-parent direction at an
    #    internal node)
    add("from_above", changed(t, node=TC, new=leaf("c", x)), TC, arms=("from_child_at_root",), stats=dict(root_right_made=1, items_mode2=2))
    # -- A at no distance from INNER: probVectTotUp of A is absent over length 0
    t0 = tree(leaf("a"), leaf("b"), leaf("c"), da=0.0)
    add("zero_len_tip", changed(t0, new=leaf("a", x)), TA, arms=("from_parent_totup_zero_len", "from_child_at_root"), stats=dict(totup_cleared=1))
    # -- INNER lacks the list its other child sees / its own lower list, as after a tree edit.  The reference leaves an absent upper
    #    list absent and does not visit the child that would see it (M:5722, 5798); the library makes it (there is no old list to
    #    be the same as) and goes on to that child.  The twin is finished by hand in that one place (make_absent_upper).
    g = changed(t0, new=leaf("a", x))
    g.probVectUpLeft[INNER] = None
    add("upper_absent", g, TA, arms=("other_upper_absent",), after=lambda oo, tt, res: make_absent_upper(oo, tt, INNER, 0, res))
    g = changed(t0, new=leaf("a", x))
    g.probVect[INNER] = None
    add("lower_absent", g, TA, arms=("old_lower_absent",), stats=dict(items_old_absent=1))
    # -- A and B with 257-600 entries: the wavefront kernel hands INNER's item (and those of A's and B's upper lists) to lane 0
    la, lb, la2 = (le.random_list(rng, ref, u, n, tails=False, flags=False) for n in (280, 300, 290))
    assert all(257 <= len(gl) <= 600 for gl in (la, lb, la2)), [len(gl) for gl in (la, lb, la2)]
    tl = tree(la, lb, leaf("c"))
    add("long_lists", changed(tl, new=la2), TA, arms=("from_child_at_root",), stats=dict(items_mode0=2))
    # -- minor sequences on leaf A: it is no tip for the merges
    tm = tree(leaf("a"), leaf("b"), leaf("c"), minor=(2, 0, 0))
    add("minor_leaf", changed(tm, new=leaf("a", x)), TA, arms=("from_child_at_root",))
    # -- a lower merge that is None between two zero-length branches: A (now x) against B (y), both at INNER; updateBLen gives A
    #    a length and the list is made again
    t = tree(bare("a", y), bare("b", y), bare("c"), da=0.0, db=0.0, minor=hard)
    add("lower_none_child", changed(t, new=bare("a", x)), TA, arms=("from_child_lower_none_child_lengthened",),
        stats=dict(phaseA_none=1, phaseA_reest_first=1), never=("phaseA_reest_second",))
    # -- the same with B the changed child: the branch above the CHANGED child is estimated first, whichever child it is (estimating
    #    A's first finds no length, B's is estimated all the same and the lists come out alike: only the counters tell)
    add("lower_none_second_child", changed(t, node=TB, new=bare("b", x)), TB, arms=("from_child_lower_none_child_lengthened",),
        stats=dict(phaseA_none=1, phaseA_reest_first=1), never=("phaseA_reest_second",))
    # -- the lower merge at INNER is fine (B is N at S), but A (x, length 0) contradicts what INNER (length 0) sees from above: C
    #    (y, length 0).  The twin meets it in INNER's list for B; the library one level up, in ROOT's lower merge.  Both lengthen INNER.
    t = tree(bare("a", y), bare("b", None, N_AT_S), bare("c", y), da=0.0, db=1e-4, dc=0.0, di=0.0, minor=hard, mut_on=TB)
    add("upvect_none_node", changed(t, new=bare("a", x)), TA, arms=("from_child_upvect_none_node_lengthened",),
        stats=dict(phaseA_none=1, phaseA_reest_first=1), again=True)
    # -- the upper None arms (hand-set, see above): C changes to x at length 0; INNER at length 0; the child K merged with what
    #    INNER sees is at length 0 and hand-set to y.  *_child: INNER's lower list is N at S (the other child is), INNER's new length
    #    comes back 0 and K is lengthened; *_node: the other child shows y over a length, INNER's lower list with it, and INNER is
    #    lengthened.
    for side, kid in (("upright", TB), ("upleft", TA)):
        oth = "a" if kid == TB else "b"
        kk = "b" if kid == TB else "a"
        for what, s_other in (("child", None), ("node", y)):
            lists = {kk: bare(kk, None, N_AT_S), oth: bare(oth, s_other, () if s_other is not None else N_AT_S), "c": bare("c")}
            d = dict(da=0.0 if kid == TA else 1e-4, db=0.0 if kid == TB else 1e-4)
            t = tree(lists["a"], lists["b"], lists["c"], dc=0.0, di=0.0, minor=hard, mut_on=TA if kid == TB else TB, **d)
            g = changed(t, node=TC, new=bare("c", x))
            g.probVect[kid] = [tuple(e) for e in bare(kk, y)]
            add(f"parent_{side}_none_{what}", g, TC, arms=(f"from_parent_{side}_none_{what}_lengthened",),
                stats={"rounds": 2, f"upper_none_{side}": 1, "upper_reest_node": 1, **({"upper_reest_child": 1} if what == "child" else {})},
                python_loop_raises=True, redo=[(INNER, 2)] if what == "child" else (), complete=what == "child")
    # -- both children of INNER hand-set to y at length 0: both upper merges of INNER's level are None.  The reference gives up the
    #    item at the first (B is lengthened) and never makes the second; the library's level has both items, the first one deals with
    #    INNER and the second is skipped (`deferred`).  With B lengthened INNER's lower list shows y without a length (A), against C's
    #    x: ROOT's lower merge is None between two zero-length branches and INNER is lengthened too.
    t = tree(bare("a", None, N_AT_S), bare("b", None, N_AT_S), bare("c"), da=0.0, db=0.0, dc=0.0, di=0.0, minor=hard, mut_on=None)
    g = changed(t, node=TC, new=bare("c", x))
    g.probVect[TA], g.probVect[TB] = [tuple(e) for e in bare("a", y)], [tuple(e) for e in bare("b", y)]
    add("parent_both_none", g, TC, arms=("from_parent_upright_none_child_lengthened", "from_child_lower_none_child_lengthened"),
        stats=dict(rounds=2, upper_none_upright=1, upper_none_upleft=1, upper_deferred_skip=1, upper_reest_node=1, upper_reest_child=1,
                   phaseA_none=1), python_loop_raises=True, redo=[(INNER, 2)])
    # -- the thirteen-node frame: a change at the deepest leaf climbs four levels and comes down through levels of two internal
    #    nodes; a change at a leaf below w comes down the other side
    names = ("a", "b", "v", "u1", "u2", "w1", "w2")
    own13 = {k: _background(rng, ref, 3, taken) for k in names}
    # (only a and w1 say anything at S, the other leaves are N there: what changes at S is not outvoted on the way up)
    lf = lambda k, s=None: _sites(ref, u, {**base, **own13[k], **({S: s} if s is not None else {})},     # noqa: E731
                                  () if k in ("a", "w1") else N_AT_S)
    dists = dict(a=1e-4, b=2e-4, v=1e-4, u1=3e-4, u2=1e-4, w1=2e-4, w2=1e-4, s=1e-4, P=2e-4, u=1e-4, G=1e-4, w=3e-4)
    t13 = thirteen([lf(k) for k in names], dists)
    t13.mutations[t13.mark["G"]], t13.mutations[t13.root] = [tuple(m) for m in muts[0]], [tuple(m) for m in muts[1]]
    t13 = consistent(o, t13)
    for name, leaf_name in (("deep_tip", "a"), ("deep_other_side", "w1")):
        v = t13.mark[leaf_name]
        add(name, changed(t13, node=v, new=lf(leaf_name, x)), v, arms=("from_child_at_root",), stats=dict(items_mode0=2, items_mode2=6))
    return out


def zero_gadgets(o, mode):
    """The gadgets of the two zero-rate modes (le.Q_ZERO: A -> C and G -> T cannot happen), at a site Z whose reference is G or T;
    fr = A, to = C.
      no_change          a consistent tree, nothing changed: the call that must succeed after a fatal one
      lower_raise        B shows fr at length 0, A's new list shows `to` over a positive length: no merge although a length is not
                         zero.  The twin raises where the reference does (M:5695-5697); the library returns MAPLE_ERR_FATAL.
      upper_raise        the same in the upper pass (M:5581-5583): C changes to fr at length 0, INNER at length 0, B hand-set to
                         `to` over a positive length (INNER's lower list is N at Z: see gadgets() on hand-set children)
    Arms no gadget reaches, in any mode, and why (the tests assert that they stay 0):
      from_child_lower_none_other_lengthened    the first estimate must find no length between two lists that contradict each other at
                         no distance.  estimateBranchLengthWithDerivative sees a zero rate only where the upper list's entry carries
                         lengths (M:5171-5172, 5241-5242) or, under an error model, a flag (M:5178-5179); the entry of a leaf at
                         length 0 carries neither, and against a tail-less entry the estimate is about 1 / lRef (measured: 6.67e-4)
      from_child_upvect_none_child_lengthened   INNER and A at length 0 and both estimates without a length: the reference pushes the
                         same two items again and never ends (here: the library's cap of 64 rounds)
      from_parent_totup_none, from_child_totup_none   a None probVectTotUp over a positive length d means the two sides cannot be
                         joined over d, so the estimate of that branch finds no length either, the second merge is None as well
                         and the reference fails in shorten(None)
      from_child_upvect_raise   what INNER sees shows fr without any length only if C is at length 0 with INNER: the library meets
                         the contradiction one level up, in ROOT's lower merge between two zero-length branches, and re-estimates
                         where the reference raises -- the two go different ways by design (update_plan.h), nothing to compare"""
    assert mode.startswith("zeroq")
    ref = le.reference()
    u = bool(le.model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(400 + le.MODES.index(mode))
    fr, to = le.ZERO_RATES[0]
    Z = next(p for p in range(S, S + 40) if int(ref[p - 1]) in (2, 3))
    taken = {Z}
    base = _background(rng, ref, 10, taken)
    hard = (1, 1, 1) if u else (0, 0, 0)
    n_at_z = [(Z - 2, Z + 2)]

    def leaf(s=None, n=()):
        return _sites(ref, u, {**base, **({Z: s} if s is not None else {})}, n)

    def tree(*args, **kw):
        return consistent(o, five(*args, minor=hard, **kw))

    out = {}
    t = tree(leaf(fr), leaf(fr), leaf(), da=1e-4, db=0.0)
    out["no_change"] = Gadget("no_change", t.copy(), TA, arms=("stop_lower_same",))
    g = t.copy()
    g.probVect[TA] = [tuple(e) for e in leaf(to)]
    out["lower_raise"] = Gadget("lower_raise", g, TA, arms=("from_child_lower_raise",), raises=f"node {INNER}")
    t = tree(leaf(None, n_at_z), leaf(None, n_at_z), leaf(), da=1e-4, db=1e-4, dc=0.0, di=0.0)
    g = t.copy()
    g.probVect[TC] = [tuple(e) for e in leaf(fr)]
    g.probVect[TB] = [tuple(e) for e in leaf(to)]
    out["upper_raise"] = Gadget("upper_raise", g, TC, arms=("from_parent_raise",), raises=f"node {INNER}", python_loop_raises=True)
    return out


# ---- a library's repair against the twin's ------------------------------------------------------------------------------------------
ATTRS = dict(probVect="id_lower", probVectUpRight="id_upRight", probVectUpLeft="id_upLeft", probVectTotUp="id_totUp")


def deviation(got, want):
    """the largest relative difference between the doubles of two lists of the same structure"""
    worst = 0.0
    for a, b in zip(got, want):
        for x, y in zip(a[2:], b[2:]):
            for p, q in zip(*((x, y) if isinstance(x, list) else ([x], [y]))):
                if not isinstance(p, bool) and p != q:
                    worst = max(worst, abs(p - q) / max(abs(p), abs(q)))
    return worst


def repaired_by_library(dev, before, changed, native=True):
    """the library's repair (maple_update_partials, or the Python level loop of tree_host) of a copy of the tree on `dev`: the
    HostTree afterwards.  Raises what the loop raises."""
    from maple_amd.tree_host import update_genome_lists
    host = before.copy().host_tree().upload(dev)
    host.replaced = update_genome_lists(dev, host, [changed], native=native)
    return host


def compare_with_twin(dev, o, host, twin, before, rel, worst=None, tag=""):
    """The bars of a repaired tree against the twin's: the same branch lengths changed, to `rel`; every list of every node equal
    to shorten(the twin's) -- shorten because of the reference's unshortened re-merges -- in structure and to `rel`, and "same" for
    areVectorsDifferent both ways round on `dev`; absent lists absent on both sides.  worst: a dict that receives the largest
    deviation per field."""
    from golden_util import close, lists_match
    worst = {} if worst is None else worst
    nodes = twin.reachable()
    moved = {v for v in nodes if twin.dist[v] != before.dist[v]}
    assert moved == {v for v in nodes if float(host.dist[v]) != before.dist[v]}, (tag, moved, list(host.dist), before.dist)
    for v in nodes:
        assert close(float(host.dist[v]), twin.dist[v], rel), (v, host.dist[v], twin.dist[v])
        if twin.dist[v]:
            worst["dist"] = max(worst.get("dist", 0.0), abs(float(host.dist[v]) - twin.dist[v]) / twin.dist[v])
    for key, attr in ATTRS.items():
        ids = getattr(host, attr)
        have = [v for v in nodes if getattr(twin, key)[v] is not None]
        assert all(ids[v] < 0 for v in nodes if v not in have), (key, [v for v in nodes if v not in have and ids[v] >= 0])
        assert all(ids[v] >= 0 for v in have), (key, [v for v in have if ids[v] < 0])
        want = [o.shorten(getattr(twin, key)[v]) for v in have]
        got = dev.download(ids[have])
        for v, g, w in zip(have, got, want):
            assert lists_match(g, w, rel), (tag, key, v, g, w)
            worst[key] = max(worst.get(key, 0.0), deviation(g, w))
        want_ids = dev.upload(want)
        differ = dev.differ_batch(ids[have], want_ids) | dev.differ_batch(want_ids, ids[have])
        assert not differ.any(), (tag, key, [have[i] for i in np.nonzero(differ)[0]])
    return worst


def twin_lk(o, t):
    _, contrib, root = st.oracle_tree_lk(o, t)
    total = 0.0
    for x in contrib:
        total += x
    return total + root


# ---- the fused item kernels on list_edges.fam_update_items --------------------------------------------------------------------------
ITEM_REL = 1e-9
LANE_OVER = 4096                                                   # update_items: more items than this go one lane per item


def same_packed(dev, ids_a, ids_b):
    """Two sets of device lists are the same words and the same doubles, bit for bit."""
    a, b = dev.download_packed(ids_a), dev.download_packed(ids_b)
    return (all(np.array_equal(getattr(a, k), getattr(b, k)) for k in ("ent_off", "pos", "meta", "aux_off"))
            and np.array_equal(a.aux.view(np.uint64), b.aux.view(np.uint64)))


def item_shapes(lists, items):
    """the shapes the kernels cut their work along, as the family has them: {name: present?}"""
    n1 = {len(lists[it["i1"]]) for it in items}
    n2 = {len(lists[it["i2"]]) for it in items}
    n_old = {len(lists[it["iold"]]) for it in items if it["iold"] >= 0}
    merged = {len(it["m"]) for it in items if it["m"] is not None}
    names = {it["name"][0][0] if it["name"][0][0] != "shape_none" else it["name"][0] for it in items}
    out = {f"n1={n}": n in n1 for n in le.UPDATE_SIZES}
    out.update({f"n2={n}": n in n2 for n in le.UPDATE_SIZES})
    out.update({f"nOld={n}": n in n_old for n in (512, 513)})
    out["old absent"] = any(it["iold"] < 0 for it in items)
    out.update({f"merged={n}": n in merged for n in le.UPDATE_MERGED})
    out["merged>=449"] = max(merged) >= 449
    for nm in ("shape_ties", "shape_ties_updown", "shape_absorb_three_chunks", "shape_O_straddle"):
        out[nm] = nm in names
    for where in ("first", "middle", "last", "two_in_a_chunk"):
        out[f"none at {where}"] = ("shape_none", where) in names
    # a run with distances whose first entry lies in the chunk of 64 entries before the entry decided, and a refusal on the head
    heads = {it["name"][0][1][1] for it in items if it["name"][0][0] == "shorten" and it["name"][0][1][0] == "head"}
    out["run across entry 64"] = {62, 63} <= heads
    out["run across entry 128"] = {126, 127} <= heads
    return out


def check_items(dev, o, mode, fam, fused=True, forms=True, worst=None):
    """Every item of the family in the three modes.  The chain maple_merge_batch -> maple_shorten_batch -> maple_differ_batch against
    the oracle (None flags and structure exact, doubles to ITEM_REL, the verdict exact where the oracle's is stable under +-1e-9);
    fused: maple_debug_update_items against that chain bit for bit, in every form; the arena's list count comes back."""
    from golden_util import lists_match
    worst = {} if worst is None else worst
    lists, items = fam
    n = len(items)
    assert n <= LANE_OVER
    u = bool(le.model(mode).get("usingErrorRate"))
    count0 = dev.stats()["n_lists"]
    mark = dev.mark()
    ids = dev.upload(lists)
    col = lambda k, dt=None: np.asarray([it[k] for it in items], dtype=dt)          # noqa: E731
    l1, l2, iold = ids[col("i1")], ids[col("i2")], col("iold")
    old = np.where(iold >= 0, ids[np.maximum(iold, 0)], -1).astype(np.int32)
    b1, b2, t1, t2, ud = col("b1"), col("b2"), col("t1", np.uint8), col("t2", np.uint8), col("ud", np.uint8)
    reps = LANE_OVER // n + 1
    tile = np.tile(np.arange(n), reps)
    seen_verdicts = set()
    for md in (0, 1, 2):
        expect = [le.update_item_expect(o, it, None if it["iold"] < 0 else lists[it["iold"]], md) for it in items]
        stable = [md == 1 or it["iold"] < 0 or it["m"] is None or not it["threshold"] or le.verdict_stable(o, it, lists[it["iold"]], md)
                  for it in items]
        m_ids = dev.merge_batch(l1, b1, t1, l2, b2, t2, ud)
        ok = m_ids >= 0
        s_ids = np.full(n, -1, np.int32)
        s_ids[ok] = dev.shorten_batch(m_ids[ok])
        verdict = np.ones(n, bool)
        cmp = ok & (old >= 0)
        if md == 0:
            verdict[cmp] = dev.differ_batch(s_ids[cmp], old[cmp])
        elif md == 2:
            verdict[cmp] = dev.differ_batch(old[cmp], m_ids[cmp])
        chain = np.where(ok & (verdict | (md != 2)), s_ids, -1).astype(np.int32)
        got = dev.download(chain)
        for k, it in enumerate(items):
            want, none, flag = expect[k]
            assert (not ok[k]) == none, (it["name"], md)
            if stable[k]:
                assert bool(verdict[k]) == flag, (it["name"], md, verdict[k], flag)
                assert lists_match(got[k], want, ITEM_REL), (it["name"], md, got[k], want)
                if want is not None:
                    worst["item lists"] = max(worst.get("item lists", 0.0), deviation(got[k], want))
            else:                                                       # the verdict hangs on rounding: either answer, and the list that goes with it
                assert lists_match(got[k], it["s"] if (md != 2 or verdict[k]) else None, ITEM_REL), (it["name"], md)
            seen_verdicts.add((md, flag))
        if not fused:
            continue
        good = chain >= 0
        res = []
        for form in ("wave", "lane", "tiled") if forms else ("wave",):
            dev.set_tuning(wave_per_item_max=-1 if form == "lane" else 0)
            idx = tile if form == "tiled" else np.arange(n)
            out, none, diff = dev.debug_update_items(l1[idx], b1[idx], t1[idx], l2[idx], b2[idx], t2[idx], ud[idx], md, old[idx])
            dev.set_tuning()
            for lo in ((0, (reps - 1) * n) if form == "tiled" else (0,)):
                sl = slice(lo, lo + n)
                assert np.array_equal(none[sl], ~ok), (form, md, [items[k]["name"] for k in np.nonzero(none[sl] != ~ok)[0]][:5])
                assert np.array_equal(diff[sl], verdict), (form, md, [items[k]["name"] for k in np.nonzero(diff[sl] != verdict)[0]][:5])
                assert np.array_equal(out[sl] >= 0, good), (form, md, [items[k]["name"] for k in np.nonzero((out[sl] >= 0) != good)[0]][:5])
                assert same_packed(dev, out[sl][good], chain[good]), (form, md)
            res.append(form)
        assert len(res) == (3 if forms else 1)
    dev.release(mark)
    assert dev.stats()["n_lists"] == count0
    assert seen_verdicts >= {(0, True), (0, False), (2, True), (2, False), (1, True)}
    return u
