"""An oracle twin of the branch-length sweep (traverseTreeToOptimizeBranchLengths, M:8727-8889) with one counter per place the
function can go, and small trees that send the sweep into the arms real, nearly converged trees do not take.

A helper module like update_trees.py, on which it stands.  The twin works on tuple lists (update_trees.Lists) and calls nothing
but the C oracle (oracle/oracle_py.py) and update_trees.oracle_update_partials:

  oracle_optimize_blens(o, tree, dirty, effectivelyNon0BLen, fastPass, counts, log=None, watch=None)
        one call of the reference's function without `testing`, HnZ and time trees.  The root's two branches first: the grid of
        half-mutation steps over their total length (mergeVectors with returnLK, the pass through the root's own mutation list,
        findProbRoot; Python's round(): half to even; the first strict maximum wins), then both children repaired whether they
        moved or not, each with the reference's own work list [(child, 2), (root, 0)] -- also for the SECOND child (M:8796).
        Then every other branch in the reference's LIFO order: estimateBranchLengthWithDerivative of what the parent shows the
        node (through the node's mutation list), Python's truthiness of `False` / 0.0, the 1 % rule, and after every change the
        repair [(node, 2), (up, child)] at once.  `dirty` (a list of bool) is read at a node's turn, cleared where the length is
        kept and set for every node a repair pops or re-estimates; it is changed in place, like the tree.  Where the reference
        raises (a grid merge that is None or underflows, a repair that raises) the twin raises SweepError; the order swap of the
        root step's `except:` (M:8798-8810) is counted (root_step_raises) and not made -- the library returns MAPLE_ERR_FATAL there.
        counts: a dict that receives the counters of ARMS.  log: a list that receives (arm, node).  watch: a dict that receives
        "ratios" -- every dist / bestLength the 1 % rule saw -- and "grids" -- the (cost, bLen1) of every grid point.
        Returns dict(updates, order, dirty, dist): the return value, the nodes handed to a repair in order (fastPass: whose length
        changed), the flags and the lengths afterwards.

The gadgets (gadgets(o, mode, mutations)) stand on update_trees.five and update_trees.thirteen over lRef = le.L_REF.  Each states the
arms it is built for; tests/test_sweep_trees.py checks that it takes them and that none of its verdicts hangs on rounding.
"""
import math

import numpy as np

import list_edges as le
import sink_trees as st
import update_trees as ut

ARMS = ("root_no_children", "root_grid_skipped", "root_grid_run", "root_grid_round_half_even", "root_grid_equal_costs",
        "root_grid_clamped_steps", "root_child_mutations", "root_mutations", "root_child_unmoved_repaired", "root_best2_clamped",
        "root_step_raises", "node_clean", "est_false_len_zero", "est_false_len_positive", "est_positive_len_zero", "est_tenth",
        "within_one_percent", "moved", "node_mutations", "tip_with_minor_sequences")


class SweepError(RuntimeError):
    """where the reference's sweep raises"""


def oracle_optimize_blens(o, tree, dirty, effectivelyNon0BLen, fastPass, counts, log=None, watch=None):
    ch, up, dist, mut = tree.children, tree.up, tree.dist, tree.mutations
    low, ur, ul = tree.probVect, tree.probVectUpRight, tree.probVectUpLeft
    tip = st.default_tip(tree)
    root, lRef, eff = tree.root, float(o.lRef), float(effectivelyNon0BLen)
    order, repair_arms = [], {}
    updates = 0

    def arm(name, node=None):
        assert name in ARMS
        counts[name] = counts.get(name, 0) + 1
        if log is not None:
            log.append((name, node))

    def result():
        return dict(updates=updates, order=order, dirty=dirty, dist=dist, repair_arms=repair_arms)

    def repair(node_list):
        res = ut.oracle_update_partials(o, tree, node_list, repair_arms)
        for v in set(res["popped"]) | res["dirty"]:
            dirty[v] = True

    if not ch[root]:
        arm("root_no_children", root)
        return result()
    c1, c2 = ch[root]
    if dist[c1] > eff or dist[c2] > eff:                                # ---- the root's two branches, M:8746-8810
        arm("root_grid_run", root)
        tot = (dist[c1] + dist[c2]) * lRef
        pv = []
        for c in (c1, c2):
            if low[c] is None:
                raise SweepError(f"node {c} (a child of the root) has no lower list")
            if mut[c]:
                arm("root_child_mutations", c)
                pv.append(o.passGenomeListThroughBranch(low[c], mut[c], True))
            else:
                pv.append(low[c])
        if mut[root]:
            arm("root_mutations", root)
        steps = round(tot)                                              # (Python's: half to even)
        if steps != math.floor(tot + 0.5):
            arm("root_grid_round_half_even", root)
        grid, clamped = [], 0
        best_cost, best1 = float("-inf"), None
        for i in range(max(1, steps) * 2 + 1):
            clamped += float(i) / 2 > tot
            b1 = min(tot, float(i) / 2)
            b2 = max(tot - b1, 0.0)
            b1, b2 = b1 / lRef, b2 / lRef
            try:
                res = o.mergeVectors(pv[0], b1, tip[c1], pv[1], b2, tip[c2], returnLK=True)
            except RuntimeError as err:
                raise SweepError(f"the root grid's merge fails at step {i}: {err}")
            if res is None:
                raise SweepError(f"None root vector in the root branch-length grid at step {i}")
            vec, cost = res
            if mut[root]:
                vec = o.passGenomeListThroughBranch(vec, mut[root], True)
            cost += o.findProbRoot(vec, [])
            grid.append((cost, b1))
            if cost > best_cost:
                best_cost, best1 = cost, b1
        if clamped:
            arm("root_grid_clamped_steps", root)
        if watch is not None:
            watch.setdefault("grids", []).append(grid)
        if best1 is None:
            raise SweepError("no finite likelihood in the root branch-length grid")
        if len({b for c, b in grid if c == best_cost}) > 1:
            arm("root_grid_equal_costs", root)
        best2 = dist[c1] + dist[c2] - best1
        if best2 < 0.0:
            arm("root_best2_clamped", root)
        best2 = max(best2, 0.0)
        try:
            for c, new in ((c1, best1), (c2, best2)):
                moved = dist[c] != new
                dist[c] = new
                if fastPass:
                    if moved:
                        order.append(c)
                    continue
                if not moved:
                    arm("root_child_unmoved_repaired", c)
                order.append(c)
                repair([(c, 2), (root, 0)])                             # (root, 0) for both children: M:8790, 8796
        except ut.RepairError as err:
            arm("root_step_raises", root)
            raise SweepError(f"the repair of the root's branches raises: {err}")
    else:
        arm("root_grid_skipped", root)
    stack = list(ch[c1]) + list(ch[c2])                                 # ---- every other branch, M:8812-8885
    while stack:
        node = stack.pop()
        if dirty[node]:
            p = up[node]
            child = 0 if ch[p][0] == node else 1
            vect = ur[p] if child == 0 else ul[p]
            if vect is None or low[node] is None:
                raise SweepError(f"node {node}: a list of its estimate is None")
            if mut[node]:
                arm("node_mutations", node)
                vect = o.passGenomeListThroughBranch(vect, mut[node], False)
            if not ch[node] and not tip[node]:
                arm("tip_with_minor_sequences", node)
            best = o.estimateBranchLengthWithDerivative(vect, low[node], tip[node])
            if best is not False and best == 0.1:
                arm("est_tenth", node)
            if not best:
                arm("est_false_len_positive" if dist[node] else "est_false_len_zero", node)
            if best or dist[node]:
                if best and dist[node] and watch is not None:
                    watch.setdefault("ratios", []).append((node, dist[node] / best))
                if (not best) or (not dist[node]) or dist[node] / best > 1.01 or dist[node] / best < 0.99:
                    if best:
                        arm("moved" if dist[node] else "est_positive_len_zero", node)
                    dist[node] = float(best) if best else 0.0           # (the reference stores False: the same number everywhere)
                    updates += 1
                    order.append(node)
                    if not fastPass:
                        repair([(node, 2), (p, child)])
                else:
                    arm("within_one_percent", node)
                    dirty[node] = False
            else:
                dirty[node] = False
        else:
            arm("node_clean", node)
        stack.extend(ch[node])
    return result()


# ---- the gadgets ----------------------------------------------------------------------------------------------------------------------
EFF = 1e-8                                                        # effectivelyNon0BLen of every gadget sweep
TA, TB, INNER, TC, ROOT = ut.TA, ut.TB, ut.INNER, ut.TC, ut.ROOT
L = le.L_REF


class SweepGadget:
    """tree: the tree going in (consistent lists unless the gadget says otherwise); dirty: the flags going in (None: all set);
    arms: the twin's counters the gadget is built for; raises: a piece of the library's message where the twin raises SweepError and
    the library returns MAPLE_ERR_FATAL; equal_costs: the gadget built for two grid points of the same cost (no margin is asked)"""

    def __init__(self, name, tree, arms=(), dirty=None, raises=None, equal_costs=False):
        self.name, self.tree, self.arms, self.raises, self.equal_costs = name, tree, tuple(arms), raises, equal_costs
        self.dirty = [True] * tree.n if dirty is None else [bool(x) for x in dirty]


def clear_of_rounding(g, ratios, grids):
    """no verdict hangs on rounding: every dist / bestLength the 1 % rule saw is far outside the rule's window or in its very middle,
    and the grid's best cost beats the runner-up by far more than fp64 noise (costs are sums of a few thousand terms of magnitude up
    to 1e3: noise below 1e-9) or -- the gadget built for it -- equals it as a double at another grid point"""
    if any(not (r < 0.9 or r > 1.1 or 0.999 <= r <= 1.001) for _, r in ratios):
        return False
    for grid in grids:
        costs = sorted({c for c, _ in grid}, reverse=True)
        tied = len({b for c, b in grid if c == costs[0]}) > 1
        if (not tied) if g.equal_costs else (len(costs) > 1 and costs[0] - costs[1] <= 1e-8):
            return False
    return True


def sweeps_to_compare(o, g, fastPass):
    """2 where the gadget's SECOND sweep, from the flags the first left, stays clear of rounding too, else 1: after one sweep a
    perturbed tree is nearly converged, with quotients anywhere between 0.99 and 1.01"""
    watch = {}
    run_twin(o, g, fastPass=fastPass, watch=watch, sweeps=2)
    return 2 if clear_of_rounding(g, watch.get("ratios", []), watch.get("grids", [])) else 1


def run_twin(o, g, fastPass=False, counts=None, watch=None, sweeps=1):
    """the twin on a copy of the gadget's tree, `sweeps` calls in a row from the flags the call before left:
    (tree after, [result per call]); raises SweepError"""
    t = g.tree.copy()
    dirty = list(g.dirty)
    counts = {} if counts is None else counts
    out = []
    for _ in range(sweeps):
        res = oracle_optimize_blens(o, t, dirty, EFF, fastPass, counts, watch=watch)
        out.append(dict(updates=res["updates"], order=list(res["order"]), dirty=list(dirty), dist=list(t.dist)))
    return t, out


SECOND_SWEEP = ("converged", "false_zero", "tenth", "lone_root")


def settled(o, tree, rounds=4):
    """a copy of the tree after three times a sweep of the twin (the root's two branches settle on a grid point) followed by `rounds`
    rounds in which every swept branch is set to its own estimate and the lists are repaired"""
    t = tree.copy()
    for _ in range(3):
        oracle_optimize_blens(o, t, [True] * t.n, EFF, False, {})
        _settle_rounds(o, t, rounds)
    return t


def _settle_rounds(o, t, rounds):
    tip = st.default_tip(t)
    kids = set(t.children[t.root])
    nodes = [v for v in t.reachable() if v != t.root and v not in kids]
    for _ in range(rounds):
        for v in nodes:
            p = t.up[v]
            child = 0 if t.children[p][0] == v else 1
            vect = t.probVectUpRight[p] if child == 0 else t.probVectUpLeft[p]
            if t.mutations[v]:
                vect = o.passGenomeListThroughBranch(vect, t.mutations[v], False)
            best = o.estimateBranchLengthWithDerivative(vect, t.probVect[v], tip[v])
            t.dist[v] = float(best) if best else 0.0
            ut.oracle_update_partials(o, t, [(v, 2), (p, child)], {})


# where the last point of grid_best2_clamped's grid wins (elsewhere the gadget is one more clamped grid)
BEST2_CLAMPED = (("jc", True), ("unrest", False), ("ratevar", False), ("ratevar", True))


def overshooting_total(lo=2.55):
    """two lengths d1, d2 whose total is clamped at the grid's last point (round(tot) > tot) and comes back from the grid one ulp
    longer: fl(fl((d1 + d2) * lRef) / lRef) > d1 + d2"""
    for k in range(1, 200000):
        t0 = lo + k * 1.7e-6
        d1, d2 = 0.62 * t0 / L, 0.38 * t0 / L
        tot = (d1 + d2) * float(L)
        if tot / float(L) > d1 + d2 and round(tot) > tot:
            return d1, d2
    raise AssertionError("no such pair")


def gadget_names(mode, mutations):
    """the names gadgets() gives for a mode: known without an oracle, for parametrised tests"""
    names = ["perturbed", "converged", "false_positive", "false_zero", "zero_to_positive", "tenth", "minor_leaf", "grid_skipped",
             "partly_clean", "grid_half_even", "grid_best2_clamped", "grid_clamped"]
    if not le.model(mode).get("usingErrorRate") and not mutations:
        names.append("grid_equal")
    return names + ["lone_root", "thirteen_perturbed"]


def exact_total(target, share=0.4):
    """two lengths whose sum times lRef is exactly `target` substitutions as doubles"""
    for k in range(1, 4000):
        a = (target * share + k * 1e-3) / L
        b = target / L - a
        if a > 0 and b > 0 and (a + b) * float(L) == target:
            return a, b
    raise AssertionError(target)


def gadgets(o, mode, mutations=False):
    """{name: SweepGadget} of a standard model mode (the oracle must be set to it); mutations: mutation lists on the branches above
    a swept leaf, above INNER (a child of the root) and on the root, at sites no leaf names.
    Five-node trees root -> (INNER, C), INNER -> (A, B): the sweep's grid works on INNER and C, its loop visits B, then A.
      perturbed         every length far from its optimum: both leaves move, each repair changes what the other sees
      converged         `perturbed` with every length set to its own estimate until nothing moves (settled()): every estimate
                        within 0.1 % of the length; the second sweep finds A and B clean
      false_positive    A shows nothing its parent does not: the estimate is False over a length, which goes to 0
      false_zero        the same at length 0: nothing changes
      zero_to_positive  A differs from its parent at length 0
      tenth             A and what INNER shows it are list_edges.fam_blen_tenth's pair: the early 0.1
      minor_leaf        A has minor sequences: isTip is false on a leaf
      grid_skipped      both root branches at length 0
      partly_clean      the same with A's flag cleared: A keeps a length that is far from its estimate
      grid_half_even    the root's branches are 2.5 substitutions long together: round() gives 2, five grid points
      grid_best2_clamped  2.55 substitutions, C bare: where the grid's last point wins (BEST2_CLAMPED) the first branch takes the whole
                        total, which times lRef and divided by lRef again is one ulp more than the two lengths together, and the
                        second length is clamped to 0 instead of becoming -1 ulp
      grid_clamped      1.6 substitutions: the last grid point is clamped to the total
      grid_equal        INNER and C show the same all-reference list and are 2 substitutions apart: grid points i and 4 - i have
                        the same two lengths swapped and the same cost; the first strict maximum decides
      lone_root         a tree of one node
    Thirteen-node frame (update_trees.thirteen): every length three times too long and all flags set -- most branches move, every
    repair dirties and changes the lists of nodes still to come, in the reference's LIFO order.
    root_step_raises needs a repair that raises, a None over a positive length: only the zero-rate modes have one (zero_gadgets).
    A second sweep, from the flags the first left, is compared wherever it stays clear of rounding too (sweeps_to_compare, per
    gadget, mode and fastPass; SECOND_SWEEP names the gadgets for which that must hold everywhere)."""
    ref = le.reference()
    u = bool(le.model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(700 + le.MODES.index(mode))
    taken = set()
    base = ut._background(rng, ref, 10, taken)
    own = {k: ut._background(rng, ref, 4, taken) for k in "abc"}
    shared = ut._background(rng, ref, 3, taken)                     # what A and B have and C has not: the branch above INNER
    out = {}
    muts = [[], [], []]
    if mutations:
        ps = [int(p) for p in rng.choice([p for p in range(30, L - 30, 13) if p not in taken and not ut.S - 40 <= p <= ut.S + 40], size=9,
                                         replace=False)]
        muts = [sorted(le.mutation(ref, p, True, le.other(rng, int(ref[p - 1]))) for p in ps[k::3]) for k in (0, 1, 2)]
        taken.update(ps)                                            # (no leaf of the thirteen-node frame names a mutated site)

    def leaf(k, extra=None):
        return ut._sites(ref, u, {**base, **(own[k] if k in own else {}), **(shared if k in "ab" else {}), **(extra or {})})

    def tree(a, b, c, mut_leaf=TA, **kw):
        t = ut.five(a, b, c, **kw)
        if mut_leaf is not None and t.dist[mut_leaf] > 0.0:
            t.mutations[mut_leaf] = [tuple(m) for m in muts[0]]
        if t.dist[INNER] > 0.0:
            t.mutations[INNER] = [tuple(m) for m in muts[1]]
        t.mutations[ROOT] = [tuple(m) for m in muts[2]]
        return ut.consistent(o, t)

    def add(name, t, arms=(), **kw):
        out[name] = SweepGadget(name, t, arms, **kw)

    wrong = dict(da=1e-4, db=9e-3, dc=2e-4, di=6e-3)
    t = tree(leaf("a"), leaf("b"), leaf("c"), **wrong)
    add("perturbed", t, arms=("root_grid_run", "moved") + (("node_mutations", "root_child_mutations", "root_mutations") if mutations else ()))
    add("converged", settled(o, t), arms=("within_one_percent", "root_child_unmoved_repaired", "node_clean"))
    same = ut._sites(ref, u, {**base, **shared})
    add("false_positive", tree(same, leaf("b"), leaf("c"), mut_leaf=TB, da=3e-4, db=2e-3, dc=1e-3, di=2e-3), arms=("est_false_len_positive",))
    add("false_zero", tree(same, leaf("b"), leaf("c"), mut_leaf=TB, da=0.0, db=2e-3, dc=1e-3, di=2e-3), arms=("est_false_len_zero",))
    add("zero_to_positive", tree(leaf("a"), leaf("b"), leaf("c"), mut_leaf=TB, da=0.0, db=2e-3, dc=1e-3, di=2e-3), arms=("est_positive_len_zero",))
    case = le.corpus(mode)["blen_tenth"][0]
    add("tenth", tree(case["C"], case["P"], case["P"], mut_leaf=None, da=1e-3, db=1e-3, dc=1e-3, di=1e-3), arms=("est_tenth",))
    add("minor_leaf", tree(leaf("a"), leaf("b"), leaf("c"), minor=(2, 0, 0), **wrong), arms=("tip_with_minor_sequences", "moved"))
    t = tree(leaf("a"), leaf("b"), same, da=1e-4, db=9e-3, dc=0.0, di=0.0)
    add("grid_skipped", t, arms=("root_grid_skipped", "moved"))
    flags = [True] * t.n
    flags[TA] = False                                               # (no repair at the root: nothing sets the flag again before A's turn)
    add("partly_clean", t.copy(), arms=("node_clean", "moved"), dirty=flags)
    di, dc = exact_total(2.5)
    bare_c = ut._sites(ref, u, base)            # (C shows nothing of its own: under JC the grid's last point wins, all length above INNER)
    add("grid_half_even", tree(leaf("a"), leaf("b"), bare_c, da=2e-3, db=2e-3, dc=dc, di=di), arms=("root_grid_round_half_even",))
    di, dc = overshooting_total()
    add("grid_best2_clamped", tree(leaf("a"), leaf("b"), bare_c, da=2e-3, db=2e-3, dc=dc, di=di),
        arms=("root_grid_clamped_steps",) + (("root_best2_clamped",) if (mode, mutations) in BEST2_CLAMPED else ()))
    add("grid_clamped", tree(leaf("a"), leaf("b"), leaf("c"), da=2e-3, db=2e-3, dc=0.6 / L, di=1.0 / L), arms=("root_grid_clamped_steps",))
    if not u and not mutations:
        di, dc = exact_total(2.0, 0.5)
        plain = [(4, L)]
        add("grid_equal", ut.consistent(o, ut.five(plain, plain, plain, da=1e-4, db=1e-4, dc=dc, di=di)), arms=("root_grid_equal_costs",),
            equal_costs=True)
    lone = ut.Lists()
    lone.root = lone.add(leaf("c"))
    add("lone_root", lone, arms=("root_no_children",))
    names = ("a", "b", "v", "u1", "u2", "w1", "w2")
    own13 = {k: ut._background(rng, ref, 3 + j % 3, taken) for j, k in enumerate(names)}
    clade = {"s": ut._background(rng, ref, 2, taken), "P": ut._background(rng, ref, 3, taken), "u": ut._background(rng, ref, 2, taken),
             "G": ut._background(rng, ref, 2, taken), "w": ut._background(rng, ref, 4, taken)}
    below = dict(a="sPG", b="sPG", v="PG", u1="uG", u2="uG", w1="w", w2="w")
    lf = lambda k: ut._sites(ref, u, {**base, **own13[k], **{p: x for c in below[k] for p, x in clade[c].items()}})     # noqa: E731
    good = {k: len(own13[k]) / L for k in names}
    good.update({k: len(v) / L for k, v in clade.items()})
    t13 = ut.thirteen([lf(k) for k in names], {k: 3.0 * d for k, d in good.items()})
    for name, ml in zip(("a", "P", "G"), muts):
        t13.mutations[t13.mark[name]] = [tuple(m) for m in ml]
    t13.mutations[t13.root] = [tuple(m) for m in muts[2]]
    t13 = ut.consistent(o, t13)
    add("thirteen_perturbed", t13, arms=("moved", "root_grid_run"))
    return out


def zero_gadgets(o, mode):
    """The gadget of the two zero-rate modes (le.Q_ZERO: A -> C cannot happen), at a site Z whose reference is G or T.
      step_raises a repair of the root's branches that raises (see below)
      grid_none   A and B show A at Z at length 0, so INNER shows it without any length; C shows C.  The grid's first point puts INNER
                  at the root: A -> C over the whole length has no probability, mergeVectors finds no root vector and the reference
                  fails (M:8767).  The lists themselves are consistent: at the lengths the tree has, the root may be C."""
    assert mode.startswith("zeroq")
    ref = le.reference()
    u = bool(le.model(mode).get("usingErrorRate"))
    rng = np.random.default_rng(700 + le.MODES.index(mode))
    fr, to = le.ZERO_RATES[0]
    Z = next(p for p in range(ut.S, ut.S + 40) if int(ref[p - 1]) in (2, 3))
    taken = {Z}
    base = ut._background(rng, ref, 10, taken)
    hard = (1, 1, 1) if u else (0, 0, 0)
    leaf = lambda s: ut._sites(ref, u, {**base, Z: s})              # noqa: E731
    t = ut.consistent(o, ut.five(leaf(fr), leaf(fr), leaf(to), da=0.0, db=0.0, dc=1e-3, di=1e-3, minor=hard))
    out = {"grid_none": SweepGadget("grid_none", t, raises="root")}
    # step_raises: A and B are N at Z, C shows A there; after the lists were made B is hand-set to C over its positive length (a tree
    # edit that was not announced, as in update_trees.gadgets).  The grid sees INNER's lower list, N at Z, and runs; the repair of
    # INNER that follows merges what INNER sees from C with B: A -> C has no probability over any length, the reference raises
    # (M:5583) inside the root step's try, and its except: arm would raise again.
    n_at_z = [(Z - 2, Z + 2)]
    blank = lambda: ut._sites(ref, u, dict(base), n_at_z)           # noqa: E731
    t = ut.consistent(o, ut.five(blank(), blank(), leaf(fr), da=1e-3, db=1e-3, dc=0.0, di=2e-3, minor=hard))
    t.probVect[TB] = [tuple(e) for e in leaf(to)]
    out["step_raises"] = SweepGadget("step_raises", t, arms=("root_step_raises",), raises="node")
    return out
