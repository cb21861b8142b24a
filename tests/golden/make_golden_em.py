#!/usr/bin/env python3
"""Golden vectors for the EM step (expectationMaximizationCalculationRates, M:10077-10947) -- BUILD CONTAINER ONLY.

Two kinds of cases, each written as DATA to tests/golden/em_<name>.json.gz:

  (a) trees the unmodified reference built itself (make_golden_search.frozen_reference_tree), with the model its run ended with;
  (b) hand-built caterpillar trees (internal node i has children [leaf_i, internal_{i+1}]), whose (upper, lower) list pair of
      every branch is set by hand -- the function reads nothing else of a tree -- from the corpora of tests/list_edges.py plus
      pairs aimed at the arms no reference run reaches, each tree under four models (plain, rate variation, global error rate,
      the full model).

Per case: the tree snapshot, the model, the returned 4-tuple, the sufficient statistics at M:10852 (`raw`: what
maple_em_expectation returns) and at the return (`final`), and the set of reference lines of M:10138-10947 the call executed.
tests/golden/em_arms.json lists the arm-opening lines of M:10168-10790 and M:10855-10946 (first line of every if / elif / else
/ loop body; bodies that only raise and bodies under trackMutations are left out: a call that raises returns nothing to record
and trackMutations is out of scope) and the arms no committed fixture reaches, with a reason each.

    python tests/golden/make_golden_em.py [case ...]       # no argument: every case, then em_arms.json
    python tests/golden/make_golden_em.py arms             # em_arms.json from the committed fixtures only
"""
import ast
import contextlib
import copy
import glob
import gzip
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import make_golden_search as mgs  # noqa: E402
from make_golden import REF, ser_list  # noqa: E402
import list_edges as le  # noqa: E402

MAT12 = ["--maxNumDescendantsForMATClade", "12"]
REF_RUNS = {
    "synth_unrest": mgs.RUNS["synth_unrest"],
    "synth_siteerr": mgs.RUNS["synth_siteerr"],
    "example_siteerr": mgs.RUNS["example_siteerr"],
    "synth_gtr_err": ["--model", "GTR", "--estimateErrorRate"] + MAT12,
    "synth_ratevar": ["--model", "UNREST", "--rateVariation"] + MAT12,
}
CAT_MODES = {"plain": "unrest", "ratevar": "ratevar", "gerr": "gerr", "full": "siteerr"}     # -> list_edges mode
CAT_TREES = ("cat_a", "cat_b", "cat_zero")
E_STEP_LINE = 10852                      # "if usingErrorRate:" right after the walk
WALK = (10138, 10947)
ARM_RANGES = ((10168, 10790), (10855, 10946))
STAT_KEYS = ("counts", "waitingTimes", "numTips", "errorCount", "observedTotNucsSites", "observedNucsSites", "errorCountSites",
             "totTreeLength", "waitingTimesSites", "countsSites", "trackingNs")
CTX_KEYS = ("lRef", "thresholdProb", "minBLenSensitivity", "thresholdDiffForUpdate", "thresholdFoldChangeUpdate", "defaultBLen")


def traced_em(g, tree, root):
    """The reference's EM step under a line trace: (4-tuple or None if it raised, raw statistics, final statistics, lines)."""
    fn = g["expectationMaximizationCalculationRates"]
    code = fn.__code__
    lines, snap = set(), {}

    def grab(L):
        return {k: copy.deepcopy(L[k]) for k in STAT_KEYS if k in L}

    def local(frame, event, arg):
        if event == "line":
            ln = frame.f_lineno
            lines.add(ln)
            if ln == E_STEP_LINE and "raw" not in snap:
                snap["raw"] = grab(frame.f_locals)
        elif event == "return":
            snap["final"] = grab(frame.f_locals)
        return local

    def tracer(frame, event, arg):
        return local if (event == "call" and frame.f_code is code) else None

    ret, err = None, None
    sys.settrace(tracer)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            ret = fn(tree, root)
    except Exception as e:                                  # raise Exception("exit"): MAPLE_ERR_FATAL on the device
        err = repr(e)
    finally:
        sys.settrace(None)
    lines = sorted(x for x in lines if WALK[0] <= x <= WALK[1])
    return ret, err, snap.get("raw"), snap.get("final"), lines


def model_of(g):
    return dict(useRateVariation=bool(g["useRateVariation"]), usingErrorRate=bool(g["usingErrorRate"]),
                errorRateSiteSpecific=bool(g["errorRateSiteSpecific"]), Q=[list(r) for r in g["mutMatrixGlobal"]],
                siteRates=list(g["siteRates"]) if g["useRateVariation"] else None,
                errorRateGlobal=g["errorRateGlobal"] if g["usingErrorRate"] else 0.0,
                errorRates=list(g["errorRates"]) if (g["usingErrorRate"] and g["errorRateSiteSpecific"]) else None,
                emModel=g["model"])


def context_of(g):
    ctx = {k: g[k] for k in CTX_KEYS}
    ctx["rootFreqs"] = list(g["rootFreqs"])
    ctx["ref"] = g["ref"]
    return ctx


def write_fixture(name, fixture):
    path = os.path.join(HERE, f"em_{name}.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as raw:
        raw.write(json.dumps(fixture).encode())
    print(f"[{name}] -> {path} {os.path.getsize(path) / 1e6:.3f} MB, {len(fixture['lines'])} lines"
          + (f", raised {fixture['raised']}" if fixture.get("raised") else ""), flush=True)


def record(name, g, tree, root, snap, extra=None):
    ret, err, raw, final, lines = traced_em(g, tree, root)
    fx = dict(name=name, context=context_of(g), model=model_of(g), tree=snap, lines=lines, raised=err)
    if ret is not None:
        fx["ret"] = dict(Q=[list(r) for r in ret[0]], siteRates=ret[1], errorRate=ret[2], siteErrRates=ret[3])
        fx["raw"], fx["final"] = raw, final
    fx.update(extra or {})
    return fx, ret


# ---- (a) trees of the reference's own runs -----------------------------------------------------------------------------------
def run_reference_tree(name):
    g, tree, t1, _, inp = mgs.frozen_reference_tree(name, REF_RUNS[name])
    snap = mgs.snapshot_tree(tree, t1)
    fx, ret = record(name, g, tree, t1, snap, dict(flags=REF_RUNS[name], input=os.path.basename(inp)))
    if not g["usingErrorRate"]:                             # "LK after one round of EM", M:12401-12407
        with contextlib.redirect_stdout(io.StringIO()):
            g["mutMatrixGlobal"], g["siteRates"] = ret[0], ret[1]
            g["updateMutMatrices"](ret[0], siteRates=ret[1])
            g["setAllDirty"](tree, t1)
            g["reCalculateAllGenomeLists"](tree, t1)
            fx["lkAfterOneRound"] = g["calculateTreeLikelihood"](tree, t1)
    write_fixture(name, fx)


# ---- (b) caterpillar trees -------------------------------------------------------------------------------------------------
def mask_n(gl, a, b):
    """The list with N over positions [a, b] (1-based, inclusive)."""
    out, pos = [], 0
    for e in gl:
        end = e[1] if e[0] in (4, 5) else pos + 1
        lo, hi = pos + 1, end
        if hi < a or lo > b:
            out.append(e)
        else:
            if lo < a:
                out.append((e[0], a - 1) + tuple(e[2:]))
            out.append((5, min(hi, b)))
            if hi > b:
                out.append(e)
        pos = end
    return le.merge_n_runs(out)


def combo_pair(rng, ref, u, big_d0):
    """One (upper, lower) pair with every kind of parent entry against every kind of child entry, one site each."""
    L = len(ref)
    P, C = le.Builder(ref, u), le.Builder(ref, u)
    r = lambda p: int(ref[p - 1])                             # noqa: E731
    d0s = 3.0 if big_d0 else 1e-4
    p_kinds = ["R", "R_d0", "R_d0d1", "R_flag", "nuc", "nuc_d0", "nuc_d0d1", "nuc_d0d1_flag", "O", "O_d0", "N", "nucB_d0d1"]
    c_kinds = ["R", "R_d0", "same", "diff", "diff_d0", "O_hit", "O_miss", "O_ref", "O_d0", "N", "O_soft"]
    s = 6
    for pk in p_kinds:
        for ck in c_kinds:
            s += 2
            x = le.other(rng, r(s))                          # the parent's nucleotide where it shows one
            i1 = x if pk.startswith("nuc") else r(s)
            if pk == "R":
                pass
            elif pk == "R_d0":
                P.run(4, s, s, d0=d0s)
            elif pk == "R_d0d1":
                P.run(4, s, s, d0=d0s, d1=2e-4)
            elif pk == "R_flag":
                P.run(4, s, s, d0=0.0, flag=True)
            elif pk == "nuc":
                P.nuc(s, x)
            elif pk == "nuc_d0":
                P.nuc(s, x, d0=d0s)
            elif pk in ("nuc_d0d1", "nucB_d0d1"):
                P.nuc(s, x, d0=(3.0 if pk == "nucB_d0d1" else d0s), d1=(2.5 if pk == "nucB_d0d1" else 3e-4))
            elif pk == "nuc_d0d1_flag":
                P.nuc(s, x, d0=d0s, d1=1e-4, flag=True)
            elif pk == "O":
                P.o(s, rng.dirichlet([1.0] * 4))
            elif pk == "O_d0":
                P.o(s, rng.dirichlet([1.0] * 4), d0=d0s)
            elif pk == "N":
                P.run(5, s, s)
            if ck == "R":
                pass
            elif ck == "R_d0":
                C.run(4, s, s, d0=2e-4, flag=bool(s % 4 == 0))
            elif ck == "same":
                if i1 != r(s):
                    C.nuc(s, i1)
            elif ck == "diff":
                C.nuc(s, le.other(rng, r(s), (i1,)))
            elif ck == "diff_d0":
                C.nuc(s, le.other(rng, r(s), (i1,)), d0=1e-4, flag=True)
            elif ck == "O_hit":                              # the parent's nucleotide is possible
                y = le.other(rng, i1)
                C.o(s, [0.5 if k in (i1, y) else 0.0 for k in range(4)])
            elif ck == "O_miss":                             # ... is not
                ys = [k for k in range(4) if k != i1][: 2 + s % 2]
                C.o(s, [1.0 / len(ys) if k in ys else 0.0 for k in range(4)])
            elif ck == "O_ref":
                y = le.other(rng, r(s))
                C.o(s, [0.5 if k in (r(s), y) else 0.0 for k in range(4)])
            elif ck == "O_d0":
                C.o(s, rng.dirichlet([1.0] * 4), d0=3e-4)
            elif ck == "N":
                C.run(5, s, s)
            elif ck == "O_soft":
                C.o(s, le.o_vec(rng, i1, 0.04))
    assert s < L - 400
    # runs: N against R / N / R with a tail, ending inside the other side's run, and N up to lRef on one side
    P.run(5, L - 380, L - 360).run(4, L - 359, L - 340, d0=1e-4).run(5, L - 320, L - 300)
    C.run(5, L - 370, L - 350).run(5, L - 345, L - 330).run(4, L - 325, L - 310, d0=2e-4)
    if big_d0:
        P.run(5, L - 40, L)
    else:
        C.run(5, L - 25, L)
    return P.done(), C.done()


def caterpillar(tree_name, lmode):
    """(columns of the tree, pair labels): the recipe of a tree for the tuple grammar of a list_edges mode."""
    ref = le.reference()
    L = len(ref)
    u = bool(le.model(lmode).get("usingErrorRate"))
    rng = np.random.default_rng({"cat_a": 11, "cat_b": 12, "cat_zero": 13}[tree_name])
    pairs = []                                               # (P, C, dist, wantLeaf or None, nMinor)
    if tree_name == "cat_zero":                              # nucleotide 0 never waits: the child lists are R runs with a length
        sites = [p for p in range(50, L - 50) if int(ref[p - 1]) != 0]          # of their own (no R / R contribution), but for one
        for k in range(5):                                   # site where two of the other nucleotides meet
            s = sites[37 * (k + 1)]
            x = next(i for i in (1, 2, 3) if i != int(ref[s - 1]))
            y = next(i for i in (1, 2, 3) if i not in (x, int(ref[s - 1])))
            P = le.Builder(ref, u).nuc(s, x).done()
            C = le.Builder(ref, u).run(4, 1, s - 1, d0=1e-4).nuc(s, y).run(4, s + 1, L, d0=1e-4).done()
            pairs.append((P, C, 1e-3, None, k % 2))
    else:
        fam = le.corpus(lmode)
        dists = [1e-4, 0.0, 2.5, 3e-5, 0.7]
        for big in (False, True):
            for leaf in (True, False):
                for d in ((1e-4, 0.0, 2.5) if leaf else (1e-4, 2.5)):
                    for nm in ((0, 2) if leaf else (0,)):
                        P, C = combo_pair(rng, ref, u, big)
                        pairs.append((P, C, d, leaf, nm))
        if tree_name == "cat_a":
            src = fam["append_d1_O"][:24] + fam["skip_edges"][::5] + fam["long"] + fam["append_carry"][:2]
        else:
            src = fam["append_d1_O"][24:] + fam["skip_edges"][2::7] + fam["append_carry"][2:3]
        for k, c in enumerate(src):
            pairs.append((c["P"], c["C"], dists[k % 5], None, (k % 7 == 0) * 1))
        for k in range(30 if tree_name == "cat_a" else 95):  # (cat_b: more than one block of branches, a ragged last wavefront)
            pairs.append((le.rich_list(rng, ref, u, mean_gap=[8, 20, 45][k % 3]),
                          le.rich_list(rng, ref, u, mean_gap=[10, 30][k % 2], d1=False), dists[(k + 1) % 5], None, (k % 9 == 0) * 3))
        if tree_name == "cat_b":                             # short lists, many of them: the branches fill more than one block
            for k in range(330):
                pairs.append((le.rich_list(rng, ref, u, mean_gap=[120, 200, 300][k % 3]),
                              le.rich_list(rng, ref, u, mean_gap=[150, 260][k % 2], d1=False), dists[(k + 2) % 5], None, (k % 11 == 0) * 1))
        if tree_name == "cat_b":                             # a stretch where EVERY branch is N: totExpected == 0, observedNuc == 0
            pairs = [(mask_n(P, 2, 5), mask_n(C, 2, 5), d, lf, nm) for (P, C, d, lf, nm) in pairs]
    for P, C, _, _, _ in pairs:
        le.check_grammar(P, L, u)
        le.check_grammar(C, L, u)
    # K internal nodes hold K + 1 leaf branches and K - 1 internal ones; pairs that do not care fill what is left of either
    mustL, mustI = [p for p in pairs if p[3] is True], [p for p in pairs if p[3] is False]
    und = [p for p in pairs if p[3] is None]
    K = max(len(mustL) - 1, len(mustI) + 1, (len(pairs) + 1) // 2, 2)
    nl = min(len(und), K + 1 - len(mustL))
    leafP, intP = mustL + und[:nl], mustI + und[nl:]
    filler = ([(4, L)], le.Builder(ref, u).run(4, 1, L, d0=1e-4).done() if tree_name == "cat_zero" else [(4, L)], 2e-5, None, 0)
    intP += [filler] * (K - 1 - len(intP))
    leafP += [filler] * (K + 1 - len(leafP))
    assert len(intP) == K - 1 and len(leafP) == K + 1
    n = 2 * K + 1
    internal = list(range(K))                                # node ids: internal 0..K-1, leaf_i = K + i
    up, children, dist = [None] * n, [[] for _ in range(n)], [0.0] * n
    pv, ur, ul, nminor = [[(4, L)] for _ in range(n)], [None] * n, [None] * n, [0] * n
    for i in internal:
        right = internal[i + 1] if i + 1 < K else K + K      # the last internal node carries two leaves
        children[i] = [K + i, right]
        up[K + i], up[right] = i, i
    li = ii = 0
    for i in internal:
        for which, v in enumerate(children[i]):
            if children_is_leaf(v, K):
                P, C, d, _, nm = leafP[li]
                li += 1
            else:
                P, C, d, _, nm = intP[ii]
                ii += 1
                nm = 0
            if which == 0:
                ur[i] = P
            else:
                ul[i] = P
            pv[v], dist[v], nminor[v] = C, d, nm
    assert li == len(leafP) and ii == len(intP)
    mutations = [[] for _ in range(n)]
    if tree_name != "cat_zero":                              # a root with mutations, a reference branch above an internal node and
        cur = np.array(ref).copy()                           # above a leaf; one site mutated twice, one mutated back to the reference

        def mut(node, sites):
            for p in sites:
                to = int(ref[p - 1]) if (cur[p - 1] != ref[p - 1] and p % 2) else le.other(rng, int(cur[p - 1]))
                mutations[node].append((p, int(cur[p - 1]), to))
                cur[p - 1] = to
        mut(0, [9, 40, 700, L - 5])
        mut(min(3, K - 1), [9, 41, 120, 701, L - 300])
        leaf_under = children[min(5, K - 1)][0]
        mut(leaf_under, [41, 300, L])
    tot = [None] * n
    return dict(root=0, up=up, children=children, dist=dist, mutations=[[list(m) for m in ml] for ml in mutations], nMinor=nminor,
                probVect=[ser_list(x) for x in pv], probVectUpRight=[ser_list(x) for x in ur],
                probVectUpLeft=[ser_list(x) for x in ul], probVectTotUp=tot, n=n)


def children_is_leaf(v, K):
    return v >= K


_cat_g = {}


def cat_globals():
    """The reference's globals for lRef = 1500 over list_edges.reference(): one tiny run of the unmodified reference."""
    if "g" not in _cat_g:
        ref = le.reference()
        tmp = tempfile.mkdtemp(prefix="maple_golden_em_")
        inp = os.path.join(tmp, "tiny.maple.txt")
        with open(inp, "w") as fh:
            fh.write(">reference\n" + "".join("acgt"[int(x)] for x in ref) + "\n")
            for k in range(5):
                fh.write(f">T{k}\n")
                for p in range(10 + 7 * k, 1400, 211 + 13 * k):
                    fh.write(f"{'acgt'[(int(ref[p - 1]) + 1 + k % 3) % 4]}\t{p}\n")
        mgs.INPUTS["em_tiny"] = inp
        _cat_g["g"] = mgs.frozen_reference_tree("em_tiny", ["--model", "UNREST", "--numTopologyImprovements", "0"])[0]
    return _cat_g["g"]


def set_model(g, m, em_model="UNREST"):
    sr, er = m.get("siteRates"), m.get("errorRates")
    g["model"] = em_model
    g["useRateVariation"], g["usingErrorRate"] = sr is not None, bool(m.get("usingErrorRate"))
    g["errorRateSiteSpecific"] = er is not None
    g["mutMatrixGlobal"], g["siteRates"] = [list(r) for r in m["Q"]], (list(sr) if sr is not None else None)
    g["updateMutMatrices"](g["mutMatrixGlobal"], siteRates=g["siteRates"])
    g["errorRateGlobal"] = m.get("errorRateGlobal", 0.0) if g["usingErrorRate"] else None
    g["errorRates"] = list(er) if er is not None else None


def as_tree(snap):
    tl = lambda col: [None if x is None else [tuple(e) for e in x] for x in col]         # noqa: E731
    return types.SimpleNamespace(
        up=list(snap["up"]), children=[list(c) for c in snap["children"]], dist=list(snap["dist"]),
        mutations=[[tuple(m) for m in ml] for ml in snap["mutations"]], minorSequences=[["m"] * k for k in snap["nMinor"]],
        probVect=tl(snap["probVect"]), probVectUpRight=tl(snap["probVectUpRight"]), probVectUpLeft=tl(snap["probVectUpLeft"]),
        probVectTotUp=[None] * snap["n"])


def run_caterpillar(tree_name):
    g = cat_globals()
    for mode, lmode in CAT_MODES.items():
        snap = caterpillar(tree_name, lmode)
        variants = [("", "UNREST", le.model(lmode))]
        if (tree_name == "cat_a" and mode in ("plain", "gerr")) or (tree_name == "cat_zero" and mode == "plain"):
            variants.append(("_gtr", "GTR", le.model(lmode)))
        if tree_name == "cat_a" and mode == "ratevar":       # a negative rate: the reference raises (M:10336 and its kin)
            bad = dict(le.model(lmode))
            bad["Q"] = [list(r) for r in bad["Q"]]
            for i, j in ((0, 1), (1, 2), (2, 3), (3, 0)):
                bad["Q"][i][j] = -abs(bad["Q"][i][j])
            variants.append(("_negq", "UNREST", bad))
        for suffix, em_model, m in variants:
            set_model(g, m, em_model)
            name = f"{tree_name}_{mode}{suffix}"
            fx, _ = record(name, g, as_tree(snap), snap["root"], snap)
            assert (fx["raised"] is not None) == (suffix == "_negq"), (name, fx["raised"])
            write_fixture(name, fx)


# ---- the arms ----------------------------------------------------------------------------------------------------------------
def arm_lines():
    """First line of every if / elif / else / loop body in ARM_RANGES of the reference, without bodies that only raise (and
    print) and without anything under a test of trackMutations."""
    src = open(REF).read()
    mod = ast.parse(src)
    fn = next(n for n in ast.walk(mod) if isinstance(n, ast.FunctionDef) and n.name == "expectationMaximizationCalculationRates")
    arms = set()

    def only_raises(body):
        return all(isinstance(s, ast.Raise) or (isinstance(s, ast.Expr) and isinstance(s.value, ast.Call)
                                                and getattr(s.value.func, "id", "") == "print") for s in body)

    def visit(stmts):
        for s in stmts:
            if isinstance(s, (ast.If, ast.While, ast.For)):
                test_src = ast.get_source_segment(src, s.test) if not isinstance(s, ast.For) else ""
                if "trackMutations" in test_src and "not trackMutations" not in test_src:
                    visit(s.orelse)
                    continue
                for body in (s.body, s.orelse):
                    if not body:
                        continue
                    if not only_raises(body) and not (len(body) == 1 and isinstance(body[0], ast.If) and body is s.orelse):
                        arms.add(body[0].lineno)
                    visit(body)
    visit(fn.body)
    return sorted(a for a in arms if any(lo <= a <= hi for lo, hi in ARM_RANGES))


# arms no committed fixture reaches: {line: reason}; at most three
UNREACHABLE = {}


def write_arms():
    arms = arm_lines()
    seen = set()
    for path in sorted(glob.glob(os.path.join(HERE, "em_*.json.gz"))):
        with gzip.open(path, "rt") as fh:
            seen.update(json.load(fh)["lines"])
    missed = [a for a in arms if a not in seen]
    print(f"{len(arms)} arms; not reached: {missed}", flush=True)
    out = dict(arms=arms, ranges=[list(r) for r in ARM_RANGES],
               unreachable=[dict(line=a, reason=UNREACHABLE[a]) for a in missed if a in UNREACHABLE])
    with open(os.path.join(HERE, "em_arms.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    return missed


if __name__ == "__main__":
    todo = sys.argv[1:] or (list(CAT_TREES) + list(REF_RUNS) + ["arms"])
    for nm in todo:
        if nm == "arms":
            write_arms()
        elif nm in CAT_TREES:
            run_caterpillar(nm)
        else:
            run_reference_tree(nm)
