#!/usr/bin/env python3
"""Golden vectors for the per-sample error report (calculateErrorProbabilities, M:9783-10020) -- BUILD CONTAINER ONLY.

The function reads a tree and the error model and writes text; every case runs the unmodified reference's function on the tree of
a committed tests/golden/em_<name>.json.gz fixture (the tree is not duplicated: `em` names it) under that fixture's model, for
minErrorProb in THRESHOLDS, and records as DATA in tests/golden/errprob_<name>.json.gz, per threshold: the leaves in the order
the function met them, each leaf's records (pos, allele index or 4 for "X", prob) and the SHA-256 of the exact text -- plus what
the text's names were made from (the nodes' name ids, the minor sequences' ids, namesInTree).

  caterpillar cases: the snapshot of the em_ fixture under the reference's globals of make_golden_em.cat_globals();
  reference-run cases: make_golden_search.frozen_reference_tree again, its snapshot asserted equal to the committed one.

errprob_arms.json: the arm-opening lines of M:9820-10004 and those no fixture reached (none).
errprob_zero_div.json.gz: one hand-built tree of its own on which the reference raises ZeroDivisionError (error rate 0, a leaf
at distance 0 whose parent shows the reference without lengths where the leaf shows a substitution).

A recorded probability within MARGIN (relative) of a non-zero threshold would let a last-bit difference move a record across it:
the generator refuses to write such a fixture.

    python tests/golden/make_golden_errprob.py [case ...]      # no argument: every case, then errprob_arms.json
"""
import ast
import contextlib
import gzip
import hashlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))
import make_golden_em as mge  # noqa: E402
import make_golden_search as mgs  # noqa: E402
from make_golden import REF, ser_list  # noqa: E402
import list_edges as le  # noqa: E402

THRESHOLDS = (0.0, 0.01, 0.5)
MARGIN = 1e-9
ARM_RANGE = (9820, 10004)
CAT_CASES = ("cat_a_gerr", "cat_a_full", "cat_a_gerr_gtr", "cat_b_gerr", "cat_b_full", "cat_zero_gerr", "cat_zero_full")
REF_CASES = ("synth_siteerr", "example_siteerr", "synth_gtr_err")
ALLELES = {"A": 0, "C": 1, "G": 2, "T": 3, "X": 4}


def load_em(name):
    with gzip.open(os.path.join(HERE, f"em_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


def traced_report(g, tree, root, thr, names):
    """(text or None, repr of what it raised or None, lines of ARM_RANGE executed) of one call of the reference's function."""
    fn = g["calculateErrorProbabilities"]
    code = fn.__code__
    lines = set()

    def local(frame, event, arg):
        if event == "line":
            lines.add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        return local if (event == "call" and frame.f_code is code) else None

    out, err = io.StringIO(), None
    sys.settrace(tracer)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn(tree, root, out, thr, names)
    except ZeroDivisionError as e:
        err = repr(e)
    finally:
        sys.settrace(None)
    return (None if err else out.getvalue()), err, sorted(x for x in lines if ARM_RANGE[0] <= x <= ARM_RANGE[1])


def parse_report(text, names, tree):
    """The text back into (leaf nodes in order, records per leaf); a leaf's own name line is told from its minor sequences' by
    the ids: every name id is used once."""
    node_of_name = {names[tree.name[v]]: v for v in range(len(tree.up)) if not tree.children[v]}
    assert len(node_of_name) == sum(1 for c in tree.children if not c)
    leaves, recs = [], []
    for line in text.splitlines():
        if line.startswith(">"):
            if line[1:] in node_of_name:
                leaves.append(node_of_name[line[1:]])
                recs.append([])
        else:
            p, a, x = line.split("\t")
            assert repr(float(x)) == x
            recs[-1].append([int(p), ALLELES[a], float(x)])
    return leaves, recs


def record(name, em_name, g, tree, root, names, extra=None):
    fx = dict(name=name, em=em_name, namesInTree=list(names), nodeName=list(tree.name),
              minorIds=[list(m) for m in tree.minorSequences], thresholds=[])
    seen = set()
    for thr in THRESHOLDS:
        text, err, lines = traced_report(g, tree, root, thr, names)
        assert err is None, (name, thr, err)
        seen.update(lines)
        leaves, recs = parse_report(text, names, tree)
        for rl in recs:
            for _, _, x in rl:
                assert thr == 0.0 or abs(x - thr) > MARGIN * thr, (name, thr, x)
        fx["thresholds"].append(dict(minErrorProb=thr, leaves=leaves, records=recs, sha256=hashlib.sha256(text.encode()).hexdigest()))
    fx["lines"] = sorted(seen)
    fx.update(extra or {})
    write_fixture(name, fx)


def write_fixture(name, fixture):
    path = os.path.join(HERE, f"errprob_{name}.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as raw:
        raw.write(json.dumps(fixture).encode())
    n0 = sum(len(r) for r in fixture["thresholds"][0]["records"]) if fixture.get("thresholds") else 0
    print(f"[{name}] -> {path} {os.path.getsize(path) / 1e3:.1f} kB, {n0} records at threshold 0"
          + (f", raised {fixture['raised']}" if fixture.get("raised") else ""), flush=True)


def named(tree, n_minor):
    """name ids and integer minor-sequence ids for a tree that has only counts; namesInTree to go with them."""
    n = len(tree.up)
    tree.name = list(range(n))
    nxt = n
    tree.minorSequences = []
    for k in n_minor:
        tree.minorSequences.append(list(range(nxt, nxt + k)))
        nxt += k
    return [f"S{i}" for i in range(nxt)]


def run_caterpillar(name):
    em = load_em(name)
    g = mge.cat_globals()
    m = em["model"]
    mge.set_model(g, dict(Q=m["Q"], siteRates=m["siteRates"], usingErrorRate=m["usingErrorRate"], errorRateGlobal=m["errorRateGlobal"],
                          errorRates=m["errorRates"]), m["emModel"])
    tree = mge.as_tree(em["tree"])
    names = named(tree, em["tree"]["nMinor"])
    record(name, name, g, tree, em["tree"]["root"], names)


def run_reference_tree(name):
    em = load_em(name)
    g, tree, t1, _, _ = mgs.frozen_reference_tree(name, mge.REF_RUNS[name])
    snap = json.loads(json.dumps(mgs.snapshot_tree(tree, t1)))
    assert snap == em["tree"], f"{name}: the re-run's tree is not the committed em_ fixture's"
    assert json.loads(json.dumps(mge.model_of(g))) == em["model"], f"{name}: the re-run's model is not the committed em_ fixture's"
    record(name, name, g, tree, t1, g["namesInTree"])


def run_zero_div():
    ref = le.reference()
    L = len(ref)
    g = mge.cat_globals()
    m = dict(le.model("gerr"))
    m["errorRateGlobal"] = 0.0
    mge.set_model(g, m)
    s = 700
    x = (int(ref[s - 1]) + 1) % 4
    R = [(4, L)]
    sub = le.Builder(ref, True).nuc(s, x).done()
    # root 0 = [1, 2], node 2 = [3, 4]; leaf 3 at distance 0 under a parent list without lengths
    up, children = [None, 0, 0, 2, 2], [[1, 2], [], [3, 4], [], []]
    dist = [0.0, 1e-4, 1e-4, 0.0, 2e-4]
    pv = [R, R, R, sub, R]
    ur, ul = [R, None, R, None, None], [R, None, R, None, None]
    snap = dict(root=0, up=up, children=children, dist=dist, mutations=[[] for _ in up], nMinor=[0] * 5,
                probVect=[ser_list(q) for q in pv], probVectUpRight=[None if q is None else ser_list(q) for q in ur],
                probVectUpLeft=[None if q is None else ser_list(q) for q in ul], probVectTotUp=[None] * 5, n=5)
    tree = mge.as_tree(snap)
    names = named(tree, snap["nMinor"])
    text, err, _ = traced_report(g, tree, 0, 0.0, names)
    assert text is None and "ZeroDivisionError" in err, (text, err)
    write_fixture("zero_div", dict(name="zero_div", context=mge.context_of(g), model=mge.model_of(g), tree=snap, raised=err,
                                   node=3, position=s))


def arm_lines():
    """First line of every if / elif / else / loop body of the function within ARM_RANGE (make_golden_em.arm_lines' rule)."""
    src = open(REF).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "calculateErrorProbabilities")
    arms = set()

    def visit(stmts):
        for s in stmts:
            if isinstance(s, (ast.If, ast.While, ast.For)):
                for body in (s.body, s.orelse):
                    if not body:
                        continue
                    if not (len(body) == 1 and isinstance(body[0], ast.If) and body is s.orelse):
                        arms.add(body[0].lineno)
                    visit(body)
    visit(fn.body)
    return sorted(a for a in arms if ARM_RANGE[0] <= a <= ARM_RANGE[1])


def write_arms():
    arms = arm_lines()
    seen = set()
    for name in CAT_CASES + REF_CASES:
        path = os.path.join(HERE, f"errprob_{name}.json.gz")
        if os.path.exists(path):
            with gzip.open(path, "rt") as fh:
                seen.update(json.load(fh)["lines"])
    missed = [a for a in arms if a not in seen]
    print(f"{len(arms)} arms; not reached: {missed}", flush=True)
    with open(os.path.join(HERE, "errprob_arms.json"), "w") as fh:
        json.dump(dict(arms=arms, range=list(ARM_RANGE), reached=[a for a in arms if a in seen], unreached=missed), fh, indent=1)


if __name__ == "__main__":
    todo = sys.argv[1:] or (list(CAT_CASES) + list(REF_CASES) + ["zero_div", "arms"])
    for nm in todo:
        if nm == "arms":
            write_arms()
        elif nm == "zero_div":
            run_zero_div()
        elif nm in CAT_CASES:
            run_caterpillar(nm)
        else:
            run_reference_tree(nm)
