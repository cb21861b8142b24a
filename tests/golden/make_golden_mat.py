#!/usr/bin/env python3
"""Golden vectors for the mutation-annotated tree (expectationMaximizationCalculationRates(tree, root, trackMutations=True),
M:10077-10850, and stringForNode, M:2673-2809; --estimateMAT) -- BUILD CONTAINER ONLY.

Every case runs the unmodified reference's function on the tree of a committed tests/golden/em_<name>.json.gz fixture (the tree is
not duplicated: `em` names it) under that fixture's model, with the reference's global minMutProb set to each of the thresholds,
and records as DATA in tests/golden/mat_<name>.json.gz, per threshold: tree.mutationsInf / tree.Ns / tree.errors per node -- a
mutation or error record as [pos, from, to, prob] (the reference's tuple is (from, pos, to, prob)), an Ns record as the
reference's int or [first, last] -- each node's stringForNode(tree, v, "", dist[v], estimateMAT=True, networkOutput=False,
aBayesPlusOn=False) text ("" for a slot the root does not reach) and the SHA-256 of the texts joined by "\\n"; plus the appending lines the calls executed.  Where a
fixture would pass TEXT_LIMIT bytes compressed, texts are left out from the lowest threshold up until it fits (`texts` is null
there; the SHA-256 and the root's own text, `rootText`, stay).

  caterpillar cases: the snapshot of the em_ fixture under the reference's globals of make_golden_em.cat_globals();
  reference-run cases: make_golden_search.frozen_reference_tree again, its snapshot asserted equal to the committed one;
  em_cat_a_ratevar_negq: the reference raises Exception('exit') at every threshold, which is what is recorded.

Thresholds: 0.0, 0.01 and a third that starts at 0.3 and goes up by 0.01 until no probability of any fixture's threshold-0 run
(both streams) lies within MARGIN (relative) of it -- a recorded probability that close to a non-zero threshold would let a
last-bit difference move a record across the strict `>`: the generator refuses to write such a fixture.  (0.5 is no candidate:
the hand-set O vectors of the caterpillars give probabilities of exactly 0.5.)

mat_arms.json: the eighteen appending lines and the fixtures that reach each; `unreached` must be empty.
mat_root_ns.json.gz: two hand-built trees of their own (no committed tree gives the root an Ns record): five nodes whose root
and zero-length internal child show an N run, a one-site N run and an O entry; and a root without children with an O entry.

    python tests/golden/make_golden_mat.py [case ...]      # no argument: every case, then mat_root_ns and mat_arms.json
"""
import contextlib
import glob
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
from make_golden import ser_list  # noqa: E402
import list_edges as le  # noqa: E402

MARGIN = 1e-9
THIRD_START, THIRD_STEP = 0.3, 0.01
TEXT_LIMIT = 400_000
APPEND_LINES = (10182, 10256, 10330, 10358, 10378, 10415, 10432, 10620, 10670, 10715, 10717, 10735, 10737, 10760, 10779, 10815,
                10817, 10825)
NEGQ = "cat_a_ratevar_negq"
REF_CASES = tuple(mge.REF_RUNS)


def em_names():
    return sorted(os.path.basename(p)[len("em_"):-len(".json.gz")] for p in glob.glob(os.path.join(HERE, "em_*.json.gz")))


def load_em(name):
    with gzip.open(os.path.join(HERE, f"em_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


def traced_mat(g, tree, root, thr):
    """(repr of what the call raised or None, appending lines executed); the records are left on the tree."""
    fn = g["expectationMaximizationCalculationRates"]
    code = fn.__code__
    lines = set()
    for attr in ("mutationsInf", "Ns", "errors"):
        if hasattr(tree, attr):
            delattr(tree, attr)

    def local(frame, event, arg):
        if event == "line":
            lines.add(frame.f_lineno)
        return local

    def tracer(frame, event, arg):
        return local if (event == "call" and frame.f_code is code) else None

    err = None
    g["minMutProb"] = thr
    sys.settrace(tracer)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            fn(tree, root, trackMutations=True)
    except Exception as e:                                   # raise Exception("exit"): MAPLE_ERR_FATAL on the device
        err = repr(e)
    finally:
        sys.settrace(None)
    return err, sorted(x for x in lines if x in APPEND_LINES)


def records_of(g, tree, root, thr):
    n = len(tree.up)
    ev = lambda col: [[[m[1], m[0], m[2], m[3]] for m in col[v]] for v in range(n)]          # noqa: E731
    ns = [[x if isinstance(x, int) else [x[0], x[1]] for x in tree.Ns[v]] for v in range(n)]
    reached, st = set(), [root]                              # a slot the root does not reach is never written: its text is ""
    while st:
        v = st.pop()
        reached.add(v)
        st.extend(tree.children[v])
    with contextlib.redirect_stdout(io.StringIO()):
        texts = [g["stringForNode"](tree, v, "", tree.dist[v], estimateMAT=True, networkOutput=False, aBayesPlusOn=False)
                 if v in reached else "" for v in range(n)]
    return dict(minMutProb=thr, mutationsInf=ev(tree.mutationsInf), Ns=ns,
                errors=ev(tree.errors) if g["usingErrorRate"] else None, texts=texts, rootText=texts[root],
                sha256=hashlib.sha256("\n".join(texts).encode()).hexdigest())


def probabilities(rec):
    out = [m[3] for ml in rec["mutationsInf"] for m in ml]
    if rec["errors"] is not None:
        out += [m[3] for ml in rec["errors"] for m in ml]
    return out


def prepared(name):
    """(the reference's globals set to the fixture's model, the tree, the root, the em_ fixture)"""
    em = load_em(name)
    if name in REF_CASES:
        g, tree, root, _, _ = mgs.frozen_reference_tree(name, mge.REF_RUNS[name])
        snap = json.loads(json.dumps(mgs.snapshot_tree(tree, root)))
        assert snap == em["tree"], f"{name}: the re-run's tree is not the committed em_ fixture's"
        assert json.loads(json.dumps(mge.model_of(g))) == em["model"], f"{name}: the re-run's model is not the committed em_ fixture's"
    else:
        g = mge.cat_globals()
        m = em["model"]
        mge.set_model(g, dict(Q=m["Q"], siteRates=m["siteRates"], usingErrorRate=m["usingErrorRate"],
                              errorRateGlobal=m["errorRateGlobal"], errorRates=m["errorRates"]), m["emModel"])
        tree, root = mge.as_tree(em["tree"]), em["tree"]["root"]
        tree.name = list(range(len(tree.up)))
    return g, tree, root, em


def output_context(g):
    return dict(effectivelyNon0BLen=g["effectivelyNon0BLen"], supportFor0Branches=bool(g["supportFor0Branches"]))


def third_threshold(zero_runs):
    """the first of 0.3, 0.31, ... with no probability of any fixture's threshold-0 run within MARGIN of it"""
    probs = [x for rec in zero_runs.values() for x in probabilities(rec)]
    assert min(probs) > 1e-300, min(probs)
    assert all(abs(x - 0.01) > MARGIN * 0.01 for x in probs), "0.01 is within MARGIN of a recorded probability"
    k = 0
    while True:
        thr = round(THIRD_START + k * THIRD_STEP, 2)
        if all(abs(x - thr) > MARGIN * thr for x in probs):
            return thr
        k += 1


def write_fixture(name, fixture):
    path = os.path.join(HERE, f"mat_{name}.json.gz")

    def dump():
        with gzip.GzipFile(path, "wb", mtime=0) as raw:
            raw.write(json.dumps(fixture).encode())
        return os.path.getsize(path)
    size = dump()
    for rec in fixture.get("thresholds") or []:              # too large: the texts go, the lowest threshold's first
        if size <= TEXT_LIMIT:
            break
        rec["texts"] = None
        fixture["textsLeftOut"] = "the fixture would pass %d bytes with them; the SHA-256 of the texts and rootText stay" % TEXT_LIMIT
        size = dump()
    t = fixture.get("thresholds") or (fixture["cases"][0]["thresholds"] if "cases" in fixture else None)
    print(f"[{name}] -> {path} {size / 1e3:.1f} kB, "
          + (f"raised {fixture['raised']}" if fixture.get("raised") else
             f"{sum(len(x) for x in t[0]['mutationsInf'])} mutations, {sum(len(x) for x in t[0]['Ns'])} Ns, "
             f"{sum(len(x) for x in t[0]['errors']) if t[0]['errors'] is not None else 0} errors at threshold 0"), flush=True)


def run_all(names):
    zero, env = {}, {}
    for name in names:                                       # threshold 0 of everything first: the third threshold depends on all
        g, tree, root, em = prepared(name)
        err, lines = traced_mat(g, tree, root, 0.0)
        if name == NEGQ:
            assert err is not None
            env[name] = (g, tree, root, em, lines, err)
            continue
        assert err is None, (name, err)
        zero[name] = records_of(g, tree, root, 0.0)
        env[name] = (g, tree, root, em, lines, None)
    third = third_threshold(zero)
    print(f"third threshold: {third}", flush=True)
    for name in names:
        g, tree, root, em, lines, err = env[name]
        if name not in REF_CASES:                            # (the caterpillars share one set of globals)
            g, tree, root, em = prepared(name)
        seen = set(lines)
        if name == NEGQ:
            raised = []
            for thr in (0.0, 0.01, third):
                e, ln = traced_mat(g, tree, root, thr)
                assert e is not None
                raised.append(dict(minMutProb=thr, raised=e))
                seen.update(ln)
            write_fixture(name, dict(name=name, em=name, raised=err, perThreshold=raised, lines=sorted(seen)))
            continue
        recs = [zero[name]]
        for thr in (0.01, third):
            e, ln = traced_mat(g, tree, root, thr)
            assert e is None, (name, thr, e)
            seen.update(ln)
            rec = records_of(g, tree, root, thr)
            for x in probabilities(zero[name]):
                assert abs(x - thr) > MARGIN * thr, (name, thr, x)
            recs.append(rec)
        write_fixture(name, dict(name=name, em=name, output=output_context(g), thresholds=recs, lines=sorted(seen)))
    return third


def root_ns_cases():
    ref = le.reference()
    L = len(ref)
    R = [(4, L)]
    shown = le.Builder(ref, False).run(5, 100, 140).run(5, 300, 300).o(500, [0.5, 0.5, 0.0, 0.0]).run(5, 900, 901).done()
    leaf0 = le.Builder(ref, False).run(5, 10, 10).o(20, [0.0, 0.25, 0.25, 0.5]).run(5, 30, 60).done()
    # root 0 = [1, 2], node 2 = [3, 4] at distance 0, leaf 3 at distance 0 (no error model: a single-list leaf)
    up, children = [None, 0, 0, 2, 2], [[1, 2], [], [3, 4], [], []]
    dist = [0.0, 1e-4, 0.0, 0.0, 2e-4]
    pv = [shown, R, shown, leaf0, R]
    ur, ul = [R, None, R, None, None], [R, None, R, None, None]
    five = dict(root=0, up=up, children=children, dist=dist, mutations=[[] for _ in up], nMinor=[0] * 5,
                probVect=[ser_list(q) for q in pv], probVectUpRight=[None if q is None else ser_list(q) for q in ur],
                probVectUpLeft=[None if q is None else ser_list(q) for q in ul], probVectTotUp=[None] * 5, n=5)
    lone = le.Builder(ref, False).run(5, 1, 3).o(700, [0.1, 0.2, 0.3, 0.4]).run(5, L, L).done()
    one = dict(root=0, up=[None], children=[[]], dist=[0.0], mutations=[[]], nMinor=[0], probVect=[ser_list(lone)],
               probVectUpRight=[None], probVectUpLeft=[None], probVectTotUp=[None], n=1)
    return [("five_nodes", five), ("lone_root", one)]


def run_root_ns(third):
    g = mge.cat_globals()
    mge.set_model(g, dict(le.model("unrest")))
    cases, seen = [], set()
    for label, snap in root_ns_cases():
        tree = mge.as_tree(snap)
        tree.name = list(range(snap["n"]))
        recs = []
        for thr in (0.0, 0.01, third):
            err, lines = traced_mat(g, tree, snap["root"], thr)
            assert err is None, (label, err)
            seen.update(lines)
            recs.append(records_of(g, tree, snap["root"], thr))
        assert recs[0]["Ns"][snap["root"]], label
        cases.append(dict(label=label, tree=snap, thresholds=recs))
    five = cases[0]["thresholds"][0]["Ns"]
    assert five[0] == [[100, 140], 300, [900, 901]] and five[2] == five[0] and five[3] == [10, 20, [30, 60]], five
    assert cases[1]["thresholds"][0]["Ns"][0] == [[1, 3], 700, len(le.reference())], cases[1]["thresholds"][0]["Ns"]
    write_fixture("root_ns", dict(name="root_ns", context=mge.context_of(g), model=mge.model_of(g), output=output_context(g),
                                  cases=cases, lines=sorted(seen)))


def write_arms():
    reach = {str(a): [] for a in APPEND_LINES}
    thirds = set()
    for path in sorted(glob.glob(os.path.join(HERE, "mat_*.json.gz"))):
        with gzip.open(path, "rt") as fh:
            fx = json.load(fh)
        for a in fx["lines"]:
            reach[str(a)].append(fx["name"])
        if fx.get("thresholds"):
            thirds.add(fx["thresholds"][2]["minMutProb"])
    assert len(thirds) == 1, thirds
    missed = [a for a in APPEND_LINES if not reach[str(a)]]
    print(f"{len(APPEND_LINES)} appending lines; not reached: {missed}", flush=True)
    with open(os.path.join(HERE, "mat_arms.json"), "w") as fh:
        json.dump(dict(lines=list(APPEND_LINES), reached=reach, unreached=missed, thresholds=[0.0, 0.01, thirds.pop()],
                       margin=MARGIN), fh, indent=1)


if __name__ == "__main__":
    names = sys.argv[1:] or em_names()
    run_root_ns(run_all(names))
    write_arms()
