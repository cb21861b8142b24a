"""The branch-length sweep's logic (maple_amd/csrc/sweep_plan.h) on the CPU: tests/sweep_plan_main.cpp, compiled on its own with
the host sanitizers.  blen_verdict against the reference's rule written out in Python (same fp64 operations), sweep_order
against the recorded update orders of the 8 fixture trees, and the driver on a toy model of lists-as-version-numbers: every
chunk size, and the adaptive policy, must give what one estimate at a time gives."""
import gzip
import json
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
GOLDEN = os.path.join(HERE, "golden")
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TREES = sorted(f[len("update_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("update_"))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/sweep_plan_main.cpp"
    exe = str(tmp_path_factory.mktemp("sweep_plan") / "sweep_plan_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(HERE, "sweep_plan_main.cpp")])
    return exe


def run(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def load(kind, name):
    with gzip.open(os.path.join(GOLDEN, f"{kind}_{name}.json.gz"), "rt") as fh:
        return json.load(fh)


_topo = {}


def topology(name):
    """(n, root, up, c0, c1) of a fixture tree"""
    if name not in _topo:
        t = load("search", name)["tree"]
        n = len(t["up"])
        up = [-1 if u is None else u for u in t["up"]]
        c0 = [c[0] if c else -1 for c in t["children"]]
        c1 = [c[1] if c else -1 for c in t["children"]]
        _topo[name] = (n, t["root"], up, c0, c1)
    return _topo[name]


def toy_trees():
    out = {nm: topology(nm) for nm in TREES}
    out["three"] = (3, 0, [-1, 0, 0], [1, -1, -1], [2, -1, -1])                      # a root whose children are tips
    out["single"] = (1, 0, [-1], [-1], [-1])
    # a caterpillar of 40 tips: internal node i has the tip 2i+1 and the next internal node (or the last tip) as children
    m = 39
    up, c0, c1 = [-1] * (2 * m + 1), [-1] * (2 * m + 1), [-1] * (2 * m + 1)
    for i in range(m):
        node, tip, nxt = 2 * i, 2 * i + 1, 2 * i + 2
        c0[node], c1[node] = (tip, nxt) if i % 2 == 0 else (nxt, tip)
        up[tip] = up[nxt] = node
    out["caterpillar"] = (2 * m + 1, 0, up, c0, c1)
    # seven nodes, balanced: the smallest tree with swept branches on both sides of the root
    out["seven"] = (7, 0, [-1, 0, 0, 1, 1, 2, 2], [1, 3, 5, -1, -1, -1, -1], [2, 4, 6, -1, -1, -1, -1])
    return out


def py_verdict(cur, t, is_false):
    """M:8835 / 8869-8883 with the reference's own expressions"""
    best = False if is_false else t
    dist = cur
    if best or dist:
        if (not best) or (not dist) or dist / best > 1.01 or dist / best < 0.99:
            return True, float(best or 0.0)
    return False, float(best or 0.0)


def test_blen_verdict_table(program):
    import math
    b = 3.3e-5
    cases = [(0.0, 0.0, 0), (0.0, 0.0, 1), (0.0, 1e-5, 1),                          # both zero (False and 0.0 alike)
             (b, 0.0, 1), (b, 5e-5, 1), (b, 0.0, 0),                                 # positive to zero: False, and a plain 0.0
             (0.0, b, 0),                                                            # zero to positive
             (b, b, 0), (b * 1.5, b, 0), (b * 0.5, b, 0)]
    # ratios 1.01 and 0.99 exactly, and one ulp to either side: cur is searched for so that cur / best IS the double wanted
    for want in (1.01, 0.99):
        cur = want * b
        while cur / b > want:
            cur = math.nextafter(cur, 0.0)
        while cur / b < want:
            cur = math.nextafter(cur, math.inf)
        assert cur / b == want
        lo = cur
        while lo / b == want:
            lo = math.nextafter(lo, 0.0)
        hi = cur
        while hi / b == want:
            hi = math.nextafter(hi, math.inf)
        cases += [(cur, b, 0), (lo, b, 0), (hi, b, 0)]
    exact = {(c, t): py_verdict(c, t, False)[0] for c, t, f in cases[-6:]}
    assert sorted(exact.values()) == [False, False, False, False, True, True]   # at 1.01 / 0.99 and inside: kept; outside: updated
    out = run(program, [f"V {float(c).hex()} {float(t).hex()} {f}" for c, t, f in cases])
    assert len(out) == len(cases)
    for (c, t, f), line in zip(cases, out):
        k, upd, best = line.split()
        want_upd, want_best = py_verdict(c, t, bool(f))
        assert k == "V" and bool(int(upd)) == want_upd and float.fromhex(best) == want_best, (c, t, f, line)
    # the cases the issue names, by value
    got = [bool(int(line.split()[1])) for line in out]
    assert got[:7] == [False, False, False, True, True, True, True]


def test_next_chunk_bounds(program):
    lines = [f"N {cur} {used} {broke}" for cur in (4, 5, 256, 1000, 1024) for used in (0, 1, 3, 100, 256, 1024) for broke in (0, 1)
             if used <= cur]
    out = run(program, lines)
    for ln, o in zip(lines, out):
        cur, used, broke = (int(x) for x in ln.split()[1:])
        nxt = int(o.split()[1])
        assert 4 <= nxt <= 1024, (ln, o)
        if broke:
            assert nxt <= cur, (ln, o)                                           # shrinks, towards the run that was used
            assert nxt == max(4, min(cur, 2 * max(used, 1))), (ln, o)
        elif used >= cur:
            assert nxt == min(1024, max(cur, 2 * cur)), (ln, o)                  # grows after a chunk used in full


def py_order(root, c0, c1):
    if c0[root] < 0:
        return []
    stack = []
    for ch in (c0[root], c1[root]):
        if c0[ch] >= 0:
            stack += [c0[ch], c1[ch]]
    order = []
    while stack:
        v = stack.pop()
        order.append(v)
        if c0[v] >= 0:
            stack += [c0[v], c1[v]]
    return order


def test_sweep_order(program):
    trees = toy_trees()
    names = sorted(trees)
    out = run(program, ["O %d %d %s %s" % (n, root, " ".join(map(str, c0)), " ".join(map(str, c1)))
                        for n, root, up, c0, c1 in (trees[nm] for nm in names)])
    orders = {}
    for nm, line in zip(names, out):
        w = line.split()
        assert w[:2] == ["O", "1"], nm
        orders[nm] = [int(x) for x in w[2:]]
        n, root, up, c0, c1 = trees[nm]
        assert orders[nm] == py_order(root, c0, c1), nm
    assert orders["three"] == [] and orders["single"] == [] and orders["seven"] == [6, 5, 4, 3]
    # the recorded sweeps: every node the reference repaired, the root's children aside, in visiting order
    n_checked = 0
    for nm in TREES:
        n, root, up, c0, c1 = trees[nm]
        pos = {v: i for i, v in enumerate(orders[nm])}
        recs = list(load("update", nm).get("blen_full_sweeps", []))
        path = os.path.join(GOLDEN, f"blen_rounds_{nm}.json.gz")
        assert os.path.exists(path), path
        recs += load("blen_rounds", nm)["sweeps"]
        for rec in recs:
            seq = list(rec["update_order"])
            kids = [c0[root], c1[root]]
            if seq[:2] == kids:
                seq = seq[2:]
            assert all(v in pos for v in seq), nm
            assert [pos[v] for v in seq] == sorted(set(pos[v] for v in seq)), nm    # strictly increasing: each once, in order
            assert len(seq) == rec["updates"], nm
            n_checked += len(seq)
    assert n_checked > 1000
    # not a tree: a node with one child, a child out of range, a node reached twice
    bad = run(program, ["O 3 0 1 -1 -1 -1 -1 -1", "O 3 0 1 -1 -1 5 -1 -1", "O 7 0 1 3 5 -1 -1 -1 -1 2 4 3 -1 -1 -1 -1"])
    assert [ln.split()[1] for ln in bad] == ["0", "0", "0"]


def drive(program, tree, seed, chunk, sweeps, dirty):
    n, root, up, c0, c1 = tree
    line = "D %d %d %d %d %d %s %s %s %s" % (n, root, seed, chunk, sweeps, " ".join(map(str, up)), " ".join(map(str, c0)),
                                             " ".join(map(str, c1)), " ".join(map(str, dirty)))
    out = run(program, [line])
    assert len(out) == sweeps
    res = []
    for ln in out:
        head, order, dist, flags = ln.split("|")
        h = head.split()
        assert h[0] == "S"
        res.append(dict(updates=int(h[1]), computed=int(h[2]), used=int(h[3]), repairs=int(h[4]), launches=int(h[5]),
                        order=order.split(), dist=dist.split(), dirty=flags.split()))
    return res


@pytest.mark.parametrize("name", sorted(toy_trees()))
def test_driver_chunking_never_changes_results(program, name):
    tree = toy_trees()[name]
    n = tree[0]
    rng = random.Random(5)
    inputs = [[1] * n, [int(rng.random() < 0.3) for _ in range(n)], [int(rng.random() < 0.05) for _ in range(n)]]
    total_updates = 0
    for k, dirty in enumerate(inputs):
        seed = 1000 + k
        naive = drive(program, tree, seed, -1, 5, dirty)
        one = drive(program, tree, seed, 1, 5, dirty)
        keys = ("updates", "order", "dist", "dirty", "repairs")
        assert [{q: s[q] for q in keys} for s in one] == [{q: s[q] for q in keys} for s in naive], "chunk 1 against the reference's loop"
        for s in one:
            assert s["computed"] == s["used"] == s["launches"]
            assert s["updates"] == len(s["order"]) == s["repairs"]
        total_updates += sum(s["updates"] for s in one)
        for chunk in (2, 7, 256, 0):
            got = drive(program, tree, seed, chunk, 5, dirty)
            for i, (g, w) in enumerate(zip(got, one)):
                for q in keys:
                    assert g[q] == w[q], (name, k, chunk, i, q)
                assert g["computed"] >= g["used"] == w["used"] and g["launches"] <= w["launches"]
    if name in ("three", "single"):
        assert total_updates == 0
    else:
        assert total_updates > 0
