"""The level loops of updatePartials and of the list rebuild (maple_amd/csrc/update_plan.h) on the CPU: tests/update_plan_main.cpp,
compiled on its own with the host sanitizers, plugs a toy model of lists into the plan (a list is a 64-bit content; merge,
pass-through-branch and root-vector hash their inputs, shorten keeps the content).  The oracle is the Python level loop of
maple_amd/tree_host.py (update_genome_lists / rebuild_genome_lists with native=False) driven by ToyDev below, a stand-in for
Device with the same toy model: list ids differ between the two sides (the Python loop numbers the unshortened lists too), so
the contents behind the ids are compared.  Where the Python loop raises (a None in the upper pass) the outcomes are stated."""
import os
import random
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import test_sweep_plan as SP
from maple_amd.tree_host import HostTree, rebuild_genome_lists, update_genome_lists

FLAGS = SP.FLAGS
M64 = (1 << 64) - 1
ARG, FATAL = 1, 2
FIVE = (5, 0, [-1, 0, 0, 1, 1], [1, 3, -1, -1, -1], [2, 4, -1, -1, -1])        # root -> (inner 1, tip 2), inner -> (tip 3, tip 4)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/update_plan_main.cpp"
    exe = str(tmp_path_factory.mktemp("update_plan") / "update_plan_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(SP.HERE, "update_plan_main.cpp")])
    return exe


def test_header_compiles_on_its_own(tmp_path):
    src = tmp_path / "only.cpp"
    src.write_text('#include "%s"\nint main() { return 0; }\n' % os.path.join(SP.ROOT, "maple_amd", "csrc", "update_plan.h"))
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", str(src)])


# ---- the toy model, as in update_plan_main.cpp ------------------------------------------------------------------------------

def hash_of(*xs):
    h = 0x9e3779b97f4a7c15
    for x in xs:
        h = ((h ^ x) * 0xbf58476d1ce4e5b9) & M64
        h ^= h >> 32
    return h


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64).tolist()


class ToyDev:
    """The batch operations the Python level loops call on a Device."""

    def __init__(self, coarse=0):
        self.content, self.coarse, self.rules, self.blen_queue = [], coarse, [], []

    def make(self, c):
        self.content.append(c)
        return len(self.content) - 1

    def is_none(self, h, b1, b2, ud):
        return any(((m >> ud) & 1) and (not z or (b1 == 0.0 and b2 == 0.0)) and (not hv or b1 == b2) and h % mod == rem
                   for m, z, hv, mod, rem in self.rules)

    def different(self, a, b):
        return a % self.coarse != b % self.coarse if self.coarse else a != b

    def merge_batch(self, l1, b1, t1, l2, b2, t2, ud):
        n = len(l1)
        wide = lambda x, kind: [kind(x)] * n if np.ndim(x) == 0 else [kind(y) for y in x]
        b1, b2 = wide(b1, float), wide(b2, float)
        c, out, ud = self.content, [], int(ud)
        for x, y, u, v, p, q, f, g in zip(np.asarray(l1).tolist(), np.asarray(l2).tolist(), b1, b2, bits(b1), bits(b2), wide(t1, int), wide(t2, int)):
            h = hash_of(1, c[x], p, f, c[y], q, g, ud)
            out.append(-1 if self.rules and self.is_none(h, u, v, ud) else self.make(h))
        return np.asarray(out, dtype=np.int32)

    def shorten_batch(self, ids):
        return np.asarray([self.make(self.content[i]) for i in np.asarray(ids).tolist()], dtype=np.int32)

    def differ_batch(self, a, b):
        c = self.content
        return np.asarray([self.different(c[x], c[y]) for x, y in zip(np.asarray(a).tolist(), np.asarray(b).tolist())], dtype=bool)

    def pass_branch_batch(self, ids, muts, direction_up):
        c = self.content
        return np.asarray([self.make(hash_of(2, c[i], m, int(bool(direction_up))))
                           for i, m in zip(np.asarray(ids).tolist(), np.asarray(muts).tolist())], dtype=np.int32)

    def root_vector_batch(self, lists, dist, tip, paths):
        c, out = self.content, []
        for i, b, t, p in zip(np.asarray(lists).tolist(), bits(dist), np.asarray(tip).tolist(), paths):
            out.append(self.make(hash_of(3, c[i], b, int(t), (p[0] if p else -1) & M64)))
        return np.asarray(out, dtype=np.int32)

    def blen_batch(self, up, low, tip):
        c, t, f = self.content, [], []
        for u, lo, tp in zip(np.asarray(up).tolist(), np.asarray(low).tolist(), np.asarray(tip).tolist()):
            h = hash_of(4, c[u], c[lo], int(tp))
            if self.blen_queue:
                x, isf = self.blen_queue.pop(0)
            else:
                x, isf = 1e-4 * float(1 + ((h >> 8) & 3)), (h & 7) == 0
            t.append(x)
            f.append(bool(isf))
        return np.asarray(t), np.asarray(f)


# ---- trees -------------------------------------------------------------------------------------------------------------------

def all_trees():
    out = SP.toy_trees()
    out["five"] = FIVE
    return out


def make_case(name, with_mut, dists=None):
    """a tree with lengths (some zero), the tips' lower contents and, with_mut, toy mutation-list ids on some branches"""
    n, root, up, c0, c1 = all_trees()[name]
    rng = random.Random(zlib.crc32(name.encode()))
    depth, order = [0] * n, [root]
    for v in order:
        for ch in (c0[v], c1[v]):
            if ch >= 0:
                depth[ch] = depth[v] + 1
                order.append(ch)
    reach = set(order)                                          # (a fixture's columns may hold slots that are not in the tree)
    dist = [0.0 if rng.random() < 0.08 else 1e-4 * (1 + rng.randrange(4)) * (1.0 + 0.01 * rng.randrange(8)) for _ in range(n)]
    if dists is not None:
        dist = [float(x) for x in dists]
    mut = [1000 + v if with_mut and rng.random() < 0.25 else -1 for v in range(n)]
    if with_mut and n > 1:
        mut[order[-1]] = 1000 + order[-1]                       # (at least one, also on the smallest trees)
    low = [10000 + v if c0[v] < 0 and v in reach else 0 for v in range(n)]
    return dict(name=name, nodes=sorted(reach), n=n, root=root, up=up, c0=c0, c1=c1, tip=[int(c < 0) for c in c0], mut=mut, depth=depth, dist=dist, low=low)


def tree_lines(t, coarse):
    row = lambda xs: " ".join(str(x) for x in xs)
    return ["tree %d %d %d" % (t["n"], t["root"], coarse), row(t["up"]), row(t["c0"]), row(t["c1"]), row(t["tip"]), row(t["mut"]),
            row(t["depth"]), row(float(x).hex() for x in t["dist"]), row(t["low"])]


def run(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def parse_state(line):
    """(lower, upRight, upLeft, totUp contents, dist) of an "S" line"""
    assert line.startswith("S"), line
    parts = [p.split() for p in line[1:].split("|")]
    assert len(parts) == 5
    return tuple([None if x == "-" else int(x) for x in p] for p in parts[:4]) + ([float.fromhex(x) for x in parts[4]],)


def parse_result(line):
    """("ok", value) or ("err", kind, message)"""
    if line.startswith("ok "):
        return ("ok", int(line[3:]))
    assert line.startswith("err "), line
    kind, msg = line[4:].split("|", 1)
    return ("err", int(kind), msg)


def parse_log(line):
    """the items calls of an "L" line, each a list of (node, kind); and the whole list of operations in order"""
    assert line.startswith("L"), line
    calls, ops = [], []
    for w in line[1:].split():
        if w == "I":
            calls.append([])
            ops.append("I")
        elif ":" in w:
            calls[-1].append(tuple(int(x) for x in w.split(":")))
        else:
            ops.append(w)
    return calls, ops


def parse_book(line):
    assert line.startswith("B"), line
    rep, vis, zero, _ = line[1:].split("|")
    return [int(x) for x in rep.split()], [int(x) for x in vis.split()], zero.strip() == "1"


def parse_stats(line):
    """the arm counters of the last repair (update_plan::Stats), by name"""
    return {k: int(v) for k, v in (x.split("=") for x in line[1:].split("|")[3].split())}


class Oracle:
    """the Python level loops on the toy model"""

    def __init__(self, t, coarse=0):
        self.t, self.dev = t, ToyDev(coarse)
        kids = [[a, b] if a >= 0 else [] for a, b in zip(t["c0"], t["c1"])]
        self.tree = HostTree(t["root"], [None if u < 0 else u for u in t["up"]], kids, t["dist"], [[] for _ in kids], [0] * t["n"],
                             None, None, None, None)
        self.tree.id_mut = np.asarray(t["mut"], dtype=np.int32)
        self.tree.id_lower = np.asarray([self.dev.make(c) if c else -1 for c in t["low"]], dtype=np.int32)
        self.base = tuple(np.asarray(x, dtype=np.int32) for x in rebuild_genome_lists(self.dev, self.tree, native=False))
        self.base_dist = self.tree.dist.copy()

    def reset(self):
        tr = self.tree
        tr.id_lower, tr.id_upRight, tr.id_upLeft, tr.id_totUp = (x.copy() for x in self.base)
        tr.dist = self.base_dist.copy()

    def state(self, cols=None):
        tr, c = self.tree, self.dev.content
        cols = cols or (tr.id_lower, tr.id_upRight, tr.id_upLeft, tr.id_totUp)
        return tuple([None if i < 0 else c[i] for i in np.asarray(x).tolist()] for x in cols) + (tr.dist.tolist(),)

    def repair(self, mods, changed):
        self.reset()
        for what, v, x in mods:
            if what == "dist":
                self.tree.dist[v] = x
            else:
                self.tree.id_lower[v] = self.dev.make(x)
        return update_genome_lists(self.dev, self.tree, list(changed), native=False)


def change_of(t, nodes, salt):
    """the edit that makes `nodes` changed: a new length (not the root's), and a new lower list for a tip"""
    mods = []
    for v in nodes:
        if v != t["root"]:
            mods.append(("dist", v, 3.3e-4 + 1e-6 * ((v + salt) % 7)))
        if t["tip"][v]:
            mods.append(("low", v, 5000000 + 4000 * salt + v))
    return mods


def mod_lines(mods):
    return ["dist %d %s" % (v, float(x).hex()) if what == "dist" else "low %d %d" % (v, x) for what, v, x in mods]


def parts_of(name):
    """the fixture topologies' changes go in several test cases each (the Python loop takes its time): one per 60 nodes"""
    return max(4, SP.topology(name)[0] // 60) if name in SP.TREES else 1


def change_sets(t, part):
    """every node of a toy tree; of a fixture topology at least 200 nodes (fixed seed; those next to the root among them, so that
    some coarse repairs reach it), a share per part with the root's children in each; and sets of 2, 5 and 50 changes"""
    rng = random.Random(7)
    if t["name"] in SP.TREES:
        near = [v for v in t["nodes"] if t["depth"][v] in (1, 2)]                 # (so that some coarse repairs reach the root)
        rest = [v for v in t["nodes"] if v not in near]
        singles = near + rng.sample(rest, min(len(rest), max(0, 200 - len(near))))
        assert len(singles) >= min(len(t["nodes"]), 200)
    else:
        singles = t["nodes"]
    sets = [[v] for v in singles]
    for k in (2, 5, 50):
        if len(t["nodes"]) >= k:
            sets.append(sorted(rng.sample(t["nodes"], k)))
    if t["name"] in SP.TREES:
        sets = [[v] for v in t["nodes"] if t["depth"][v] == 1] + sets[part::parts_of(t["name"])]
    return sets


# ---- 1, 2, 6: the repair against the Python loop, against the rebuild, and its bookkeeping -------------------------------------

@pytest.mark.parametrize("coarse", [0, 3])
@pytest.mark.parametrize("name,part", [(nm, p) for nm in sorted(all_trees()) for p in range(parts_of(nm))])
def test_repair_matches_the_python_loop_and_the_rebuild(program, name, part, coarse):
    """coarse: areVectorsDifferent compares the contents modulo 3, so that a repair stops early on a good share of its paths"""
    t = make_case(name, True)                                                       # (some branches carry mutation lists)
    sets = change_sets(t, part)
    lines = tree_lines(t, coarse) + ["rebuild 0", "save"]
    for k, nodes in enumerate(sets):
        lines += ["reset"] + mod_lines(change_of(t, nodes, k)) + ["repair %d %s" % (len(nodes), " ".join(map(str, nodes)))]
        if not coarse:
            lines.append("check")
    out = run(program, lines)
    orc = Oracle(t, coarse)
    assert parse_result(out[0]) == ("ok", 0) and parse_state(out[1]) == orc.state(orc.base)
    at, per = 3, 4 if coarse else 5
    assert len(out) == at + per * len(sets)
    stopped = reached = 0
    for k, nodes in enumerate(sets):
        mods = change_of(t, nodes, k)
        want_replaced = orc.repair(mods, nodes)
        res, state, log, book = out[at:at + 4]
        assert parse_result(res) == ("ok", want_replaced), (name, nodes)
        got = parse_state(state)
        assert got == orc.state(), (name, nodes)
        if not coarse:
            assert out[at + 4] == "same 1", (name, nodes)                          # the repair equals the plan's own rebuild
        # bookkeeping: what changed is reported as replaced; what was replaced or changed was visited; the flags are clear
        replaced, visited, zero = parse_book(book)
        orc.reset()
        for what, v, x in mods:
            if what == "dist":
                orc.tree.dist[v] = x
        before = orc.state()
        moved = {v for col_b, col_a in zip(before, got) for v in range(t["n"]) if col_b[v] != col_a[v]
                 and not (col_b is before[0] and t["tip"][v])}                      # (a tip's new lower list is the caller's edit)
        assert moved <= set(replaced), (name, nodes)
        assert set(nodes) <= set(visited) and set(replaced) <= set(visited)
        # phase A's frontier: from a changed node upwards, as far as the new lower list differs from the old one; phase B's todo
        # list: those, the changed nodes, and the child that sees a probVectUpRight / probVectUpLeft that was replaced
        differs = orc.dev.different
        entered = set(nodes)
        for v in nodes:
            p = t["up"][v]
            while p >= 0:
                entered.add(p)
                if not differs(got[0][p], before[0][p]):
                    break
                p = t["up"][p]
        for col, kid in ((1, t["c0"]), (2, t["c1"])):
            entered |= {kid[v] for v in t["nodes"] if got[col][v] != before[col][v]}
        assert entered <= set(visited), (name, nodes)
        assert zero
        for call in parse_log(log)[0]:                                              # per node: totUp, upRight, upLeft
            if call[0][1] != 3:
                assert call == sorted(call), (name, nodes)
        if t["root"] in replaced:
            reached += 1
        else:
            stopped += 1
        at += per
    if coarse and t["n"] > 7:
        assert stopped > 0 and reached > 0, (stopped, reached)                      # the stop rule is exercised both ways


@pytest.mark.parametrize("name", sorted(nm for nm, tr in all_trees().items() if tr[3][tr[1]] >= 0))     # (the root has children)
def test_keep_root_right_leaves_the_first_childs_side_alone(program, name):
    """Scratch::keepRootRight (the sweep's repair of the root's second child, as the reference's work list [(child, 2), (root, 0)]
    leaves it): with the root's child 1 lengthened the root's lower list and the child's own side come out as in the plain repair,
    the root's probVectUpRight and every upper list below child 0 stay what they were; the flag does nothing for child 0; and
    once it is switched off the same repair makes everything again (the plan's own rebuild agrees)."""
    t = make_case(name, True)
    root = t["root"]
    a, b = t["c0"][root], t["c1"][root]
    below_a, stack = set(), [a]
    while stack:
        v = stack.pop()
        below_a.add(v)
        stack += [k for k in (t["c0"][v], t["c1"][v]) if k >= 0]
    longer = lambda v: "dist %d %s" % (v, float(t["dist"][v] + 7.7e-4).hex())              # noqa: E731
    lines = tree_lines(t, 0) + ["rebuild 0", "save",
                                longer(b), "repair 1 %d" % b, "check",                       # 3-6: the plain repair
                                "reset", "keepright 1", longer(b), "repair 1 %d" % b,         # 7-10: child 1 with the flag
                                "keepright 0", "repair 1 %d" % b, "check",                   # 11-15: the flag off again
                                "reset", "keepright 1", longer(a), "repair 1 %d" % a, "check", "keepright 0"]   # 16-20: child 0
    out = run(program, lines)
    base = parse_state(out[1])
    plain = parse_state(out[4])
    assert parse_result(out[3])[0] == "ok" and out[7] == "same 1"
    kept = parse_state(out[9])
    assert parse_result(out[8])[0] == "ok"
    assert plain[1][root] != base[1][root] and kept[1][root] == base[1][root]               # probVectUpRight of the root
    assert kept[0][root] == plain[0][root] != base[0][root] and kept[2][root] == plain[2][root]   # its lower list, probVectUpLeft
    for v in range(t["n"]):
        for col in (1, 2, 3):
            if v in below_a:
                assert kept[col][v] == base[col][v], (v, col)
            elif v != root:
                assert kept[col][v] == plain[col][v], (v, col)
        assert kept[0][v] == plain[0][v] and kept[4][v] == plain[4][v]
    assert any(plain[col][v] != base[col][v] for v in below_a for col in (1, 2, 3))            # (the plain repair does go down there)
    assert "root_right_made=0" in out[11] and "root_right_made=1" in out[6]
    assert parse_state(out[13]) == plain and out[16] == "same 1"
    assert parse_result(out[17])[0] == "ok" and out[21] == "same 1"                            # child 0: the flag changes nothing


# ---- 3: the rebuild against the Python loop; the order of a level's items ------------------------------------------------------

@pytest.mark.parametrize("with_mut", [False, True])
@pytest.mark.parametrize("name", sorted(all_trees()))
def test_rebuild_matches_the_python_loop(program, name, with_mut):
    t = make_case(name, with_mut)
    out = run(program, tree_lines(t, 0) + ["rebuild 0"])
    orc = Oracle(t)
    assert parse_result(out[0]) == ("ok", 0)
    assert parse_state(out[1]) == orc.state(orc.base)
    if with_mut and t["n"] > 3:
        assert any(op.startswith("P") for op in parse_log(out[2])[1])                # the pass-through-branch arms ran
    # the batches: pass 1 from the deepest level, one batch of lower lists per level; pass 2 from depth 1, kind by kind -- all
    # probVectTotUp (branches of non-zero length), then all probVectUpRight, then all probVectUpLeft, ascending node within a kind
    levels = {}
    for v in t["nodes"]:
        levels.setdefault(t["depth"][v], []).append(v)
    want = []
    for d in sorted(levels, reverse=True):
        call = [(v, 3) for v in levels[d] if t["c0"][v] >= 0]
        if call:
            want.append(call)
    for d in sorted(levels):
        if d == 0:
            continue
        call = [(v, 0) for v in levels[d] if t["dist"][v] != 0.0]
        call += [(v, kind) for kind in (1, 2) for v in levels[d] if t["c0"][v] >= 0]
        if call:
            want.append(call)
    assert parse_log(out[2])[0] == want


# ---- 4: a None in the lower pass, between two zero-length branches --------------------------------------------------------------

LOWER_ZERO = "rules 1 1 1 0 1 0"          # a merge that is not upDown, between two lengths of zero, is None
UPPER_ZERO = "rules 1 2 1 0 1 0"          # an upDown merge between two lengths of zero is None
UPPER_ANY = "rules 1 2 0 0 1 0"           # every upDown merge is None
LOWER_ANY = "rules 1 1 0 0 1 0"
TOTUP_ANY = "rules 1 2 0 1 1 0"           # every upDown merge of two equal lengths (probVectTotUp: half the branch each) is None


def scripted(program, t, rules, blen, mods, changed, oracle=True):
    lines = tree_lines(t, 0) + ["rebuild 0", rules, "blen %d %s" % (len(blen), " ".join("%s %d" % (float(x).hex(), f) for x, f in blen))]
    lines += mod_lines(mods) + ["repair %d %s" % (len(changed), " ".join(map(str, changed))), "check"]
    out = run(program, lines)
    res = dict(result=parse_result(out[3]), state=parse_state(out[4]), log=parse_log(out[5]), book=parse_book(out[6]), stats=parse_stats(out[6]), same=out[7] == "same 1")
    assert res["book"][2], "flags left set"
    if oracle:
        orc = Oracle(t)
        orc.dev.rules = [tuple(int(x) for x in rules.split()[2:])]
        orc.dev.blen_queue = list(blen)
        try:
            res["py"] = ("ok", orc.repair(mods, changed))
            res["py_state"] = orc.state()
        except RuntimeError as e:
            res["py"] = ("raise", str(e))
    return res


@pytest.mark.parametrize("name", ["seven", "five"])
def test_none_in_the_lower_pass(program, name):
    n = all_trees()[name][0]
    d = [2e-4 + 1e-5 * v for v in range(n)]
    d[4] = 0.0                                                   # node 1's children are 3 and 4
    t = make_case(name, False, d)
    new3 = [("dist", 3, 0.0), ("low", 3, 77)]
    # the changed child (3) is estimated first; its length becomes non-zero: the other one is left alone, the merge runs again
    r = scripted(program, t, LOWER_ZERO, [(1.5e-4, 0)], new3, [3])
    assert r["result"] == r["py"] and r["state"] == r["py_state"] and r["same"]
    assert r["state"][4][3] == 1.5e-4 and r["state"][4][4] == 0.0
    assert r["log"][1][:3] == ["I", "E", "I"] and r["log"][0][:2] == [[(1, 3)], [(1, 3)]] and r["log"][1].count("E") == 1
    assert {3, 1} <= set(r["book"][0]) and {3, 1} <= set(r["book"][1])
    st = r["stats"]
    assert (st["rounds"], st["phaseA_none"], st["phaseA_reest_first"], st["phaseA_reest_second"]) == (1, 1, 1, 0), st
    assert st["items_mode0"] >= 2 and st["upper_none_totup"] + st["upper_none_upright"] + st["upper_none_upleft"] == 0, st
    # it stays at zero (False): the other child is estimated too
    r = scripted(program, t, LOWER_ZERO, [(1.5e-4, 1), (2.5e-4, 0)], new3, [3])
    assert r["result"] == r["py"] and r["state"] == r["py_state"] and r["same"]
    assert r["state"][4][3] == 0.0 and r["state"][4][4] == 2.5e-4 and r["log"][1][:4] == ["I", "E", "E", "I"]
    assert {3, 4, 1} <= set(r["book"][0])
    assert (r["stats"]["phaseA_none"], r["stats"]["phaseA_reest_first"], r["stats"]["phaseA_reest_second"]) == (1, 1, 1), r["stats"]
    # child 4 marked changed: it goes first
    d2 = list(d)
    d2[3] = 0.0
    t2 = make_case(name, False, d2)
    r = scripted(program, t2, LOWER_ZERO, [(1.5e-4, 0)], [("low", 4, 78)], [4])
    assert r["result"] == r["py"] and r["state"] == r["py_state"] and r["same"]
    assert r["state"][4][4] == 1.5e-4 and r["state"][4][3] == 0.0
    assert (r["stats"]["phaseA_reest_first"], r["stats"]["phaseA_reest_second"]) == (1, 0), r["stats"]
    # both stay at zero: the second merge is None as well
    r = scripted(program, t, LOWER_ZERO, [(0.0, 1), (0.0, 1)], new3, [3])
    assert r["result"] == ("err", FATAL, "None vector after updateBLen at node 1") and r["py"] == ("raise", "None vector after updateBLen")
    # a None from non-zero distances
    r = scripted(program, t, LOWER_ANY, [], [("low", 3, 77)], [3])
    assert r["result"] == ("err", FATAL, "None vector from non-zero distances in the lower merge at node 1 (the reference raises too)")
    assert r["py"][0] == "raise" and r["py"][1].startswith("None vector from non-zero distances in the lower merge")


# ---- 5: a None in the upper pass (the Python loop raises there: stated outcomes) --------------------------------------------------

@pytest.mark.parametrize("name", ["seven", "five"])
def test_none_in_the_upper_pass(program, name):
    n = all_trees()[name][0]
    d = [2e-4 + 1e-5 * v for v in range(n)]
    d[1] = d[3] = 0.0                                            # node 1 and its child 3: probVectUpLeft of 1 merges across both
    t = make_case(name, False, d)
    both = [("low", 3, 77), ("low", 4, 78)]
    # the node's own branch is estimated; it becomes non-zero: the node starts another round, which makes all its vectors anew
    r = scripted(program, t, UPPER_ZERO, [(1.5e-4, 0)], both, [3, 4], oracle=False)
    assert r["result"][0] == "ok" and r["same"]
    assert r["state"][4][1] == 1.5e-4 and r["state"][4][3] == 0.0 and r["log"][1].count("E") == 1
    calls, ops = r["log"]
    first = next(i for i, c in enumerate(calls) if (1, 2) in c)
    assert (1, 1) in calls[first] and (1, 0) not in calls[first]                     # (a zero-length branch has no probVectTotUp)
    later = [c for c in calls[first + 1:] if (1, 0) in c]
    assert later and (1, 1) in later[0] and (1, 2) in later[0]                       # the next round: the node's three vectors
    assert any((3, 0) in c for c in calls[first + 1:]) is False                      # (3 still hangs on a zero-length branch)
    assert any((4, 0) in c for c in calls[first + 1:])                               # its children follow, after the node
    assert r["state"][2][1] is not None and r["state"][3][1] is not None
    if name == "five":
        # nothing the first round computed for node 1 was stored.  Round 1: the lower lists of 1 and 0, probVectUpLeft of 0,
        # probVectTotUp of 2 and 4 (5); round 2: the lower list of 0, probVectUpLeft of 0, the three vectors of 1, probVectTotUp
        # of 2 and 4 (7)
        assert r["result"] == ("ok", 12)
    assert {1, 0} <= set(r["book"][1]) and 1 in r["book"][0]
    st = r["stats"]
    assert st["rounds"] == 2 and st["upper_none_upleft"] >= 1 and (st["upper_reest_node"], st["upper_reest_child"]) == (1, 0), st
    assert st["phaseA_none"] == 0 and st["items_mode2"] >= 2 and st["items_mode1"] >= 1, st
    # it stays at zero: the branch of the child that was being merged is estimated, and that child starts the next round
    r = scripted(program, t, UPPER_ZERO, [(0.0, 1), (2.5e-4, 0)], both, [3, 4], oracle=False)
    assert r["result"][0] == "ok" and r["same"]
    assert r["state"][4][1] == 0.0 and r["state"][4][3] == 2.5e-4 and r["log"][1].count("E") == 2
    assert r["state"][3][1] is None and r["state"][3][3] is not None                 # probVectTotUp: none at 1, one at 3 now
    assert {1, 0, 3} <= set(r["book"][1]) and {1, 3} <= set(r["book"][0])
    assert r["stats"]["rounds"] == 2 and (r["stats"]["upper_reest_node"], r["stats"]["upper_reest_child"]) == (1, 1), r["stats"]
    # neither can be lengthened
    r = scripted(program, t, UPPER_ZERO, [(0.0, 1), (0.0, 1)], both, [3, 4], oracle=False)
    assert r["result"] == ("err", FATAL, "None upper vector at node 1 and no branch length to lengthen")
    # a None upper vector from non-zero distances
    d2 = list(d)
    d2[3] = 2.3e-4
    r = scripted(program, make_case(name, False, d2), UPPER_ANY, [], [("low", 3, 77)], [3], oracle=False)
    assert r["result"] == ("err", FATAL, "None upper vector from non-zero distances at node 1 (the reference raises too)")
    # a None probVectTotUp: the node's branch is estimated (there is no child in that merge); False: nothing to lengthen
    d3 = [2e-4 + 1e-5 * v for v in range(n)]
    t3 = make_case(name, False, d3)
    r = scripted(program, t3, TOTUP_ANY, [(0.0, 1)], [("low", 3, 77)], [3], oracle=False)
    assert r["result"] == ("err", FATAL, "None upper vector at node 1 and no branch length to lengthen") and r["log"][1].count("E") == 1
    assert r["stats"]["upper_none_totup"] == 1 and (r["stats"]["upper_reest_node"], r["stats"]["upper_reest_child"]) == (1, 0), r["stats"]
    # ... and a script that keeps answering None, whatever the new length: the cap on the rounds
    r = scripted(program, t3, TOTUP_ANY, [(1e-4 + 1e-7 * i, 0) for i in range(2000)], [("low", 3, 77)], [3], oracle=False)
    assert r["result"] == ("err", FATAL, "updatePartials keeps finding inconsistent zero-length branches")
    assert r["log"][1].count("E") >= 64
    assert r["stats"]["rounds"] == 64 and r["stats"]["upper_none_totup"] >= 64, r["stats"]
    assert sum((0, 3) in c for c in r["log"][0]) == 64                                # one lower list of the root per round


# ---- 7: malformed columns: the argument error, and no access out of bounds (the sanitizers) -------------------------------------

def test_malformed_columns(program):
    t = make_case("seven", False, [2e-4] * 7)
    head = tree_lines(t, 0)

    def rebuild(*edit):
        return parse_result(run(program, head + list(edit) + ["rebuild 0"])[0])

    def repair(changed, *edit):
        out = run(program, head + ["rebuild 0"] + list(edit) + ["repair 1 %d" % changed])
        assert parse_book(out[6])[2], "flags left set after a failed call"
        return parse_result(out[3])

    assert rebuild("col c0 1 99") == ("err", ARG, "node 1: child 99 out of range or reached twice")
    assert rebuild("col c1 1 3") == ("err", ARG, "node 1: child 3 out of range or reached twice")
    assert rebuild("col c1 1 -1") == ("err", ARG, "node 1 has one child")
    assert rebuild("col lower 3 -1") == ("err", ARG, "tip 3 has no lower list")
    assert rebuild("col up 3 2") == ("err", ARG, "node 3 is a child of 1 but its `up` entry says 2")
    assert repair(3, "col up 3 99") == ("err", ARG, "node 3: parent index out of range")
    assert repair(3, "col up 3 -5") == ("err", ARG, "node 3: parent index out of range")
    assert repair(3, "col c1 1 99") == ("err", ARG, "node 1 has a changed child but no two (valid) children")
    assert repair(3, "col c1 1 -1") == ("err", ARG, "node 1 has a changed child but no two (valid) children")
    assert repair(1, "col c1 1 99") == ("err", ARG, "node 1: child index out of range")
    assert repair(1, "col c1 1 -1") == ("err", ARG, "node 1: child index out of range")
    # the same scratch serves the next call after a failure
    out = run(program, head + ["rebuild 0", "save", "col c1 1 99", "repair 1 3", "reset"] + mod_lines(change_of(t, [3], 0)) + ["repair 1 3", "check"])
    assert parse_result(out[3])[0] == "err" and parse_book(out[6])[2]
    assert parse_result(out[7])[0] == "ok" and parse_book(out[10])[2] and out[11] == "same 1"
