"""Which branches the EM step, the mutation events and the error report walk, and in which order
(maple_amd/csrc/branch_walk_plan.h) on the CPU: tests/branch_walk_plan_main.cpp, compiled on its own with the host sanitizers and
run as a child process.  gather() must give what the reference's own loops give -- expectationMaximizationCalculationRates,
M:10138-10155 and M:10808-10848, and calculateErrorProbabilities, M:9801-9812 and M:10006-10020 -- written out in Python below
with the reference's variable names."""
import gzip
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
GOLDEN = os.path.join(HERE, "golden")
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TREES = sorted(f[len("update_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("update_"))
EM, EVENTS, ERRORS = 0, 1, 2
OK, BAD_ARG, BAD_STATE = 0, 1, 2


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/branch_walk_plan_main.cpp"
    exe = str(tmp_path_factory.mktemp("branch_walk_plan") / "branch_walk_plan_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(HERE, "branch_walk_plan_main.cpp")])
    return exe


class Tree:
    """the columns maple_tree_upload keeps on the host; lists: lower[v] = v, upLeft[v] = n + v and upRight[v] = 2n + v of an
    internal node, so that a row names its lists' owner and side"""

    def __init__(self, n, root, c0, c1, dist=None, mutations=None, nMinor=None, up=None):
        self.n, self.root, self.c0, self.c1 = n, root, list(c0), list(c1)
        self.dist = [float(d or 0.0) for d in dist] if dist is not None else [1e-4 * (1 + v % 7) for v in range(n)]
        if up is None:
            up = [-1] * n
            for v in range(n):
                for ch in (c0[v], c1[v]):
                    if 0 <= ch < n and ch != root:
                        up[ch] = v
        self.up = list(up)
        self.lower = list(range(n))
        self.upLeft = [n + v if c0[v] >= 0 else -1 for v in range(n)]
        self.upRight = [2 * n + v if c0[v] >= 0 else -1 for v in range(n)]
        self.nLists = 3 * n
        has = [bool(m) for m in mutations] if mutations is not None else [False] * n
        self.mut, k = [], 0
        for v in range(n):
            self.mut.append(k if has[v] else -1)
            k += has[v]
        self.nMutLists = k
        self.nMinor = list(nMinor) if nMinor is not None else None
        self._ref = None               # (as_reference() once the columns stand)

    def line(self, U):
        cols = [self.up, self.c0, self.c1, [repr(d) for d in self.dist], self.lower, self.upLeft, self.upRight, self.mut]
        if self.nMinor is not None:
            cols.append(self.nMinor)
        head = [self.n, self.root, int(U), self.nLists, self.nMutLists, int(self.nMinor is not None)]
        return "G " + " ".join(map(str, head)) + " " + " ".join(" ".join(map(str, c)) for c in cols)

    def as_reference(self):
        """(up, children, dist, mutations, minorSequences, probVect, probVectUpRight, probVectUpLeft) in the reference's form"""
        if self._ref is None:
            self._ref = self._as_reference()
        return self._ref

    def ref_nodes(self):
        """per node: nearest_reference (memoised down from the root would be faster; the trees here are small or chains of tips)"""
        up, _, _, mutations = self.as_reference()[:4]
        out = [None] * self.n
        for v in range(self.n):
            path, u = [], v
            while u is not None and out[u] is None and not mutations[u]:
                path.append(u)
                u = up[u]
            r = -1 if u is None else (u if mutations[u] else out[u])
            for x in path:
                out[x] = r
            if mutations[v]:
                out[v] = v
        return out

    def _as_reference(self):
        up = [None if self.up[v] < 0 else self.up[v] for v in range(self.n)]
        children = [[] if self.c0[v] < 0 else [self.c0[v], self.c1[v]] for v in range(self.n)]
        mutations = [[1] if m >= 0 else [] for m in self.mut]
        minor = [[0] * (self.nMinor[v] if self.nMinor is not None else 0) for v in range(self.n)]
        return up, children, self.dist, mutations, minor, self.lower, self.upRight, self.upLeft


def run(program, jobs):
    """jobs: (tree, U) -> per job and rule (EM, EVENTS, ERRORS) (status, message) or (0, dict of what gather() returned)"""
    text = "\n".join(t.line(U) for t, U in jobs) + "\n"
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]                # (a sanitizer report is a non-zero exit)
    out = []
    lines = r.stdout.splitlines()
    assert len(lines) == 3 * len(jobs)
    for k, line in enumerate(lines):
        rule = k % 3
        w = line.split()
        assert w[0] == "G"
        if w[1] != "0":
            out.append((int(w[1]), " ".join(w[2:])))
            continue
        numTips, nRows, nPass, nLeaves = (int(x) for x in w[2:6])
        p = 6 + 7 * nRows
        r7 = w[6:p]
        rows = list(zip(map(int, r7[0::7]), map(int, r7[1::7]), map(int, r7[2::7]), map(int, r7[3::7]), map(float.fromhex, r7[4::7]),
                        map(int, r7[5::7]), map(int, r7[6::7])))
        rest = [int(x) for x in w[p:]]
        assert len(rest) == nPass + nLeaves + (nRows if rule == ERRORS else 0)
        out.append((0, dict(numTips=numTips, rows=rows, passIdx=rest[:nPass], leaves=rest[nPass:nPass + nLeaves],
                            itemLeaf=rest[nPass + nLeaves:])))
    return [out[k:k + 3] for k in range(0, len(out), 3)]


def nearest_reference(up, mutations, v):
    """v's nearest ancestor-or-self with mutations in the tree as it stands (whose accumulated list is the reference's
    mutationsList while it is at v, M:10107-10109 and M:10828-10848), -1 if there is none"""
    while v is not None:
        if mutations[v]:
            return v
        v = up[v]
    return -1


def reference_walk(root, up, children, first=0):
    """the loop both reference functions share (direction 0: from the parent, 1: from a child): the nodes in the order it meets
    them in direction 0.  first = 0 is the reference (children[node][0] first); first = 1 is the mirror image."""
    order = []
    node, lastNode, direction = root, None, 0
    while node is not None:
        if direction == 0:
            order.append(node)
            if children[node]:
                node = children[node][first]
            else:
                lastNode = node
                node = up[node]
                direction = 1
        else:
            if lastNode == children[node][first]:
                node = children[node][1 - first]
                direction = 0
            else:
                lastNode = node
                node = up[node]
                direction = 1
    return order


def reference_em(t, usingErrorRate, trackMutations, first):
    """M:10138-10155 (and, under trackMutations, the else of M:10808): rows (node, probVectP, probVectC, mutations, dist,
    leafMinor), numTips"""
    up, children, dist, mutations, minorSequences, probVect, probVectUpRight, probVectUpLeft = t.as_reference()
    rows, numTips, ref = [], 0, t.ref_nodes()
    for node in reference_walk(t.root, up, children, first):
        if len(children[node]) == 0:
            nodeIsLeaf = True
            numTips += 1 + len(minorSequences[node])
        else:
            nodeIsLeaf = False
        leafMinor = len(minorSequences[node]) if nodeIsLeaf else -1
        if (dist[node] or (usingErrorRate and nodeIsLeaf)) and up[node] is not None:
            if node == children[up[node]][0]:
                probVectP = probVectUpRight[up[node]]
            else:
                probVectP = probVectUpLeft[up[node]]
            rows.append((node, probVectP, probVect[node], t.mut[node] if mutations[node] else -1, dist[node], leafMinor, ref[node]))
        elif trackMutations:                                                   # building Ns vectors for nodes with branch length 0
            rows.append((node, -1, probVect[node], -1, dist[node], leafMinor, ref[node]))
    return rows, numTips


def reference_errors(t):
    """M:9801-9812: the leaves as the report names them, and the rows of those without minor sequences"""
    up, children, dist, mutations, minorSequences, probVect, probVectUpRight, probVectUpLeft = t.as_reference()
    leaves, rows, itemLeaf, ref = [], [], [], t.ref_nodes()
    for node in reference_walk(t.root, up, children):
        if len(children[node]) == 0:
            if len(minorSequences[node]) > 0:
                pass
            elif up[node] is not None:                                         # (a root without children: the reference fails on up[root])
                if node == children[up[node]][0]:
                    probVectP = probVectUpRight[up[node]]
                else:
                    probVectP = probVectUpLeft[up[node]]
                itemLeaf.append(len(leaves))
                rows.append((node, probVectP, probVect[node], t.mut[node] if mutations[node] else -1, dist[node],
                             len(minorSequences[node]), ref[node]))
            leaves.append(node)
    return leaves, rows, itemLeaf


def check(program, trees, Us=(False, True), mirror=True):
    """every rule on every tree against the loops above"""
    jobs = [(nm, U) for nm in sorted(trees) for U in Us]
    got = run(program, [(trees[nm], U) for nm, U in jobs])
    by = {}
    for (nm, U), rule, (status, g) in ((j, rule, res[rule]) for j, res in zip(jobs, got) for rule in (EM, EVENTS, ERRORS)):
        t = trees[nm]
        assert status == 0, (nm, rule, U, g)
        by[nm, rule, U] = g
        if rule == ERRORS:
            leaves, rows, itemLeaf = reference_errors(t)
            assert g["leaves"] == leaves and g["itemLeaf"] == itemLeaf, (nm, U)
        else:
            # The EM step's launch order is the mirror image of the reference's (children[1] first): its totals are sums over the
            # branches, so their values do not depend on it, but k_em_walk adds them block by block, so their bits do, and the
            # call has had this order since it exists.  The events are laid out by node id: they keep the reference's order.
            rows, numTips = reference_em(t, U, rule == EVENTS, first=1 if rule == EM else 0)
            assert g["numTips"] == numTips, (nm, rule, U)
            if rule == EM and mirror:                                          # the same branches either way
                assert sorted(rows) == sorted(reference_em(t, U, False, first=0)[0]), (nm, U)
        assert g["rows"] == rows, (nm, rule, U)
        assert g["passIdx"] == [k for k, r in enumerate(rows) if r[3] >= 0], (nm, rule, U)
    return by


def fixture_tree(name):
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        t = json.load(fh)["tree"]
    n = len(t["up"])
    return Tree(n, t["root"], [c[0] if c else -1 for c in t["children"]], [c[1] if c else -1 for c in t["children"]], t["dist"],
                t["mutations"], t["nMinor"], [-1 if u is None else u for u in t["up"]])


def caterpillar(tips, left, **kw):
    """internal node i is node 2i, its tip 2i+1, the last tip 2(tips-1); left: the chain runs through children[0]"""
    m = tips - 1
    n = 2 * m + 1
    c0, c1 = [-1] * n, [-1] * n
    for i in range(m):
        c0[2 * i], c1[2 * i] = (2 * i + 2, 2 * i + 1) if left else (2 * i + 1, 2 * i + 2)
    return Tree(n, 0, c0, c1, **kw)


SEVEN = (7, 0, [1, 3, 5, -1, -1, -1, -1], [2, 4, 6, -1, -1, -1, -1])


def small_trees():
    out = {nm: fixture_tree(nm) for nm in TREES}
    out["single"] = Tree(1, 0, [-1], [-1])
    out["three"] = Tree(3, 0, [1, -1, -1], [2, -1, -1])
    out["root_not_0"] = Tree(3, 2, [-1, -1, 0], [-1, -1, 1])
    out["seven"] = Tree(*SEVEN)
    # slots the root does not reach: a detached cherry (7, 8, 9), a lone slot (10) and a slot that names nodes of the tree as
    # its children (11) after the balanced seven; their columns are nonsense (no lists, a negative nMinor)
    un = Tree(12, 0, [1, 3, 5, -1, -1, -1, -1, 8, -1, -1, -1, 3], [2, 4, 6, -1, -1, -1, -1, 9, -1, -1, -1, 4],
              nMinor=[0] * 7 + [-3] * 5, up=[-1, 0, 0, 1, 1, 2, 2, -1, 7, 7, -1, -1])
    un.lower[7:] = [-1] * 5
    out["unreachable"] = un
    out["root_mut"] = Tree(*SEVEN, mutations=[[1], [], [1], [], [1], [], []])                # the root's own list is never passed
    # zero-length branches above internal nodes (1) and leaves (3, 6); leaves with minor sequences, one of them at distance 0
    out["zero_len"] = Tree(*SEVEN, dist=[0.0, 0.0, 2e-4, 0.0, 1e-4, 3e-4, 0.0], mutations=[[], [1], [], [1], [], [], [1]])
    out["minor"] = Tree(*SEVEN, dist=[0.0, 1e-4, 0.0, 0.0, 1e-4, 3e-4, 0.0], nMinor=[0, 0, 0, 2, 0, 1, 0],
                        mutations=[[], [], [], [1], [1], [1], []])
    out["cat_left_40"] = caterpillar(40, True)
    out["cat_right_40"] = caterpillar(40, False)
    return out


def test_there_are_eight_fixture_topologies():
    assert len(TREES) == 8


def test_rows_are_the_reference_loops(program):
    trees = small_trees()
    by = check(program, trees)
    for nm in TREES:                                                           # the fixtures do exercise the rules
        t = trees[nm]
        assert any(d == 0.0 for d in t.dist) and any(t.nMinor) and t.nMutLists > 0, nm
        assert len(by[nm, EM, True]["rows"]) > len(by[nm, EM, False]["rows"]) > 10, nm
        up, children = t.as_reference()[:2]
        assert len(by[nm, EVENTS, False]["rows"]) == len(reference_walk(t.root, up, children)), nm
        assert len(by[nm, ERRORS, True]["rows"]) < len(by[nm, ERRORS, True]["leaves"]), nm
    assert sum(1 for nm in TREES if by[nm, EM, True]["passIdx"]) >= 4           # reference branches among the walked ones
    g = by["single", EM, True]
    assert g["rows"] == [] and g["numTips"] == 1
    assert by["single", EVENTS, True]["rows"] == [(0, -1, 0, -1, trees["single"].dist[0], 0, -1)]
    assert by["single", ERRORS, True]["leaves"] == [0] and by["single", ERRORS, True]["rows"] == []
    d = trees["three"].dist
    assert by["three", EM, False]["rows"] == [(2, 3, 2, -1, d[2], 0, -1), (1, 6, 1, -1, d[1], 0, -1)]     # children[1] first; upLeft, upRight
    assert by["three", EVENTS, False]["rows"] == [(0, -1, 0, -1, d[0], -1, -1), (1, 6, 1, -1, d[1], 0, -1), (2, 3, 2, -1, d[2], 0, -1)]
    assert [r[0] for r in by["root_not_0", EVENTS, False]["rows"]] == [2, 0, 1]
    assert [r[0] for r in by["seven", EM, False]["rows"]] == [2, 6, 5, 1, 4, 3]
    assert by["seven", ERRORS, True]["leaves"] == [3, 4, 5, 6]
    assert [r[0] for r in by["unreachable", EVENTS, True]["rows"]] == [0, 1, 3, 4, 2, 5, 6]    # nothing of slots 7-11
    assert by["root_mut", EVENTS, True]["passIdx"] == [3, 4] and by["root_mut", EM, True]["passIdx"] == [0, 4]
    # a zero-length branch is walked only above a leaf, and only under an error model (M:10146)
    assert [r[0] for r in by["zero_len", EM, False]["rows"]] == [2, 5, 4]
    assert [r[0] for r in by["zero_len", EM, True]["rows"]] == [2, 6, 5, 4, 3]
    assert [r[1] for r in by["zero_len", EVENTS, False]["rows"]] == [-1, -1, -1, 8, 7, 16, -1]
    assert [r[3] for r in by["zero_len", EVENTS, True]["rows"]] == [-1, -1, 1, -1, -1, -1, 2]   # node 1's list is not passed
    # minor sequences: counted in numTips, kept out of the error report's items, leafMinor carries them to the EM walk
    assert by["minor", EM, True]["numTips"] == 4 + 3
    assert by["minor", ERRORS, True]["leaves"] == [3, 4, 5, 6] and by["minor", ERRORS, True]["itemLeaf"] == [1, 3]
    assert [r[5] for r in by["minor", EM, True]["rows"]] == [0, 1, -1, 0, 2]


@pytest.mark.parametrize("left", [True, False])
def test_a_200000_tip_caterpillar_needs_no_recursion(program, left):
    t = caterpillar(200000, left)
    by = check(program, {"cat": t}, Us=(True,), mirror=False)
    assert len(by["cat", EVENTS, True]["rows"]) == t.n and len(by["cat", EM, True]["rows"]) == t.n - 1
    assert len(by["cat", ERRORS, True]["leaves"]) == 200000 and by["cat", EM, True]["numTips"] == 200000


def test_columns_that_are_no_tree(program):
    bad = [Tree(3, 0, [1, -1, -1], [-1, -1, -1]),                              # one child only
           Tree(3, 0, [1, -1, -1], [5, -1, -1]),                               # a child out of range
           Tree(3, 0, [1, -1, -1], [1, -1, -1]),                               # the same child twice
           Tree(7, 0, [1, 3, 5, -1, -1, -1, -1], [2, 4, 3, -1, -1, -1, -1]),   # a node reached twice
           Tree(3, 0, [1, 0, -1], [2, 2, -1]),                                 # a cycle through the root
           Tree(3, 5, [1, -1, -1], [2, -1, -1]),                               # the root is no node
           Tree(3, 0, [1, -1, -1], [2, -1, -1], up=[-1, 0, 1]),                # a child that does not point back
           Tree(3, 0, [1, -1, -1], [2, -1, -1], up=[1, 0, 0])]                 # a root with a parent
    got = run(program, [(t, True) for t in bad])
    for status, msg in (res for three in got for res in three):
        assert status == BAD_STATE and "the columns are no tree" in msg and msg.startswith("node "), msg


def test_refusals_name_the_node(program):
    def seven(**kw):
        return Tree(*SEVEN, **kw)
    neg = seven(nMinor=[0, 0, 0, 0, -2, 0, 0])
    no_upper = seven()
    no_upper.upLeft[1] = -1                                                    # the parent list of node 4 (children[1] of node 1)
    big_upper = seven()
    big_upper.upRight[2] = big_upper.nLists                                    # the parent list of node 5
    no_lower = seven()
    no_lower.lower[6] = -1
    inner_lower = seven()
    inner_lower.lower[2] = inner_lower.nLists                                  # an internal node: an item of EM and the events
    bad_mut = seven(mutations=[[], [], [], [1], [], [], []])
    bad_mut.mut[3] = 5
    cases = [(neg, (EM, EVENTS, ERRORS), BAD_ARG, "nMinor[4] = -2"),
             (no_upper, (EM, EVENTS, ERRORS), BAD_STATE, "node 4: the branch above it has no upper list of its parent"),
             (big_upper, (EM, EVENTS, ERRORS), BAD_STATE, "node 5: the branch above it has no upper list of its parent"),
             (no_lower, (EM, EVENTS, ERRORS), BAD_STATE, "node 6 has no lower list"),
             (inner_lower, (EM, EVENTS), BAD_STATE, "node 2 has no lower list"),
             (bad_mut, (EM, EVENTS, ERRORS), BAD_STATE, "node 3: mutList[] = 5 is not a mutation-list id (have 1)")]
    got = run(program, [(t, True) for t, _, _, _ in cases])
    for (t, rules, status, msg), three in zip(cases, got):
        for rule in (EM, EVENTS, ERRORS):
            if rule in rules:
                assert three[rule] == (status, msg)
            else:
                assert three[rule][0] == OK                                    # (the report walks leaves only)


def test_frames_follow_a_patch_that_moves_a_clade(program):
    """The EM step derives the reference nodes' lists once per upload; the frame of an item is its nearest ancestor-or-self with
    mutations in the columns as they stand at the call.  An SPR move applied by a patch (the same number of nodes) that carries
    a plain clade across a reference node's boundary must change the clade's frame."""
    # 0 -> (1, 2); 1 -> (3, 4); 2 -> (5, 6); 5 -> (7, 8): node 1 and node 5 have mutations
    mutations = [[], [1], [], [], [], [1], [], [], []]
    t = Tree(9, 0, [1, 3, 5, -1, -1, 7, -1, -1, -1], [2, 4, 6, -1, -1, 8, -1, -1, -1], mutations=mutations)
    # the move: leaf 4 (in node 1's frame) and leaf 6 (in no frame) change places
    moved = Tree(9, 0, [1, 3, 5, -1, -1, 7, -1, -1, -1], [2, 6, 4, -1, -1, 8, -1, -1, -1], mutations=mutations)
    assert moved.up[6] == 1 and moved.up[4] == 2
    by = check(program, {"t": t, "moved": moved})                              # (every row's refNode against nearest_reference)
    for rule in (EM, EVENTS):
        before = {r[0]: r[6] for r in by["t", rule, True]["rows"]}
        after = {r[0]: r[6] for r in by["moved", rule, True]["rows"]}
        assert [before[v] for v in range(1, 9)] == [1, -1, 1, 1, 5, -1, 5, 5]
        assert [after[v] for v in range(1, 9)] == [1, -1, 1, -1, 5, 1, 5, 5]
    # the root's own mutations are a frame too
    assert {r[6] for r in check(program, {"root_mut": Tree(*SEVEN, mutations=[[1]] + [[]] * 6)})["root_mut", EVENTS, True]["rows"]} == {0}
    by = check(program, {nm: fixture_tree(nm) for nm in TREES}, Us=(True,))
    assert sum(1 for nm in TREES if len({r[6] for r in by[nm, EM, True]["rows"]}) >= 2) >= 4   # fixtures with more than one frame
