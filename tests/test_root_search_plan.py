"""The host-only halves of maple_tree_find_best_root (maple_amd/csrc/root_search_plan.h) on the CPU: tests/root_search_plan_main.cpp,
compiled on its own with the host sanitizers.  level_lists against a Python rendition of the same grouping, replay against a
transcription of the reference's search loop (findBestRoot, M:7782-7848) that takes its scores from a table."""
import math
import random
import shutil
import subprocess
import os

import pytest

from test_tree_lk_plan import FLAGS, HERE, TREES, as_reference, caterpillar, small_trees

NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/root_search_plan_main.cpp"
    exe = str(tmp_path_factory.mktemp("root_search_plan") / "root_search_plan_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(HERE, "root_search_plan_main.cpp")])
    return exe


def hexf(x):
    return "nan" if x != x else ("inf" if x == INF else ("-inf" if x == -INF else float(x).hex()))


def unhex(w):
    return float.fromhex(w)


def converse(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def tree_words(tree):
    n, root, c0, c1 = tree
    return "%d %d %s %s" % (n, root, " ".join(map(str, c0)), " ".join(map(str, c1)))


def run_levels(program, trees):
    out = []
    for line in converse(program, ["L " + tree_words(t) for t in trees]):
        w = line.split()
        assert w[0] == "L"
        if w[1] == "0":
            out.append(None)
            continue
        k = int(w[2])
        x = [int(v) for v in w[3:]]
        node, parent, side = x[:k], x[k:2 * k], x[2 * k:3 * k]
        m = x[3 * k]
        start = x[3 * k + 1:]
        assert len(start) == m
        out.append((node, parent, side, start))
    return out


def run_replay(program, cases):
    """cases: (tree, strict, fails, thrTopology, thrOptimization, thrConsecutive, score[n])"""
    lines = ["R %s %d %d %s %s %s %s" % (tree_words(t), int(strict), fails, hexf(a), hexf(b), hexf(cc), " ".join(hexf(x) for x in score))
             for t, strict, fails, a, b, cc, score in cases]
    out = []
    for line in converse(program, lines):
        w = line.split()
        assert w[0] == "R"
        k = int(w[4])
        out.append((int(w[1]), unhex(w[2]), int(w[3]), [int(v) for v in w[5:5 + k]], [unhex(v) for v in w[5 + k:5 + 2 * k]]))
        assert len(w) == 5 + 2 * k
    return out


# ---- level lists ------------------------------------------------------------------------------------------------------------------
def reference_levels(root, children):
    """the internal nodes below the root by depth (the root's internal children first); within a level in the order of the parents'
    items, side 0 before side 1; per node the item of its parent (-1 at the top) and the side it hangs on"""
    node, parent, side, start = [], [], [], []
    cur = [(ch, -1, i) for i, ch in enumerate(children[root])]
    while cur:
        nxt, first = [], len(node)
        for v, p, s in cur:
            if children[v]:
                nxt += [(children[v][0], len(node), 0), (children[v][1], len(node), 1)]
                node.append(v), parent.append(p), side.append(s)
        if len(node) > first:
            start.append(first)
        cur = nxt
    return node, parent, side, (start + [len(node)] if node else [])


def test_level_lists_are_the_rendition(program):
    trees = small_trees()
    names = sorted(trees)
    got = run_levels(program, [trees[nm] for nm in names])
    by = dict(zip(names, got))
    for nm in names:
        n, root, c0, c1 = trees[nm]
        up, children = as_reference(n, root, c0, c1)
        assert by[nm] == reference_levels(root, children), nm
        node, parent, side, start = by[nm]
        for k, v in enumerate(node):                                       # every item hangs where it says
            above = root if parent[k] < 0 else node[parent[k]]
            assert children[above][side[k]] == v and up[v] == above, (nm, k)
        assert sorted(node) == [v for v in range(n) if c0[v] >= 0 and up[v] is not None], nm     # every internal node below the root, once
        for a, b in zip(start, start[1:]):
            assert a < b                                                   # no empty level
    assert by["single"] == by["three"] == by["root_not_0"] == ([], [], [], [])
    assert by["seven"] == ([1, 2], [-1, -1], [0, 1], [0, 2])
    assert by["unreachable"] == by["seven"]                                # nothing of slots 7-11
    assert by["cat_left_40"][0] == list(range(2, 78, 2)) and by["cat_left_40"][2] == [0] * 38
    assert by["cat_right_40"][0] == list(range(2, 78, 2)) and by["cat_right_40"][2] == [1] * 38
    assert by["cat_left_40"][3] == list(range(39))                         # 38 levels of one item
    for nm in TREES:
        assert len(by[nm][0]) > 10, nm


@pytest.mark.parametrize("left", [True, False])
def test_a_200000_tip_caterpillar_needs_no_recursion(program, left):
    tree = caterpillar(200000, left)
    n, root, c0, c1 = tree
    node, parent, side, start = run_levels(program, [tree])[0]
    assert node == list(range(2, 2 * 199998 + 1, 2)) and parent == [-1] + list(range(199997))
    assert side == [0 if left else 1] * 199998 and start == list(range(199999))


def test_columns_that_are_no_tree(program):
    bad = [(3, 0, [1, -1, -1], [-1, -1, -1]),                              # one child only
           (3, 0, [1, -1, -1], [5, -1, -1]),                               # a child out of range
           (3, 0, [1, -1, -1], [1, -1, -1]),                               # the same child twice
           (7, 0, [1, 3, 5, -1, -1, -1, -1], [2, 4, 3, -1, -1, -1, -1]),   # a node reached twice
           (3, 0, [1, 0, -1], [2, 2, -1]),                                 # a cycle through the root
           (3, 5, [1, -1, -1], [2, -1, -1])]                               # the root is no node
    assert run_levels(program, bad) == [None] * len(bad)


# ---- the replay -------------------------------------------------------------------------------------------------------------------
def reference_replay(root, children, table, strictTopologyStopRules, allowedFailsTopology, thresholdLogLKtopology,
                     thresholdLogLKoptimizationTopology, thresholdLogLKconsecutivePlacement):
    """M:7739-7848 with the reference's own variables; where it computes `score` from merges it is read from ``table`` (by the
    child node), and a NaN there stands for a merge that raised (M:7838)"""
    bestNode = root
    nodesToVisit = []
    bestLKdiff = 0.0
    bestNodes = {}
    bestNodes[root] = 0.0
    if children[root]:
        child1 = children[root][0]
        child2 = children[root][1]
        if children[child1]:
            nodesToVisit.append((child1, bestLKdiff, 0))
        if children[child2]:
            nodesToVisit.append((child2, bestLKdiff, 0))
    nodesVisitedRoot = 1
    while nodesToVisit:
        nodesVisitedRoot += 1
        t1, lastLK, failedPasses = nodesToVisit.pop()
        childs = [children[t1][0], children[t1][1]]
        for i in range(2):
            try:
                score = table[childs[i]]
                if score != score:
                    raise ValueError("no result")
                failedPassesNew = failedPasses
                if score > bestLKdiff:
                    bestLKdiff = score
                    bestNode = childs[i]
                    failedPassesNew = 0
                elif score < (lastLK - thresholdLogLKconsecutivePlacement):
                    failedPassesNew += 1
                if score >= (bestLKdiff - thresholdLogLKoptimizationTopology):
                    bestNodes[childs[i]] = score
                traverseChildren = False
                if children[childs[i]]:
                    if strictTopologyStopRules:
                        if failedPassesNew <= allowedFailsTopology and score > (bestLKdiff - thresholdLogLKtopology):
                            traverseChildren = True
                    else:
                        if failedPassesNew <= allowedFailsTopology or score > (bestLKdiff - thresholdLogLKtopology):
                            traverseChildren = True
            except ValueError:
                traverseChildren = False
            if traverseChildren:
                nodesToVisit.append((childs[i], score, failedPassesNew))
    return bestNode, bestLKdiff, nodesVisitedRoot, list(bestNodes), list(bestNodes.values())


def random_tree(rng, tips, shape):
    """node 0 is the root; shape 'random': a random leaf is split each time; 'cat0' / 'cat1': a caterpillar through that side"""
    c0, c1 = [-1], [-1]
    leaves = [0]
    for _ in range(tips - 1):
        v = leaves.pop(rng.randrange(len(leaves)) if shape == "random" else -1)
        a, b = len(c0), len(c0) + 1
        c0 += [-1, -1]
        c1 += [-1, -1]
        c0[v], c1[v] = a, b
        leaves += [b, a] if shape == "cat0" else [a, b]
    return len(c0), 0, c0, c1


def check(program, cases):
    got = run_replay(program, cases)
    for (tree, strict, fails, a, b, cc, score), g in zip(cases, got):
        n, root, c0, c1 = tree
        _, children = as_reference(n, root, c0, c1)
        want = reference_replay(root, children, score, strict, fails, a, b, cc)
        assert g[0] == want[0] and g[2] == want[2] and g[3] == want[3], (tree, strict, fails, a, b, cc, score)
        assert [x.hex() for x in [g[1]] + g[4]] == [x.hex() for x in [want[1]] + want[4]]     # the same bits
    return got


def test_replay_on_random_trees_and_scores(program):
    rng = random.Random(20)
    cases = []
    for trial in range(240):
        tree = random_tree(rng, rng.randrange(2, 60), ("random", "random", "cat0", "cat1")[trial % 4])
        n = tree[0]
        kind = trial % 3
        score = [rng.choice([-3.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0]) if kind == 0 else rng.gauss(-1.0, 2.0) for _ in range(n)]
        if kind == 2:                                                      # merges without result, on one side or on both
            for v in range(n):
                if rng.random() < 0.15:
                    score[v] = NAN
        thr_top, thr_opt, thr_cons = rng.choice([0.5, 1.0, 2.0, 40.0]), rng.choice([0.0, 1.0, 1.5, INF]), rng.choice([0.0, 0.5, 1.0])
        for strict in (False, True):
            for fails in (0, 2, 1 << 30):
                cases.append((tree, strict, fails, thr_top, thr_opt, thr_cons, score))
    got = check(program, cases)
    assert any(len(g[3]) > 10 for g in got) and any(g[0] != 0 for g in got) and any(g[2] > 20 for g in got)
    shallow = [g[2] for (t, strict, fails, *_), g in zip(cases, got) if fails == 0 and strict]
    deep = [g[2] for (t, strict, fails, *_), g in zip(cases, got) if fails == 1 << 30 and not strict]
    assert sum(shallow) < sum(deep)                                        # the stop rules do stop


def test_replay_at_the_edges_of_its_comparisons(program):
    # 0 -> (1, 2); 1 -> (3, 4); 3 -> (7, 8); 4 -> (9, 10); 2 -> (5, 6); 5 -> (11, 12); everything else a leaf
    c0 = [1, 3, 5, 7, 9, 11] + [-1] * 7
    c1 = [2, 4, 6, 8, 10, 12] + [-1] * 7
    tree = (13, 0, c0, c1)
    base = [NAN, NAN, NAN, 2.0, 2.0, -1.0, 1.0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5]
    cases = []
    for strict in (False, True):
        for fails in (0, 2, 1 << 30):
            cases.append((tree, strict, fails, 1.0, 1.0, 0.5, base))       # 4 ties with 3 at 2.0: must not replace it
            s = list(base); s[5] = 1.0; s[6] = 2.0 - 1.0                   # equal to best - thresholdLogLKoptimizationTopology: kept
            cases.append((tree, strict, fails, 1.0, 1.0, 0.5, s))
            s = list(base); s[4] = 2.0 - 1.0                               # equal to best - thresholdLogLKtopology: not "within"
            cases.append((tree, strict, fails, 1.0, 3.0, 0.5, s))
            s = list(base); s[3] = NAN                                     # one side without result
            cases.append((tree, strict, fails, 1.0, 1.0, 0.5, s))
            s = list(base); s[3] = s[4] = NAN                              # both sides
            cases.append((tree, strict, fails, 1.0, 1.0, 0.5, s))
            cases.append((tree, strict, fails, 1.0, INF, 0.5, base))       # every scored branch that is reached is kept
            cases.append((tree, strict, fails, INF, INF, 0.0, base))
    got = check(program, cases)
    tie, kept, edge, one, both, everything, _ = got[:7]                    # non-strict, allowedFails 0
    assert tie[0] == 3 and tie[1] == 2.0 and 4 in tie[3]
    assert 6 in kept[3] and kept[4][kept[3].index(6)] == 1.0
    # side 1 of node 1 sits exactly at best - threshold: under strict rules nothing below node 4 is visited
    strict_edge = got[7 * 3 + 2]
    assert 4 in strict_edge[3] and 9 not in strict_edge[3] and 10 not in strict_edge[3]
    assert one[0] == 4 and 3 not in one[3] and 7 not in one[3]
    assert both[0] in (6, 0) and not {3, 4, 7, 8, 9, 10} & set(both[3])
    assert everything[3][0] == 0 and everything[4][0] == 0.0 and len(everything[3]) == everything[2] * 2 - 1
    assert math.isinf(cases[5][4])


def test_replay_of_special_roots(program):
    single = (1, 0, [-1], [-1])
    three = (3, 0, [1, -1, -1], [2, -1, -1])
    got = check(program, [(single, False, 0, 1.0, 1.0, 1.0, [NAN]), (three, True, 5, 1.0, INF, 1.0, [NAN] * 3)])
    assert got == [(0, 0.0, 1, [0], [0.0])] * 2
