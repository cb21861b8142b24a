"""The order in which maple_tree_log_lk adds the nodes' contributions (maple_amd/csrc/tree_lk_plan.h) on the CPU:
tests/tree_lk_plan_main.cpp, compiled on its own with the host sanitizers.  lk_postorder must give the order of the reference's own
loop (calculateTreeLikelihood, M:9735-9770: direction 0 down through children[0], direction 1 up) written out in Python below."""
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


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/tree_lk_plan_main.cpp"
    exe = str(tmp_path_factory.mktemp("tree_lk_plan") / "tree_lk_plan_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(HERE, "tree_lk_plan_main.cpp")])
    return exe


def run(program, trees):
    lines = ["P %d %d %s %s" % (n, root, " ".join(map(str, c0)), " ".join(map(str, c1))) for n, root, c0, c1 in trees]
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        assert w[0] == "P"
        out.append([int(x) for x in w[2:]] if w[1] == "1" else None)
    assert len(out) == len(trees)
    return out


def reference_order(root, up, children):
    """M:9729-9770 with the reference's own variables; the nodes at which it calls mergeVectors, in that order"""
    order = []
    node, lastNode, direction = root, None, 0
    while node is not None:
        if direction == 0:
            if children[node]:
                node = children[node][0]
            else:
                lastNode = node
                node = up[node]
                direction = 1
        else:
            if lastNode == children[node][0]:
                node = children[node][1]
                direction = 0
            else:
                order.append(node)
                lastNode = node
                node = up[node]
                direction = 1
    return order


def as_reference(n, root, c0, c1):
    """(up, children) in the reference's form from the columns; up only below the root"""
    up = [None] * n
    children = [[] if c0[v] < 0 else [c0[v], c1[v]] for v in range(n)]
    stack = [root]
    while stack:
        v = stack.pop()
        for ch in children[v]:
            up[ch] = v
            stack.append(ch)
    return up, children


def fixture_tree(name):
    with gzip.open(os.path.join(GOLDEN, f"search_{name}.json.gz"), "rt") as fh:
        t = json.load(fh)["tree"]
    n = len(t["up"])
    return n, t["root"], [c[0] if c else -1 for c in t["children"]], [c[1] if c else -1 for c in t["children"]]


def caterpillar(tips, left):
    """internal node i is node 2i, its tip 2i+1, the last tip 2(tips-1); left: the chain runs through children[0]"""
    m = tips - 1
    n = 2 * m + 1
    c0, c1 = [-1] * n, [-1] * n
    for i in range(m):
        c0[2 * i], c1[2 * i] = (2 * i + 2, 2 * i + 1) if left else (2 * i + 1, 2 * i + 2)
    return n, 0, c0, c1


def small_trees():
    out = {nm: fixture_tree(nm) for nm in TREES}
    out["single"] = (1, 0, [-1], [-1])
    out["three"] = (3, 0, [1, -1, -1], [2, -1, -1])
    out["root_not_0"] = (3, 2, [-1, -1, 0], [-1, -1, 1])
    out["seven"] = (7, 0, [1, 3, 5, -1, -1, -1, -1], [2, 4, 6, -1, -1, -1, -1])
    out["cat_left_40"] = caterpillar(40, True)
    out["cat_right_40"] = caterpillar(40, False)
    # slots the root does not reach: a detached cherry (7, 8, 9), a lone slot (10) and a slot that names nodes of the tree as
    # its children (11) after the balanced seven
    out["unreachable"] = (12, 0, [1, 3, 5, -1, -1, -1, -1, 8, -1, -1, -1, 3], [2, 4, 6, -1, -1, -1, -1, 9, -1, -1, -1, 4])
    return out


def test_there_are_eight_fixture_topologies():
    assert len(TREES) == 8


def test_postorder_is_the_reference_loop(program):
    trees = small_trees()
    names = sorted(trees)
    got = run(program, [trees[nm] for nm in names])
    for nm, order in zip(names, got):
        n, root, c0, c1 = trees[nm]
        up, children = as_reference(n, root, c0, c1)
        want = reference_order(root, up, children)
        assert order == want, nm
    by = dict(zip(names, got))
    assert by["single"] == [] and by["three"] == [0] and by["root_not_0"] == [2]
    assert by["seven"] == [1, 2, 0]                                        # children[0] subtree, children[1] subtree, the node
    assert by["cat_left_40"] == by["cat_right_40"] == list(range(76, -1, -2))
    assert by["unreachable"] == [1, 2, 0]                                  # nothing of slots 7-11
    for nm in TREES:                                                       # every internal node the root reaches, once
        n, root, c0, c1 = trees[nm]
        up, _ = as_reference(n, root, c0, c1)
        assert sorted(by[nm]) == [v for v in range(n) if c0[v] >= 0 and (v == root or up[v] is not None)], nm
        assert len(by[nm]) > 10, nm


@pytest.mark.parametrize("left", [True, False])
def test_a_200000_tip_caterpillar_needs_no_recursion(program, left):
    tree = caterpillar(200000, left)
    n, root, c0, c1 = tree
    got = run(program, [tree])[0]
    up, children = as_reference(n, root, c0, c1)
    assert got == reference_order(root, up, children)
    assert len(got) == 199999 and got[0] == 2 * 199998 and got[-1] == 0


def test_columns_that_are_no_tree(program):
    bad = [(3, 0, [1, -1, -1], [-1, -1, -1]),                              # one child only
           (3, 0, [1, -1, -1], [5, -1, -1]),                               # a child out of range
           (3, 0, [1, -1, -1], [1, -1, -1]),                               # the same child twice
           (7, 0, [1, 3, 5, -1, -1, -1, -1], [2, 4, 3, -1, -1, -1, -1]),   # a node reached twice
           (3, 0, [1, 0, -1], [2, 2, -1]),                                 # a cycle through the root
           (3, 5, [1, -1, -1], [2, -1, -1])]                               # the root is no node
    assert run(program, bad) == [None] * len(bad)
