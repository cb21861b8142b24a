#!/usr/bin/env python3
"""Golden vectors for SUCCESSIVE calls of traverseTreeToOptimizeBranchLengths (M:8727-8893, default fastPass=False) --
BUILD CONTAINER ONLY.

update_<name>.json.gz (make_golden_update.py, ``blen_full_sweeps``) records the first sweep only: every node dirty.  The
reference's closing loop (M:11899-11906) calls the sweep up to 20 times, and every call after the first starts from the
``dirty`` flags the previous one left: the ones its own 1 % rule cleared, set again wherever an ``updatePartials`` popped
the node (M:5499-5500, 5410-5411).  This script records that sequence.

Re-runs the unmodified reference exactly like make_golden_search.py (same flags, hence the same final tree: the snapshot
in search_<name>.json.gz is the BASE and is not stored again), perturbs every non-root branch length exactly as
``blen_full_sweeps[1]`` does (random.Random(11), factor 0.4 + 2.1 u), recomputes the genome lists, sets every node dirty and
calls ``traverseTreeToOptimizeBranchLengths(tree, t1)`` until it returns 0 (at most 21 times).

Per sweep the file keeps: the dirty flags going in, the return value, the first node of every ``updatePartials`` call in
order (sys.setprofile, as make_golden_update.py), the branch lengths that changed (node -> new length), the dirty flags
coming out and calculateTreeLikelihood afterwards.  Data only: tests/golden/blen_rounds_<name>.json.gz.
"""
import contextlib
import copy
import gzip
import io
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_search import RUNS, frozen_reference_tree  # noqa: E402

MAX_SWEEPS = 21


def run(name):
    g, tree, t1, _, _ = frozen_reference_tree(name, RUNS[name])
    reach = []
    st = [t1]
    while st:
        v = st.pop()
        reach.append(v)
        st.extend(tree.children[v])
    tc = copy.deepcopy(tree)
    rng = random.Random(11)
    sweeps = []
    with contextlib.redirect_stdout(io.StringIO()):
        for v in reach:
            if v != t1 and tc.dist[v]:
                tc.dist[v] = tc.dist[v] * (0.4 + 2.1 * rng.random())
        g["setAllDirty"](tc, t1)
        g["reCalculateAllGenomeLists"](tc, t1)
        g["setAllDirty"](tc, t1)
        lk_in = g["calculateTreeLikelihood"](tc, t1)
        dist_in = [float(x or 0.0) for x in tc.dist]
        for _ in range(MAX_SWEEPS):
            dirty_in = [bool(x) for x in tc.dirty]
            before = [float(x or 0.0) for x in tc.dist]
            order = []

            def prof(frame, event, arg):
                if event == "call" and frame.f_code.co_name == "updatePartials":
                    order.append(frame.f_locals["nodeList"][0][0])
            sys.setprofile(prof)
            try:
                updates = g["traverseTreeToOptimizeBranchLengths"](tc, t1)
            finally:
                sys.setprofile(None)
            lk = g["calculateTreeLikelihood"](tc, t1)
            after = [float(x or 0.0) for x in tc.dist]
            sweeps.append(dict(dirty_in=[i for i, x in enumerate(dirty_in) if x], updates=updates, update_order=order,
                               dist_changed={str(i): after[i] for i in range(len(after)) if after[i] != before[i]},
                               dirty_out=[i for i, x in enumerate(tc.dirty) if x], treeLK=lk))
            print(f"[{name}] sweep {len(sweeps)}: dirty in {len(sweeps[-1]['dirty_in'])}, {updates} updates, "
                  f"dirty out {len(sweeps[-1]['dirty_out'])}, LK {lk:.6f}", file=sys.stderr, flush=True)
            if updates == 0:
                break
    path = os.path.join(HERE, f"blen_rounds_{name}.json.gz")
    with gzip.open(path, "wt") as fh:
        json.dump(dict(name=name, base=f"search_{name}.json.gz", n=len(dist_in), root=t1, dist_in=dist_in, treeLK_in=lk_in,
                       sweeps=sweeps, effectivelyNon0BLen=g["effectivelyNon0BLen"]), fh)
    print(f"[{name}] -> {path} {os.path.getsize(path)/1e6:.3f} MB", flush=True)


if __name__ == "__main__":
    for nm in (sys.argv[1:] or list(RUNS)):
        run(nm)
