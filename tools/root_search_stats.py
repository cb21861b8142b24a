#!/usr/bin/env python3
"""Time the search for the best root inside the library (maple_tree_find_best_root, tree_host.find_best_root_native) on a bench
tree, next to the Python path it stands beside (tree_host.find_best_root: per level five maple_merge_batch(returnLK) launches,
each committing its merged lists, the passes through reference branches, maple_root_prob_batch and numpy glue).

    python tools/root_search_stats.py --samples 100000 --model ratevar            # the headline tree (optimised, MAT local references)
    python tools/root_search_stats.py --samples 1000000 --model siteerr --tree truth --refs none

Prints one JSON line and writes it to --out (default profiles/root_search_stats_<samples>_<model>.json).  Wall-clock around the
synchronous calls; two warm-up calls, then --repeats timed ones (median, min, max) of either path.  `first_call_ms` is the native
call that also groups the tree into levels (once per uploaded tree)."""
import argparse
import json
import math
import os
import struct
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    ms, outs = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        outs.append(fn())
        ms.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3)), outs


def bits(x):
    return struct.pack("<d", x).hex()


def result_bits(r):
    """find_best_root's 4-tuple as something == compares bit for bit, the dict in its order"""
    return r[0], bits(r[1]), r[3], [(int(k), bits(v)) for k, v in r[2].items()]


def levels(tree):
    """(levels, items, items below or at a node with a mutation list) of the level loop"""
    n_levels = n_items = n_mat = 0
    root_mat = bool(tree.id_mut[tree.root] >= 0)
    cur = [(c, root_mat) for c in tree.children[tree.root]]
    while cur:
        nxt, here = [], 0
        for v, m in cur:
            if tree.children[v]:
                m = m or bool(tree.id_mut[v] >= 0)
                here += 1
                n_mat += m
                nxt += [(c, m) for c in tree.children[v]]
        n_levels += here > 0
        n_items += here
        cur = nxt
    return n_levels, n_items, n_mat


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--model", choices=["unrest", "ratevar", "siteerr"], default="ratevar")
    ap.add_argument("--tree", choices=["optimised", "truth"], default="optimised")
    ap.add_argument("--refs", choices=["auto", "local", "none"], default="auto")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--python-repeats", type=int, default=5, help="timed calls of the Python path")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from maple_amd.tree_host import HostTree, find_best_root, find_best_root_native
    bt = bench.build_bench_tree(args.samples, args.model, tree=args.tree, refs=args.refs)
    dev = bt.dev
    tree = bt.ht if bt.ht is not None else HostTree.from_mirror(bt.mirror)
    bt.upload_headline_tree()                                              # (a fresh upload: the first call below groups the tree)
    ll = math.log(dev.lRef)
    kw = dict(strictTopologyStopRules=False, allowedFailsTopology=4, thresholdLogLKtopology=14.0 * ll,
              thresholdLogLKoptimizationTopology=ll, thresholdLogLKconsecutivePlacement=1.0)
    before = dev.stats()
    t = time.perf_counter()
    first = find_best_root_native(dev, tree, **kw)
    first_ms = 1e3 * (time.perf_counter() - t)
    native, outs = timed(lambda: find_best_root_native(dev, tree, **kw), 2, args.repeats)
    arena_neutral = dev.stats() == before
    python, pouts = timed(lambda: find_best_root(dev, tree, **kw), 2, args.python_repeats)
    want = result_bits(first)
    same = all(result_bits(o) == want for o in outs + pouts)
    score = dev.tree_find_best_root(tree.n_minor if any(tree.n_minor) else None, **kw)[3]
    n_levels, n_items, n_mat = levels(tree)
    line = dict(samples=args.samples, nodes=int(tree.n), model=args.model, tree=args.tree, refs=bt.refs, reference_nodes=int(bt.n_ref),
                levels=n_levels, items=n_items, items_materialised=int(n_mat), branches_scored=int((~np.isnan(score)).sum()),
                native=native, first_call_ms=round(first_ms, 3), python_path=python,
                speedup=round(python["median_ms"] / native["median_ms"], 2), best_node=int(first[0]), best_lk_diff=first[1],
                nodes_visited=int(first[3]), best_nodes=len(first[2]), bits_equal=bool(same), arena_neutral=bool(arena_neutral),
                params=kw, calls=args.repeats, python_calls=args.python_repeats)
    text = json.dumps(line)
    out = args.out or os.path.join(ROOT, "profiles", f"root_search_stats_{args.samples}_{args.model}.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
