#!/usr/bin/env python3
"""Time the tree log-likelihood inside the library (maple_tree_log_lk, tree_host.tree_log_likelihood_native) on a bench tree,
next to the Python path it stands beside (tree_host.tree_log_likelihood: a stack walk over every node, gathered columns,
maple_merge_batch(returnLK) committing a merged list per internal node).

    python tools/tree_lk_stats.py --samples 100000 --model ratevar            # the headline tree (optimised, MAT local references)
    python tools/tree_lk_stats.py --samples 1000000 --model siteerr --tree truth --refs none

Prints one JSON line.  Wall-clock around the synchronous calls; two warm-up calls, then --repeats timed ones (median, min, max).
`first_call_ms` is the native call that also lists the tree's post-order and uploads the items (once per uploaded tree);
`kernel_ms` the HIP-event time of k_tree_lk alone in the timed calls (maple_timing_*)."""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--model", choices=["unrest", "ratevar", "siteerr"], default="ratevar")
    ap.add_argument("--tree", choices=["optimised", "truth"], default="optimised")
    ap.add_argument("--refs", choices=["auto", "local", "none"], default="auto")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--python-repeats", type=int, default=5, help="timed calls of the Python path (seconds each at 1 000 000 tips)")
    args = ap.parse_args()
    import bench
    from maple_amd.tree_host import HostTree, tree_log_likelihood, tree_log_likelihood_native
    bt = bench.build_bench_tree(args.samples, args.model, tree=args.tree, refs=args.refs)
    dev = bt.dev
    tree = bt.ht if bt.ht is not None else HostTree.from_mirror(bt.mirror)
    bt.upload_headline_tree()                                              # (a fresh upload: the first call below lists the tree)
    t = time.perf_counter()
    first = tree_log_likelihood_native(dev, tree)
    first_ms = 1e3 * (time.perf_counter() - t)
    for _ in range(2):
        tree_log_likelihood_native(dev, tree)
    dev.timing_reset()
    native, outs = timed(lambda: tree_log_likelihood_native(dev, tree), 0, args.repeats)
    n_timed, kernel_ms = dev.timing_read()
    python, pouts = timed(lambda: tree_log_likelihood(dev, tree), 2 if args.python_repeats > 1 else 0, args.python_repeats)
    same = all(bits(o[0]) == bits(first[0]) and bits(o[1]) == bits(first[1]) for o in outs + pouts)
    n_internal = int((np.asarray(bt.mirror.children[:, 0]) >= 0).sum())
    print(json.dumps(dict(samples=args.samples, nodes=int(bt.mirror.n_nodes), internal_nodes=n_internal, model=args.model, tree=args.tree,
                          refs=bt.refs, reference_nodes=int(bt.n_ref), native=native, first_call_ms=round(first_ms, 3),
                          kernel_ms=round(kernel_ms / max(n_timed, 1), 3), kernel_launches_timed=n_timed, python_path=python,
                          speedup=round(python["median_ms"] / native["median_ms"], 2), total_lk=first[0], root_lk=first[1],
                          total_lk_bits=bits(first[0]), bits_equal=bool(same), calls=args.repeats, python_calls=args.python_repeats)))


if __name__ == "__main__":
    main()
