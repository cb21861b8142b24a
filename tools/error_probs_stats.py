#!/usr/bin/env python3
"""Time the per-sample error report inside the library (maple_tree_error_probs, Device.error_probabilities) on a bench tree.

    python tools/error_probs_stats.py                                        # 100 000 tips, the full model (rate variation, site error rates)
    python tools/error_probs_stats.py --samples 1000000 --tree truth --refs none

Prints one JSON line: leaves, records, ms per call and its split.  Wall-clock around the synchronous calls, two warm-up calls of
each kind, then --repeats timed pairs of (sizing call, full call), the two taking turns (median, min, max).  `count_only` is the
sizing call (leaf collection, the pass-down launch for leaves under reference branches, the counting launch, the counts' copy and
their scan), `full` the call that also writes and copies the records.  `pass_ms` / `count_kernel_ms` / `fill_kernel_ms` are the
HIP-event times inside the full calls (maple_timing_*): the pass-down with its commit, and the two launches of k_err_walk;
`host_and_copies_ms` is the rest of the full call."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    return dict(median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--model", choices=["siteerr"], default="siteerr", help="the report needs an error model: the full model")
    ap.add_argument("--tree", choices=["optimised", "truth"], default="optimised")
    ap.add_argument("--refs", choices=["auto", "local", "none"], default="auto")
    ap.add_argument("--min-error-prob", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import bench
    from maple_amd.tree_host import HostTree
    bt = bench.build_bench_tree(args.samples, args.model, tree=args.tree, refs=args.refs)
    dev = bt.dev
    tree = bt.ht if bt.ht is not None else HostTree.from_mirror(bt.mirror)
    bt.upload_headline_tree()
    nm = np.asarray(tree.n_minor, dtype=np.int32) if any(tree.n_minor) else None   # (once: the calls below take it as it is)
    thr = args.min_error_prob
    rc, _, _, n_leaves, _, _, _, n_rec = dev.tree_error_probs(nm, thr, dev.n_nodes, 0)
    dev._ck(rc)

    def count_only():
        rc, _, _, _, _, _, _, _ = dev.tree_error_probs(nm, thr, n_leaves, 0)
        dev._ck(rc)

    def full():
        rc, leaf, off, _, pos, al, pr, _ = dev.tree_error_probs(nm, thr, n_leaves, n_rec)
        dev._ck(rc)
        return leaf, off, pos, al, pr

    first = full()
    for _ in range(2):
        count_only()
        full()
    t_count, t_full, events, same = [], [], [], True
    for _ in range(args.repeats):
        t = time.perf_counter()
        count_only()
        t_count.append(1e3 * (time.perf_counter() - t))
        dev.timing_reset()
        t = time.perf_counter()
        out = full()
        t_full.append(1e3 * (time.perf_counter() - t))
        events.append(dev.timing_read_each(cap=16))                       # [pass-down (if any leaf needs it)], count, fill
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip(out, first) if a is not None)
    ev = np.asarray(events)
    assert ev.ndim == 2 and ev.shape[1] in (2, 3), ev.shape
    med = np.median(ev, axis=0)
    pass_ms = float(med[0]) if ev.shape[1] == 3 else 0.0
    count_ms, fill_ms = float(med[-2]), float(med[-1])
    whole, count = summary(t_full), summary(t_count)
    print(json.dumps(dict(samples=args.samples, nodes=int(bt.mirror.n_nodes), model=args.model, tree=args.tree, refs=bt.refs,
                          reference_nodes=int(bt.n_ref), min_error_prob=thr, leaves=int(n_leaves),
                          leaves_with_records=int(np.count_nonzero(np.diff(first[1]) > 0)), records=int(n_rec), full=whole,
                          count_only=count, pass_ms=round(pass_ms, 3), count_kernel_ms=round(count_ms, 3),
                          fill_kernel_ms=round(fill_ms, 3),
                          host_and_copies_ms=round(whole["median_ms"] - pass_ms - count_ms - fill_ms, 3),
                          bytes_equal=bool(same), calls=args.repeats)))


if __name__ == "__main__":
    main()
