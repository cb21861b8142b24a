#!/usr/bin/env python3
"""Time the mutation events inside the library (maple_tree_mutation_events, Device.mutation_events) on a bench tree.

    python tools/mutation_events_stats.py                                        # 100 000 tips, the full model, MAT references
    python tools/mutation_events_stats.py --samples 1000000 --tree truth --refs none

Prints one JSON line: nodes, records per stream, ms per call and its split.  Wall-clock around the synchronous calls, two warm-up
calls of each kind, then --repeats timed pairs of (sizing call, full call), the two taking turns (median, min, max).  `count_only`
is the sizing call (item collection, the pass-down launch for nodes under reference branches, the counting launch, the counts' copy
and their three scans), `full` the call that also writes and copies the records.  `pass_ms` / `count_kernel_ms` / `fill_kernel_ms`
are the HIP-event times inside the full calls (maple_timing_*): the pass-down with its commit, and the two launches of k_mat_walk;
`host_and_copies_ms` is the rest of the full call.  `em_walk_kernel_ms` is k_em_walk's launch inside maple_em_expectation on the
same tree, by the same events: the walk the counting launch shares its pairs with."""
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
    ap.add_argument("--model", choices=["siteerr"], default="siteerr", help="the full model: all three streams have records")
    ap.add_argument("--tree", choices=["optimised", "truth"], default="optimised")
    ap.add_argument("--refs", choices=["auto", "local", "none"], default="auto")
    ap.add_argument("--min-mut-prob", type=float, default=0.01)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    import bench
    from maple_amd.tree_host import HostTree
    bt = bench.build_bench_tree(args.samples, args.model, tree=args.tree, refs=args.refs)
    dev = bt.dev
    tree = bt.ht if bt.ht is not None else HostTree.from_mirror(bt.mirror)
    bt.upload_headline_tree()
    nm = np.asarray(tree.n_minor, dtype=np.int32) if any(tree.n_minor) else None   # (once: the calls below take it as it is)
    thr = args.min_mut_prob
    rc, _, _, _, _, _, _, n_rec = dev.tree_mutation_events(nm, thr, 0, 0, 0)
    dev._ck(rc)
    caps = [int(x) for x in n_rec]

    def count_only():
        dev._ck(dev.tree_mutation_events(nm, thr, 0, 0, 0)[0])

    def full():
        out = dev.tree_mutation_events(nm, thr, *caps)
        dev._ck(out[0])
        return out[1:7]

    first = full()
    for _ in range(2):
        count_only()
        full()
    t_count, t_full, events, em_ms, same = [], [], [], [], True
    for _ in range(args.repeats):
        t = time.perf_counter()
        count_only()
        t_count.append(1e3 * (time.perf_counter() - t))
        dev.timing_reset()
        t = time.perf_counter()
        out = full()
        t_full.append(1e3 * (time.perf_counter() - t))
        events.append(dev.timing_read_each(cap=16))                       # [pass-down (if any node needs it)], count, fill
        same = same and all(a.tobytes() == b.tobytes() for a, b in zip(out, first) if a is not None)
        dev.timing_reset()
        dev.em_expectation(nm)
        em_ms.append(float(dev.timing_read_each(cap=16)[-1]))             # k_em_walk is the call's last timed launch
    ev = np.asarray(events)
    assert ev.ndim == 2 and ev.shape[1] in (2, 3), ev.shape
    med = np.median(ev, axis=0)
    pass_ms = float(med[0]) if ev.shape[1] == 3 else 0.0
    count_ms, fill_ms = float(med[-2]), float(med[-1])
    whole, count = summary(t_full), summary(t_count)
    print(json.dumps(dict(samples=args.samples, nodes=int(bt.mirror.n_nodes), model=args.model, tree=args.tree, refs=bt.refs,
                          reference_nodes=int(bt.n_ref), min_mut_prob=thr, mutation_records=caps[0], ns_records=caps[1],
                          error_records=caps[2], nodes_with_mutations=int(np.count_nonzero(np.diff(first[0]) > 0)), full=whole,
                          count_only=count, pass_ms=round(pass_ms, 3), count_kernel_ms=round(count_ms, 3),
                          fill_kernel_ms=round(fill_ms, 3),
                          host_and_copies_ms=round(whole["median_ms"] - pass_ms - count_ms - fill_ms, 3),
                          em_walk_kernel_ms=round(float(np.median(em_ms)), 3), bytes_equal=bool(same), calls=args.repeats)))


if __name__ == "__main__":
    main()
