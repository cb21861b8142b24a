#!/usr/bin/env python3
"""Time one EM step (maple_em_rates) on a bench tree, next to maple_tree_rebuild_lists on the same tree (a comparable number
of list pairs walked), and measure the run-to-run spread of its per-site outputs (fp64 atomic adds: DESIGN.md section 13).

    python tools/em_stats.py --samples 100000 --model ratevar            # the headline tree (optimised, MAT local references)
    python tools/em_stats.py --samples 1000000 --model siteerr --tree truth --refs none

Prints one JSON line.  Wall-clock around the synchronous calls; two warm-up calls, then --repeats timed ones (median, min, max)."""
import argparse
import json
import os
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


def rel_spread(tables):
    """[largest |a - b| / max(|a|, |b|) over all sites, largest |a - b| / (largest magnitude of the table)] between any call and
    the first.  (The first counts a sum that cancels to nearly zero in full; the second does not.)"""
    worst, scaled = 0.0, 0.0
    for t in tables[1:]:
        a, b = np.asarray(tables[0]), np.asarray(t)
        den = np.maximum(np.abs(a), np.abs(b))
        worst = max(worst, float(np.max(np.where(den > 0, np.abs(a - b) / np.where(den > 0, den, 1.0), 0.0))))
        scaled = max(scaled, float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(a))), 1e-300)))
    return [worst, scaled]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=100000)
    ap.add_argument("--model", choices=["unrest", "ratevar", "siteerr"], default="ratevar")
    ap.add_argument("--tree", choices=["optimised", "truth"], default="optimised")
    ap.add_argument("--refs", choices=["auto", "local", "none"], default="auto")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import bench
    bt = bench.build_bench_tree(args.samples, args.model, tree=args.tree, refs=args.refs)
    dev, m, ht = bt.dev, bt.mirror, bt.ht
    n = m.n_nodes
    em, outs = timed(lambda: dev.em_rates(None, "UNREST"), 2, args.repeats)
    ex, raws = timed(lambda: dev.em_expectation(None), 1, args.repeats)
    spread = {}
    if outs[0][1] is not None:
        spread["siteRates"] = rel_spread([o[1] for o in outs])
    if outs[0][3] is not None:
        spread["siteErrRates"] = rel_spread([o[3] for o in outs])
    for k in ("waitingTimesSites", "countsSites", "trackingNs", "errorCountSites"):
        if np.any(raws[0][k]):
            spread[k] = rel_spread([r[k] for r in raws])
    totals_identical = all(np.array_equal(np.asarray(raws[0][k]), np.asarray(r[k])) for r in raws[1:]
                           for k in ("counts", "waitingTimes", "errorCount", "totTreeLength", "observedTotNucsSites", "numTips"))
    dist = np.ascontiguousarray(bt.ht_dist if ht is not None else m.dist, dtype=np.float64).copy()
    mut = ht.id_mut if ht is not None else None
    lower = (ht.id_lower if ht is not None else m.lower).copy()

    def rebuild():
        mark = dev.mark()
        try:
            return dev.tree_rebuild_lists(m.root, m.parent, m.children[:, 0], m.children[:, 1], m.is_tip, mut, dist, lower)[4]
        finally:
            dev.release(mark)
    rb, _ = timed(rebuild, 1, 3)
    print(json.dumps(dict(samples=args.samples, nodes=int(n), model=args.model, tree=args.tree, refs=bt.refs, reference_nodes=int(bt.n_ref),
                          em_rates=em, em_expectation=ex, tree_rebuild_lists=rb, per_site_relative_spread=spread,
                          totals_bit_identical=bool(totals_identical), calls=args.repeats)))


if __name__ == "__main__":
    main()
