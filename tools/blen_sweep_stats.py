#!/usr/bin/env python3
"""Time the branch-length sweep inside the library (maple_tree_optimize_blens) next to the Python sweep
(maple_amd.tree_host.optimize_branch_lengths) on a bench tree, converged and with every length perturbed: the first sweep
(every node dirty) and the sweeps to convergence, each from the same lists.

    python tools/blen_sweep_stats.py --samples 10000                      # a perturbed tree costs one repair per branch: 4-6 s
    python tools/blen_sweep_stats.py --samples 10000 --chunks 0 256 --port-limit 120

Prints one JSON line: wall time, estimate launches, estimates computed / used (what the chunk policy wastes) and repairs per
run.  The Python sweep runs under --port-limit seconds (SIGALRM); past it the line says "did not finish in N s"."""
import argparse
import copy
import json
import os
import random
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def clone(t):
    c = copy.copy(t)
    c.dist = t.dist.copy()
    for k in ("id_lower", "id_upRight", "id_upLeft", "id_totUp"):
        setattr(c, k, getattr(t, k).copy())
    return c


class Limit(Exception):
    pass


def with_limit(seconds, fn):
    def on_alarm(signum, frame):
        raise Limit()
    old = signal.signal(signal.SIGALRM, on_alarm)
    signal.alarm(int(seconds))
    t = time.perf_counter()
    try:
        return fn(), time.perf_counter() - t
    except Limit:
        return None, time.perf_counter() - t
    finally:
        signal.alarm(0)
        signal.signal(signal.SIGALRM, old)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=10000)
    ap.add_argument("--model", choices=["unrest", "ratevar", "siteerr"], default="unrest")
    ap.add_argument("--refs", choices=["auto", "local", "none"], default="auto")
    ap.add_argument("--chunks", type=int, nargs="+", default=[0, 256])
    ap.add_argument("--max-sweeps", type=int, default=20)
    ap.add_argument("--port-limit", type=float, default=180.0)
    ap.add_argument("--no-port", action="store_true")
    args = ap.parse_args()
    import bench
    from maple_amd.tree_host import HostTree, optimize_branch_lengths, optimize_branch_lengths_native, rebuild_genome_lists
    bt = bench.build_bench_tree(args.samples, args.model, tree="optimised", refs=args.refs)
    dev = bt.dev
    base = bt.ht if bt.ht is not None else HostTree.from_mirror(bt.mirror)
    eff = 1.0 / (10 * dev.lRef)
    out = dict(samples=args.samples, nodes=int(base.n), model=args.model, refs=bt.refs, reference_nodes=int(bt.n_ref), runs=[])

    def native(tree, chunk, sweeps):
        s0 = dev.optimize_blens_stats()
        dirty, ups = None, []
        t = time.perf_counter()
        for _ in range(sweeps):
            u, dirty, _ = optimize_branch_lengths_native(dev, tree, eff, dirty=dirty, chunk=chunk)
            ups.append(u)
            if u == 0:
                break
        s = time.perf_counter() - t
        s1 = dev.optimize_blens_stats()
        d = {k: s1[k] - s0[k] for k in s1}
        d.update(seconds=round(s, 3), updates=ups, computed_per_used=round(d["computed"] / max(d["used"], 1), 3))
        return d

    def port(tree, sweeps):
        dirty, ups = None, []
        for _ in range(sweeps):
            u, dirty, _ = optimize_branch_lengths(dev, tree, eff, dirty=dirty)
            ups.append(u)
            if u == 0:
                break
        return ups

    for state in ("converged", "perturbed"):
        start = clone(base)
        if state == "perturbed":
            rng = random.Random(11)
            for v in start.preorder():
                if v != start.root and start.dist[v]:
                    start.dist[v] = start.dist[v] * (0.4 + 2.1 * rng.random())
            start.id_lower, start.id_upRight, start.id_upLeft, start.id_totUp = rebuild_genome_lists(dev, start)
        for what, sweeps in (("first sweep", 1), ("to convergence", args.max_sweeps)):
            for chunk in args.chunks:
                mark = dev.mark()
                r = native(clone(start), chunk, sweeps)
                dev.release(mark)
                r.update(state=state, what=what, form=f"native chunk={chunk or 'adaptive'}")
                out["runs"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
            if not args.no_port:
                mark = dev.mark()
                ups, s = with_limit(args.port_limit, lambda: port(clone(start), sweeps))
                dev.release(mark)
                r = dict(state=state, what=what, form="python optimize_branch_lengths (batch=256)",
                         seconds=round(s, 3) if ups is not None else f"did not finish in {int(args.port_limit)} s", updates=ups)
                out["runs"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
