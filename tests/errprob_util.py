"""Helpers of the error-report tests (a module like em_util.py): the committed fixtures tests/golden/errprob_<name>.json.gz made
by tests/golden/make_golden_errprob.py -- the reference's calculateErrorProbabilities (M:9783-10020) on the tree of the em_ fixture
each one names."""
import gzip
import json
import os

import numpy as np

import em_util

GOLDEN = em_util.GOLDEN
THRESHOLDS = (0.0, 0.01, 0.5)
MARGIN = 1e-9                            # no recorded probability lies this close (relative) to a non-zero threshold


def fixture_names():
    return sorted(f[len("errprob_"):-len(".json.gz")] for f in os.listdir(GOLDEN)
                  if f.startswith("errprob_") and f.endswith(".json.gz") and f != "errprob_zero_div.json.gz")


_cache = {}


def load(name):
    if name not in _cache:
        with gzip.open(os.path.join(GOLDEN, f"errprob_{name}.json.gz"), "rt") as fh:
            _cache[name] = json.load(fh)
    return _cache[name]


def arms():
    return json.load(open(os.path.join(GOLDEN, "errprob_arms.json")))


def em_of(fx):
    """The em_ fixture whose tree, model and context the error-report fixture belongs to."""
    return em_util.load(fx["em"])


def arrays(rec):
    """One threshold's record as the arrays of Device.error_probabilities: (leaf_nodes, off, pos, allele, prob)."""
    off = np.zeros(len(rec["leaves"]) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rec["records"]])
    flat = [x for r in rec["records"] for x in r]
    return (np.asarray(rec["leaves"], np.int32), off, np.asarray([x[0] for x in flat], np.int32),
            np.asarray([x[1] for x in flat], np.uint8), np.asarray([x[2] for x in flat], np.float64))


def dfs_leaves(tree):
    """The leaves in the order the reference's traversal meets them: depth first, children[v][0] before children[v][1]."""
    out, st = [], [tree["root"]]
    while st:
        v = st.pop()
        ch = tree["children"][v]
        if ch:
            st.extend(reversed(ch))
        else:
            out.append(v)
    return out
