"""Helpers of the mutation-event tests (a module like errprob_util.py): the committed fixtures tests/golden/mat_<name>.json.gz made
by tests/golden/make_golden_mat.py -- the reference's expectationMaximizationCalculationRates(tree, root, trackMutations=True)
(M:10077-10850) and stringForNode (M:2673-2809) on the tree of the em_ fixture each one names."""
import gzip
import json
import os

import numpy as np

import em_util

GOLDEN = em_util.GOLDEN
MARGIN = 1e-9                            # no recorded probability lies this close (relative) to a non-zero threshold
NEGQ = "cat_a_ratevar_negq"              # the reference raises on this one: nothing but that is recorded
ROOT_NS = "root_ns"                      # the hand-built trees: cases of their own, no em_ fixture


def fixture_names():
    """the fixtures with records: one per non-raising em_ fixture"""
    return sorted(f[len("mat_"):-len(".json.gz")] for f in os.listdir(GOLDEN)
                  if f.startswith("mat_") and f.endswith(".json.gz") and f[len("mat_"):-len(".json.gz")] not in (NEGQ, ROOT_NS))


_cache = {}


def load(name):
    if name not in _cache:
        with gzip.open(os.path.join(GOLDEN, f"mat_{name}.json.gz"), "rt") as fh:
            _cache[name] = json.load(fh)
    return _cache[name]


def arms():
    return json.load(open(os.path.join(GOLDEN, "mat_arms.json")))


def em_of(fx):
    """The em_ fixture whose tree, model and context the fixture belongs to."""
    return em_util.load(fx["em"])


def dtypes():
    from maple_amd.runtime import MUT_EVENT_DTYPE, N_RUN_DTYPE
    return MUT_EVENT_DTYPE, N_RUN_DTYPE


def arrays(rec, n, node_map=None):
    """One threshold's record as the arrays of Device.mutation_events: (mutOff, nsOff, errOff, mut, ns, err); node_map[v] = the id
    node v has in the tree the arrays describe."""
    ev_t, ns_t = dtypes()
    at = list(range(n)) if node_map is None else node_map
    old_of = [0] * n
    for v in range(n):
        old_of[at[v]] = v

    def events(col):
        off = np.zeros(n + 1, np.int64)
        flat = []
        for w in range(n):
            rl = col[old_of[w]] if col is not None else []
            flat.extend(rl)
            off[w + 1] = len(flat)
        a = np.zeros(len(flat), ev_t)
        a["pos"], a["from"], a["to"] = [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat]
        a["prob"] = [x[3] for x in flat]
        return off, a

    mo, mut = events(rec["mutationsInf"])
    eo, err = events(rec["errors"])
    no = np.zeros(n + 1, np.int64)
    flat = []
    for w in range(n):
        flat.extend([x, 0] if isinstance(x, int) else x for x in rec["Ns"][old_of[w]])
        no[w + 1] = len(flat)
    ns = np.zeros(len(flat), ns_t)
    ns["first"], ns["last"] = [x[0] for x in flat], [x[1] for x in flat]
    return mo, no, eo, mut, ns, err


def items(tree, using_error_rate):
    """(pair items, single-list items) of a tree snapshot, the reference's if / else at M:10146 / M:10808, over the nodes the root
    reaches"""
    pair, single, st = [], [], [tree["root"]]
    while st:
        v = st.pop()
        ch = tree["children"][v]
        if tree["up"][v] is not None and (tree["dist"][v] or (using_error_rate and not ch)):
            pair.append(v)
        else:
            single.append(v)
        st.extend(reversed(ch))
    return pair, single


def root_state_of(text):
    """the rootState={...} part of the root's text"""
    assert text.startswith("[&rootState={") and text.endswith("}]"), text[:60]
    return text[2:-1]
