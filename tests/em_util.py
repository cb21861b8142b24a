"""Helpers of the EM-step tests (a module like golden_util.py): the committed fixtures tests/golden/em_<name>.json.gz made by
tests/golden/make_golden_em.py, and the comparison rule of the GPU tests."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODEL_CODE = {"UNREST": 0, "GTR": 1}


def fixture_names():
    return sorted(f[len("em_"):-len(".json.gz")] for f in os.listdir(GOLDEN) if f.startswith("em_") and f.endswith(".json.gz"))


_cache = {}


def load(name):
    if name not in _cache:
        with gzip.open(os.path.join(GOLDEN, f"em_{name}.json.gz"), "rt") as fh:
            _cache[name] = json.load(fh)
    return _cache[name]


def arms():
    return json.load(open(os.path.join(GOLDEN, "em_arms.json")))


def model_code(fx):
    return MODEL_CODE.get(fx["model"]["emModel"], 2)


def ref_idx(fx):
    return np.array([{"a": 0, "c": 1, "g": 2, "t": 3}.get(ch, 0) for ch in fx["context"]["ref"].lower()], dtype=np.uint8)


def table_close(got, want, tol=1e-9):
    """|a - b| <= tol * max(|b|, scale), scale = the largest magnitude of the recorded table; returns the worst ratio to the bound
    (<= 1 passes)."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    scale = float(np.max(np.abs(want)))
    bound = tol * np.maximum(np.abs(want), scale)
    diff = np.abs(got - want)
    if not np.all(np.isfinite(got)):
        return float("inf")
    exact = diff == 0.0
    return float(np.max(np.where(exact, 0.0, diff / np.where(bound == 0.0, 1e-300, bound))))
