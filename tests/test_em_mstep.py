"""The maximisation part of the EM step (maple_amd/csrc/em_mstep.h, M:10852-10947) on the CPU: tests/em_mstep_main.cpp, compiled
on its own with the host sanitizers, is fed the statistics recorded from the reference at M:10852 and must return the
reference's 4-tuple to 1e-12 relative (no reordering on this path)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import em_util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
NAMES = [n for n in em_util.fixture_names() if "ret" in em_util.load(n)]


def case_text(fx, model=None):
    m, raw, L = fx["model"], fx["raw"], fx["context"]["lRef"]
    rv, u, ss = m["useRateVariation"], m["usingErrorRate"], m["errorRateSiteSpecific"]
    f = lambda xs: " ".join(repr(float(x)) for x in xs)                  # noqa: E731
    out = [f"{L} {em_util.model_code(fx) if model is None else model} {int(rv)} {int(u)} {int(ss)} {raw['numTips']} "
           f"{raw.get('observedTotNucsSites', 0)} {raw.get('errorCount', 0.0)!r} {raw.get('totTreeLength', 0.0)!r}",
           " ".join(str(int(x)) for x in em_util.ref_idx(fx)), f(fx["context"]["rootFreqs"]),
           f(x for row in raw["counts"] for x in row), f(raw["waitingTimes"])]
    if rv:
        out += [f(x for row in raw["waitingTimesSites"] for x in row), f(raw["countsSites"]), f(raw["trackingNs"])]
    if ss:
        out += [f(raw["observedNucsSites"]), f(raw["errorCountSites"])]
    return "\n".join(out) + "\n"


def parse(line):
    t = line.split()
    rc, q = int(t[0]), [float(x) for x in t[1:17]]
    k = 17
    n = int(t[k]); sr = [float(x) for x in t[k + 1:k + 1 + n]]; k += 1 + n          # noqa: E702
    has = int(t[k]); er = float(t[k + 1]) if has else None; k += 1 + has             # noqa: E702
    n = int(t[k]); se = [float(x) for x in t[k + 1:k + 1 + n]]                       # noqa: E702
    return rc, q, sr, er, se


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/em_mstep_main.cpp"
    exe = str(tmp_path_factory.mktemp("em_mstep") / "em_mstep_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", exe, os.path.join(HERE, "em_mstep_main.cpp")])
    return exe


def run(program, text):
    r = subprocess.run([program], input=text, capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    return [parse(ln) for ln in r.stdout.splitlines()]


def rel_close(got, want, tol=1e-12):
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    return got.shape == want.shape and bool(np.all(np.abs(got - want) <= tol * np.maximum(np.abs(got), np.abs(want))))


@pytest.mark.parametrize("name", NAMES)
def test_mstep_returns_the_recorded_tuple(program, name):
    fx = em_util.load(name)
    (rc, q, sr, er, se), = run(program, case_text(fx))
    ret, L = fx["ret"], fx["context"]["lRef"]
    assert rc == 0
    assert rel_close(q, ret["Q"]), name
    assert (ret["siteRates"] is None and not sr) or rel_close(sr, ret["siteRates"])
    assert (ret["errorRate"] is None and er is None) or rel_close([er], [ret["errorRate"]])
    assert (ret["siteErrRates"] is None and not se) or rel_close(se, ret["siteErrRates"])
    # the clamps are hit exactly where the reference hits them
    for got, want, clamps in ((sr, ret["siteRates"], (0.001, 0.005 * L)), (se, ret["siteErrRates"], (1e-10,))):
        if want is not None:
            for c in clamps:
                assert [i for i, x in enumerate(want) if x == c] == [i for i, x in enumerate(got) if x == c]


def test_several_cases_in_one_stream_and_unknown_model(program):
    a, b = em_util.load("cat_zero_plain"), em_util.load("cat_zero_full")
    out = run(program, case_text(a) + case_text(b) + case_text(a, model=2) + case_text(b, model=2))
    assert [o[0] for o in out] == [0, 0, -1, 0]                          # M:10877: only without an error model
    assert rel_close(out[0][1], a["ret"]["Q"]) and rel_close(out[1][1], b["ret"]["Q"])
