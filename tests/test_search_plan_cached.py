"""The cached launches the frontier plan queues behind an updating level (maple_amd/csrc/search_plan.h: cached_behind) on the CPU:
tests/search_plan_cached_main.cpp, compiled on its own with the host sanitizers, over the frontier scenarios of
tests/golden/search_plan_cases.json.  Every cached launch takes a snapshot of what is complete, so the count changes no search;
it is pinned here because it decides how many launches a round makes."""
import json
import os
import shutil
import subprocess

import pytest

from test_search_plan import FLAGS, HERE

EARLY_LEVELS = 6                         # the levels of a whole round that hold 95 % of its updating items
EARLY, LATER = 4, 2                      # launches behind each of them / behind a later level (2, 3 and 4 measured)


@pytest.fixture(scope="module")
def behind(tmp_path_factory):
    assert shutil.which("g++"), "g++ is needed to compile tests/search_plan_cached_main.cpp"
    golden = json.load(open(os.path.join(HERE, "golden", "search_plan_cases.json")))
    lines = ["F " + " ".join(str(v) for v in c["in"]) for c in golden["cases"] if c["kind"] == "F"]
    program = str(tmp_path_factory.mktemp("search_plan_cached") / "search_plan_cached_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", program, os.path.join(HERE, "search_plan_cached_main.cpp")])
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(out) == len(lines) > 50
    return out


def test_a_handful_of_searches_keeps_two_launches_behind_every_level(behind):
    few = [row for row in behind if row[0] <= 64]
    assert few
    for m, later, early, n_early, *per_level in few:
        assert (later, early) == (2, 2) and per_level == [2] * 12, m


def test_a_whole_round(behind):
    whole = [row for row in behind if row[0] > 64]
    assert any(row[0] >= 100000 for row in whole)
    for m, later, early, n_early, *per_level in whole:
        assert (later, early, n_early) == (LATER, EARLY, EARLY_LEVELS), m
        assert per_level == [EARLY] * EARLY_LEVELS + [LATER] * (12 - EARLY_LEVELS), m


def test_every_level_gets_a_launch(behind):
    # (the roots an updating level publishes are only ever scored by a cached launch queued after it)
    assert all(min(row[4:]) >= 1 for row in behind)
