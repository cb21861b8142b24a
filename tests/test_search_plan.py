"""The SPR tiers' pool and launch sizing (maple_amd/csrc/search_plan.h) on the CPU: tests/search_plan_main.cpp, compiled on its
own with the host sanitizers, against plans recorded from the arithmetic as it stood inside frontier_search and run_queries
before it moved (tests/golden/search_plan_cases.json), and against properties that hold whatever computes the plans."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
SZ_ITEM, SZ_VISIT = 96, 32               # sizeof(FItem), sizeof(FVisit) (frontier_dev.h asserts both)


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "search_plan_cases.json")))


def lines_of(golden):
    return [c["kind"] + " " + " ".join(str(v) for v in c["in"]) for c in golden["cases"]]


def run(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return [(ln[0], [int(v) for v in ln[1:]]) for ln in out]


@pytest.fixture(scope="module")
def plans(golden, tmp_path_factory):
    """every case of the golden file through the program, once: [(kind, numbers)]"""
    assert shutil.which("g++"), "g++ is needed to compile tests/search_plan_main.cpp"
    program = str(tmp_path_factory.mktemp("search_plan") / "search_plan_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", program, os.path.join(HERE, "search_plan_main.cpp")])
    got = run(program, lines_of(golden))
    again = run(program, lines_of(golden)[::-1])[::-1]
    return got, again


def named(golden, plans, kind):
    names_in, names_out = golden[{"F": "frontier_in", "L": "lane_in"}[kind]], golden[{"F": "frontier_out", "L": "lane_out"}[kind]]
    for case, (k, out) in zip(golden["cases"], plans[0]):
        if case["kind"] == kind:
            assert k == kind and len(out) == len(names_out) and len(case["in"]) == len(names_in), case["name"]
            yield case["name"], dict(zip(names_in, case["in"])), dict(zip(names_out, out))


def test_plans_equal_the_recorded_ones(golden, plans):
    assert 100 < len(golden["cases"]) <= 256
    for case, (kind, out) in zip(golden["cases"], plans[0]):
        names = golden["frontier_out" if kind == "F" else "lane_out"]
        assert kind == case["kind"]
        diff = {n: (g, w) for n, g, w in zip(names, out, case["out"]) if g != w}
        assert len(out) == len(case["out"]) and not diff, f"{case['name']}: (got, recorded) {diff}"


def test_same_input_same_plan(plans):
    assert plans[0] == plans[1]


def test_no_pool_is_planned_below_what_it_holds(golden, plans):
    # (the per-lane slabs and the shared regions are asked for exactly: a request below the capacity leaves a buffer as it is)
    pools = {"itemsU": "resItemsU", "itemsC": "resItemsC", "recs": "resRecs", "tw": "resTw", "ta": "resTa", "trec": "resTrec", "arec": "resArec",
             "tflag": "resTflag", "perm": "resPerm", "perm2": "resPerm2", "perm3": "resPerm3", "perm4": "resPerm4"}
    layout = {"visit": "resVisit", "lsize": "resLsize", "lpos": "resLpos", "lpar": "resLpar"}
    passes = {"passList": "resPassList", "passListR": "resPassListR"}
    for name, i, o in named(golden, plans, "F"):
        for cap, res in list(pools.items()) + (list(layout.items()) if o["layoutOK"] else []) + (list(passes.items()) if i["matTree"] else []):
            assert o[res] >= i[cap], (name, cap)
        assert o["capU"] >= i["itemsU"] // SZ_ITEM and o["capC"] >= i["itemsC"] // SZ_ITEM and o["capW"] >= i["tw"] and o["capA"] >= i["ta"], name
        assert o["capL"] >= min(i["trec"], i["tflag"]) and o["capE"] >= i["capE"], name
        # ... and none below what was planned for this call
        assert o["capU"] >= o["planU"] and o["capC"] >= o["planC"] + o["planR"] and o["capL"] >= o["planL"], name
        assert o["capW"] >= o["planW"] and o["capA"] >= o["planA"] and o["boundRecs"] >= o["capRecs"], name


def test_cached_pool_splits_into_two_parts(golden, plans):
    for name, i, o in named(golden, plans, "F"):
        roots = o["capC"] - o["capCC"]
        assert 0 <= o["capCC"] and roots >= 1 << 16 and o["capCC"] + roots == o["capC"] == max(i["itemsC"], o["resItemsC"]) // SZ_ITEM, name
        assert roots >= o["planR"], name
        assert o["capVisit"] == o["capU"] + o["capC"] and o["layoutOK"] == (i["m"] > 64 and o["capVisit"] < 2 ** 31 - 64), name


def test_growth_that_was_cut_fits_the_room(golden, plans):
    per_item = SZ_ITEM + SZ_VISIT + 12
    checked = 0
    for name, i, o in named(golden, plans, "F"):
        if not o["growthCut"]:
            continue
        fixed = (o["scratchLanes"] + o["extraSlabs"]) * o["capE"] * 64 + (o["capBig"] + o["capBig2"]) * 48
        base = (i["itemsC"] // SZ_ITEM + i["itemsU"] // SZ_ITEM) * per_item + (i["tw"] + i["ta"]) * 8 + min(i["trec"], i["tflag"]) * 24 + fixed
        room = o["room2"] / 2
        floors = {"planC": 1 << 16, "planR": 1 << 16, "planU": 1 << 14, "planL": 1 << 15, "planW": 1 << 20, "planA": 1 << 20}
        if base > room or any(o[k] <= v for k, v in floors.items()):      # (nothing left to share out / a pool at its least size)
            continue
        total = (o["planC"] + o["planR"] + o["planU"]) * per_item + (o["planW"] + o["planA"]) * 8 + o["planL"] * 24 + fixed
        assert total <= room * (1 + 1e-12), name                          # (each term is truncated: never above)
        checked += 1
    assert checked >= 20                                                  # (the sweep's rounds on a device with little free: "sweep C*")


def test_scratch_lanes_are_a_power_of_two_fraction_of_the_gpu(golden, plans):
    for name, i, o in named(golden, plans, "F"):
        lanes = o["scratchLanes"]
        assert lanes >= 16384 and 262144 % lanes == 0 and (262144 // lanes) & (262144 // lanes - 1) == 0, name
        assert o["gridUpd"] * 256 == lanes, name
        if i["m"] <= 64:
            assert (lanes, o["heavyMin"], o["bigMin"], o["groupLevels"], o["layoutOK"]) == (16384, 1, 1 << 30, 2, 0), name


def test_lane_launch_geometry(golden, plans):
    for name, i, o in named(golden, plans, "L"):
        assert o["lanes"] == o["nWaves"] * o["activeLanes"] and 1 <= o["activeLanes"] <= 64 and 1 <= o["nWaves"] <= 8192, name
        assert 64 <= o["maxLanes"] <= 4096 * 64 and o["lanesWanted"] == min(i["m"], o["maxLanes"]), name
        parts = [o[k] for k in ("bytesW", "bytesAux", "bytesH", "bytesSt", "bytesBest", "bytesAis")]
        assert sum(parts) == o["bytesTotal"] and all(p % 64 == 0 for p in parts), name
        # the workspace after the reserve holds every lane of the launch
        assert max(i["wsCap"], o["reserve"]) >= o["lanes"] * o["bytesTotal"], name
        if i["assist"] and not i["cached"]:
            assert o["activeLanes"] <= 4, name
