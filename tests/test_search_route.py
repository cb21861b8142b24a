"""Which search of an SPR round goes where (the routing rules of maple_amd/csrc/search_plan.h) on the CPU: tests/search_route_main.cpp,
compiled on its own with the host sanitizers, against what the rules gave as they stood inline in maple_spr_search_batch before they
moved (tests/golden/search_route_cases.json), and against properties that hold whatever computes them."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
FLAGS = ["-std=c++17", "-O1", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "search_route_cases.json")))


def lines_of(golden):
    return [c["kind"] + " " + " ".join(repr(v) for v in c["in"]) for c in golden["cases"]]


def run(program, lines):
    r = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr[-2000:]
    out = [ln.split() for ln in r.stdout.splitlines()]
    assert len(out) == len(lines)
    return [(ln[0], [int(v) for v in ln[1:]]) for ln in out]


@pytest.fixture(scope="module")
def routes(golden, tmp_path_factory):
    """every case of the golden file through the program, once in order and once in reverse: [(kind, numbers)]"""
    assert shutil.which("g++"), "g++ is needed to compile tests/search_route_main.cpp"
    program = str(tmp_path_factory.mktemp("search_route") / "search_route_main")
    subprocess.check_call(["g++"] + FLAGS + ["-o", program, os.path.join(HERE, "search_route_main.cpp")])
    got = run(program, lines_of(golden))
    again = run(program, lines_of(golden)[::-1])[::-1]
    return got, again


def of_kind(golden, routes, kind):
    for case, (k, out) in zip(golden["cases"], routes[0]):
        if case["kind"] == kind:
            yield case["name"], case["in"], out


def test_rules_equal_the_recorded_ones(golden, routes):
    kinds = [c["kind"] for c in golden["cases"]]
    assert all(kinds.count(k) >= 20 for k in "PBSKRWCGH") and len(kinds) <= 1024
    for case, (kind, out) in zip(golden["cases"], routes[0]):
        assert kind == case["kind"] and out == case["out"], f"{case['name']}: got {out}, recorded {case['out']}"


def test_same_input_same_answer(routes):
    assert routes[0] == routes[1]


def test_the_named_cases_are_there(golden):
    names = " | ".join(c["name"] for c in golden["cases"])
    for part in ("budget req=0 nScored=0 ", "budget req=300 ", "budget req=-1 ", "nScored=63 ", "nScored=64 ", "nScored=16384 ", "nScored=524288 ",
                 "nScored=524289 ", "uer=1 patchedOnly=1", "rows: free unknown", "rows: half of free below 4 GiB", "between 4 and 96 GiB", "above 96 GiB",
                 "clamps to 1", "63 candidates", "64 candidates", "more candidates than rows", "split: no spare rows", "split: some spare rows",
                 "more unannounced searches than spare rows", "split: matPre", "run out at k = 0", "k = 2047", "k = 2048", "bound not hit", "8 Mi",
                 "need below the capacity", "between the capacity and twice it", "need above chunk rows", "the budget changed", "the threshold changed",
                 "status -5 with nAppend -1", "nAppend at wideBudget / 4", "came back with one more"):
        assert part in names, part


def test_one_rule_for_both_row_budgets(golden, routes):
    """pre_rows_max and the chunk of the dense tier were the same arithmetic, the chunk clamped to one row: score_rows_max is the chunk's"""
    clamped = 0
    for case, (name, i, o) in zip([c for c in golden["cases"] if c["kind"] == "S"], of_kind(golden, routes, "S")):
        assert o[0] == max(1, case["rows_before_clamp"]) and o[0] >= 1, name
        clamped += case["rows_before_clamp"] == 0
        known, free, cap, n = i
        budget = max(4 << 30, min((free + cap) // 2, 96 << 30)) if known else 4 << 30
        assert o[0] == max(1, budget // (8 * n)), name
    assert clamped >= 2


def test_rows_made_ahead_fit_the_table(golden, routes):
    for name, i, (kind, made, spare) in of_kind(golden, routes, "K"):
        n_cand, rows_max = i[-2:]
        if made:
            assert kind in (1, 2) and 64 <= n_cand and n_cand + spare <= rows_max and 0 <= spare <= 4096, name
            assert spare == 0 or kind == 1, name
        else:
            assert spare == 0, name


def test_split_wide_keeps_every_search_once(golden, routes):
    for name, i, o in of_kind(golden, routes, "W"):
        m_z, spare, mat, n_batch, n_wide = i[:5]
        wide, row_of = i[5:5 + n_wide], i[5 + n_wide:]
        n_take = o[0]
        take, rows = o[1:1 + n_take], o[1 + n_take:1 + 2 * n_take]
        n_rest = o[1 + 2 * n_take]
        rest, n_spare = o[2 + 2 * n_take:2 + 2 * n_take + n_rest], o[-1]
        assert len(o) == 3 + 2 * n_take + n_rest, name
        assert sorted(take + rest) == sorted(wide) and len(set(take + rest)) == len(wide), name
        # in the order they came; rows distinct and inside the table; spare rows handed out in order, no more than there are
        assert take == [w for w in wide if w in set(take)] and rest == [w for w in wide if w in set(rest)], name
        assert len(set(rows)) == len(rows) and all(0 <= r < m_z + spare for r in rows), name
        assert [r for r in rows if r >= m_z] == list(range(m_z, m_z + n_spare)) and n_spare <= spare, name
        assert all(r == row_of[t] for t, r in zip(take, rows) if r < m_z) and all(row_of[t] < 0 for t, r in zip(take, rows) if r >= m_z), name
        if mat:
            assert not take and rest == wide, name
        else:
            assert all(row_of[w] < 0 for w in rest) and (not rest or n_spare == spare), name


def test_frame_chunk_never_takes_more_than_offered(golden, routes):
    for name, i, (m, lane_only) in of_kind(golden, routes, "C"):
        n_f, free_ent, free_aux, n_runs = i[:4]
        runs = [i[4 + 3 * r:7 + 3 * r] for r in range(n_runs)]                 # (count, entries, aux values) of the lists offered
        n_ent, n_aux = [e for cnt, e, a in runs for _ in range(cnt)], [a for cnt, e, a in runs for _ in range(cnt)]
        offered = len(n_ent)
        assert 0 <= m <= offered, name
        # what is taken fits a third of the arena and 8 Mi (query, frame) items; what is left out would not have
        assert n_f * (sum(n_ent[:m]) + 24 * m) <= free_ent // 3 and n_f * (sum(n_aux[:m]) + 8 * m) <= free_aux // 3 and m * n_f <= 8 << 20, name
        if m < offered:
            assert (n_f * (sum(n_ent[:m + 1]) + 24 * (m + 1)) > free_ent // 3 or n_f * (sum(n_aux[:m + 1]) + 8 * (m + 1)) > free_aux // 3
                    or (m + 1) * n_f > 8 << 20), name
        assert lane_only == (m < offered and m < 2048), name


def test_cache_reserve_holds_the_chunk(golden, routes):
    for name, (need, cap, chunk_rows, n_nodes), (res,) in of_kind(golden, routes, "G"):
        assert max(res, cap) >= need, name
        if need > cap:                                                     # grows by doubling, up to a full chunk's rows
            assert res >= min(2 * cap, max(chunk_rows * n_nodes, need)) and res <= max(2 * cap, need), name
        else:
            assert res == need, name
