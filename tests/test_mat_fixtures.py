"""The committed fixtures of the mutation events (tests/golden/mat_*.json.gz, mat_arms.json) are what the GPU tests take them for:
one per non-raising em_ fixture, consistent with its tree and model, the higher thresholds the threshold-0 records filtered, no
probability within MARGIN of a threshold, every appending line of the reference reached; maple_amd.ops.format_mat_annotation turns
the recorded records into the recorded text; and the binding's declaration of maple_tree_mutation_events and its two record
structs is the header's.  No GPU."""
import ctypes as C
import hashlib
import subprocess

import numpy as np
import pytest

import em_util
import mat_util as mu
from maple_amd import abi
from test_abi_signatures import INCLUDE, check_struct, parse

NAMES = mu.fixture_names()
HEADER = "maple_hip_mat.h"
APPEND_LINES = [10182, 10256, 10330, 10358, 10378, 10415, 10432, 10620, 10670, 10715, 10717, 10735, 10737, 10760, 10779, 10815,
                10817, 10825]


def test_the_expected_fixtures_exist():
    want = sorted(n for n in em_util.fixture_names() if em_util.load(n)["raised"] is None)
    assert NAMES == want and len(NAMES) == 20 and len(em_util.fixture_names()) == 21     # the twenty-first is the one that raises
    neg = mu.load(mu.NEGQ)
    assert em_util.load(mu.NEGQ)["raised"] is not None
    assert "exit" in neg["raised"] and len(neg["perThreshold"]) == 3 and all("exit" in r["raised"] for r in neg["perThreshold"])
    thr = mu.arms()["thresholds"]
    assert thr[:2] == [0.0, 0.01] and 0.3 <= thr[2] < 0.5 and abs(thr[2] * 100 - round(thr[2] * 100)) < 1e-9
    for name in NAMES:
        assert [r["minMutProb"] for r in mu.load(name)["thresholds"]] == thr, name
    assert [r["minMutProb"] for r in neg["perThreshold"]] == thr


@pytest.mark.parametrize("name", NAMES)
def test_records_are_consistent_with_the_tree(name):
    fx = mu.load(name)
    em = mu.em_of(fx)
    t, L, u = em["tree"], em["context"]["lRef"], bool(em["model"]["usingErrorRate"])
    n = t["n"]
    pair, single = mu.items(t, u)
    reached = set(pair) | set(single)
    zero = fx["thresholds"][0]
    for rec in fx["thresholds"]:
        thr = rec["minMutProb"]
        assert len(rec["mutationsInf"]) == len(rec["Ns"]) == n
        assert (rec["errors"] is not None) == u
        for v in range(n):
            for stream, col in (("mut", rec["mutationsInf"]), ("err", rec["errors"])):
                if col is None:
                    continue
                rl = col[v]
                assert not rl or v in pair, (name, v)                    # only a walked pair has any
                if stream == "err":
                    assert not rl or not t["children"][v], (name, v)     # errors only on leaves
                pos = [r[0] for r in rl]
                assert pos == sorted(pos) and all(1 <= p <= L for p in pos), (name, v)
                for p, fr, to, x in rl:
                    assert 0 <= to <= 3 and 0 <= fr <= (4 if stream == "err" else 3), (name, v, fr, to)
                    assert 0.0 <= x <= 1.0 + 1e-12 and (x > thr or x == 1.0), (name, v, x)
                # the threshold-0 records filtered by > (M:10760 appends its 1.0 whatever the threshold)
                assert rl == [r for r in (zero["mutationsInf"] if stream == "mut" else zero["errors"])[v] if r[3] > thr or r[3] == 1.0]
            ns = rec["Ns"][v]
            assert not ns or v in reached
            firsts = [x if isinstance(x, int) else x[0] for x in ns]
            assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts), (name, v)
            assert all(isinstance(x, int) or (len(x) == 2 and 1 <= x[0] <= x[1] <= L) for x in ns), (name, v)
            assert ns == zero["Ns"][v]                                   # no threshold touches them
        if rec["texts"] is not None:
            assert len(rec["texts"]) == n and rec["texts"][t["root"]] == rec["rootText"]
            assert hashlib.sha256("\n".join(rec["texts"]).encode()).hexdigest() == rec["sha256"]
    assert zero["texts"] is not None or "textsLeftOut" in fx


def test_the_fixtures_hold_the_shapes_the_format_distinguishes():
    """a run of one site recorded as a tuple, a bare int, `from` 4 in errors, M:10760's unconditional 1.0"""
    seen = set()
    for name in NAMES:
        rec = mu.load(name)["thresholds"][0]
        for ns in rec["Ns"]:
            for x in ns:
                seen.add("int" if isinstance(x, int) else ("run1" if x[0] == x[1] else "run"))
        if rec["errors"] is not None and any(r[1] == 4 for rl in rec["errors"] for r in rl):
            seen.add("from4")
        if any(r[3] == 1.0 for rl in mu.load(name)["thresholds"][2]["mutationsInf"] for r in rl):
            seen.add("sure")
    assert seen == {"int", "run1", "run", "from4", "sure"}


def test_margin_rule():
    thr = mu.arms()["thresholds"]
    assert mu.arms()["margin"] == mu.MARGIN
    smallest = 1.0
    for name in NAMES:
        rec = mu.load(name)["thresholds"][0]
        probs = np.asarray([r[3] for col in (rec["mutationsInf"], rec["errors"] or []) for rl in col for r in rl])
        smallest = min(smallest, float(probs.min()))
        for t in thr[1:]:
            assert np.all(np.abs(probs - t) > mu.MARGIN * t), (name, t)
    assert smallest > 1e-300                                             # `> 0.0` keeps every recorded probability


def test_every_appending_line_is_reached():
    arms = mu.arms()
    assert arms["lines"] == APPEND_LINES and arms["unreached"] == []
    assert all(arms["reached"][str(a)] for a in APPEND_LINES)
    for name in NAMES + [mu.NEGQ, mu.ROOT_NS]:
        for a in mu.load(name)["lines"]:
            assert name in arms["reached"][str(a)]
    # M:10825 (an O entry of a single-list leaf) needs a leaf that is no pair item: a model without an error rate
    for name in arms["reached"]["10825"]:
        if name != mu.ROOT_NS:
            assert not mu.em_of(mu.load(name))["model"]["usingErrorRate"], name


def test_root_ns_fixture():
    fx = mu.load(mu.ROOT_NS)
    five, lone = fx["cases"]
    t = five["tree"]
    assert t["n"] == 5 and t["dist"][2] == 0.0 and t["children"][2] and t["up"][0] is None
    ns = five["thresholds"][0]["Ns"]
    kinds = lambda col: {"int" if isinstance(x, int) else ("run" if x[1] > x[0] else "run1") for x in col}   # noqa: E731
    assert kinds(ns[0]) == {"int", "run"} and ns[2] == ns[0] and len(ns[0]) == 3     # (an O entry of an internal node: nothing)
    assert lone["tree"]["n"] == 1 and kinds(lone["thresholds"][0]["Ns"][0]) == {"int", "run"}
    assert any(isinstance(x, int) for x in lone["thresholds"][0]["Ns"][0][1:2])      # the O entry of a root that is a leaf
    for a in (10815, 10817, 10825):
        assert a in fx["lines"]
    # every committed tree leaves the root without Ns records: these are the ones that cover them
    for name in NAMES:
        em = mu.em_of(mu.load(name))
        assert mu.load(name)["thresholds"][0]["Ns"][em["tree"]["root"]] == []


def annotation(fx_out, tree, using_error_rate, rec, n):
    from maple_amd.ops import format_mat_annotation
    return format_mat_annotation(*mu.arrays(rec, n), root=tree["root"], up=tree["up"], children=tree["children"], dist=tree["dist"],
                                 errors_on=using_error_rate, effectivelyNon0BLen=fx_out["effectivelyNon0BLen"],
                                 supportFor0Branches=fx_out["supportFor0Branches"], root_state=mu.root_state_of(rec["rootText"]))


@pytest.mark.parametrize("name", NAMES)
def test_format_mat_annotation_gives_the_recorded_text(name):
    fx = mu.load(name)
    em = mu.em_of(fx)
    for rec in fx["thresholds"]:
        texts = annotation(fx["output"], em["tree"], bool(em["model"]["usingErrorRate"]), rec, em["tree"]["n"])
        if rec["texts"] is not None:
            assert texts == rec["texts"], (name, rec["minMutProb"])
        assert hashlib.sha256("\n".join(texts).encode()).hexdigest() == rec["sha256"], (name, rec["minMutProb"])


def test_format_mat_annotation_on_the_root_ns_trees():
    fx = mu.load(mu.ROOT_NS)
    for case in fx["cases"]:
        for rec in case["thresholds"]:
            assert annotation(fx["output"], case["tree"], False, rec, case["tree"]["n"]) == rec["texts"], case["label"]


def test_format_root_state():
    from maple_amd.ops import format_root_state
    vec = [(4, 9), (5, 12), (2, 1), (6, 0, [0.005, 0.295, 0.7, 0.0]), (4, 20), (6, 3, 1e-4, [0.25, 0.25, 0.25, 0.25])]
    assert format_root_state(vec, 0.01) == "rootState={N10-12,G13:1.0,C14:0.295,G14:0.7,A21:0.25,C21:0.25,G21:0.25,T21:0.25}"
    assert format_root_state([(4, 30)], 0.01) == "rootState={}"
    for name in NAMES:                                                   # the recorded roots are all of this shape
        for rec in mu.load(name)["thresholds"]:
            assert mu.root_state_of(rec["rootText"]).startswith("rootState={")


# ---- the binding ---------------------------------------------------------------------------------------------------------------
def test_the_header_declares_the_two_records_and_nothing_else():
    hdr = parse(HEADER)
    assert list(hdr.structs) == list(abi.MAT_STRUCTS) == ["maple_mut_event", "maple_n_run"]
    assert not hdr.protos and not hdr.enum and hdr.version is None
    assert not set(abi.MAT_STRUCTS) & (set(abi.STRUCTS) | set(abi.ROOT_SEARCH_STRUCTS))
    for name, fields in hdr.structs.items():
        check_struct(name, fields, abi.MAT_STRUCTS[name])


def test_the_layout_is_the_compilers_and_numpys(tmp_path):
    structs = parse(HEADER).structs
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "maple_hip.h"', "int main(void) {"]   # (as a caller includes it)
    for name, fields in structs.items():
        lines.append(f'    printf("{name} sizeof %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name} {f} %zu\\n", offsetof({name}, {f}));' for f, _, _ in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    ev_t, ns_t = mu.dtypes()
    for (name, fields), dt, size in zip(structs.items(), (ev_t, ns_t), (16, 8)):
        cls = abi.MAT_STRUCTS[name]
        assert C.sizeof(cls) == got[name, "sizeof"] == dt.itemsize == size
        assert list(dt.names) == [f for f, _, _ in fields]
        for f, _, _ in fields:
            assert getattr(cls, f).offset == got[name, f] == dt.fields[f][1], (name, f)


def test_the_prototype_is_in_the_table_and_the_header():
    ret, params = abi.SIGNATURES["maple_tree_mutation_events"]
    assert ret == "int" and len(params) == 13
    assert params[7] == params[11] == "maple_mut_event *" and params[9] == "maple_n_run *"
    assert abi.ctype(params[7]) is C.c_void_p and abi.ctype(params[9]) is C.c_void_p
    hdr = parse("maple_hip.h")
    assert [t for t, _ in hdr.protos["maple_tree_mutation_events"][1]] == [" ".join(p.split()) for p in params]
    assert hdr.version == abi.ABI_VERSION == 4                          # an addition breaks no caller
