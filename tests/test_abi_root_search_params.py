"""maple_root_search_params, the parameter struct of maple_tree_find_best_root: include/maple_hip_root_search.h against
abi.MapleRootSearchParams -- fields, order, types, and sizeof / offsetof as gcc lays them out -- with the parser and the checks of
tests/test_abi_signatures.py.  The struct has a header of its own (include/maple_hip.h includes it), so this is where it is held to
its ctypes class; the prototype that takes it is checked with every other one by test_abi_signatures.py.  No GPU."""
import ctypes as C
import subprocess

from maple_amd import abi
from test_abi_signatures import INCLUDE, check_struct, parse

HEADER = "maple_hip_root_search.h"


def test_the_header_declares_this_struct_and_nothing_else():
    hdr = parse(HEADER)
    assert list(hdr.structs) == list(abi.ROOT_SEARCH_STRUCTS) == ["maple_root_search_params"]
    assert not hdr.protos and not hdr.enum and hdr.version is None
    assert not set(abi.ROOT_SEARCH_STRUCTS) & set(abi.STRUCTS)


def test_the_class_restates_the_header():
    for name, fields in parse(HEADER).structs.items():
        check_struct(name, fields, abi.ROOT_SEARCH_STRUCTS[name])
    assert [f for f, _ in abi.MapleRootSearchParams._fields_][0] == "structSize"


def test_the_layout_is_the_compilers(tmp_path):
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
    assert len(got) == sum(1 + len(f) for f in structs.values())
    for name, fields in structs.items():
        cls = abi.ROOT_SEARCH_STRUCTS[name]
        assert C.sizeof(cls) == got[name, "sizeof"] == 40
        for f, _, _ in fields:
            assert getattr(cls, f).offset == got[name, f], (name, f)


def test_the_prototype_names_the_struct_and_the_binding_passes_a_pointer():
    ret, params = abi.SIGNATURES["maple_tree_find_best_root"]
    assert params[2] == "const maple_root_search_params *" and abi.ctype(params[2]) is C.c_void_p
    assert "maple_tree_find_best_root" in parse("maple_hip.h").protos
