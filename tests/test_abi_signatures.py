"""maple_amd/abi.py -- the binding's declaration of the C side -- against include/maple_hip.h and include/maple_hip_debug.h:
every prototype (return type, parameter count, each parameter's C type, both directions), the six structs (fields, order, types,
and sizeof / offsetof as gcc lays them out), the constants, and what abi.bind does with a library of another ABI version, with a
missing symbol, and with the CPU twin handed in raw.  No GPU: the headers are read as text, gcc builds two tiny C files."""
import ctypes as C
import os
import re
import subprocess

import pytest

from maple_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = {"maple_hip.h": abi.SIGNATURES, "maple_hip_debug.h": abi.DEBUG_SIGNATURES}
RETURN_TYPES = {"int", "const char *"}


# ---- a parser of these two headers that cannot skip anything: every statement is a prototype, a struct, the enum, or an error --------
def norm(ctype):
    """'const  int32_t*' -> 'const int32_t *', 'maple_ctx * *' -> 'maple_ctx **'"""
    return " ".join(re.findall(r"\w+|\*", ctype)).replace("* *", "**")


def strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


class Header:
    def __init__(self, text):
        code = strip_comments(text)
        self.version = None
        m = re.search(r"^[ \t]*#[ \t]*define[ \t]+MAPLE_ABI_VERSION[ \t]+(\d+)[ \t]*$", code, flags=re.M)
        if m:
            self.version = int(m.group(1))
        # what the prototypes must add up to: every `maple_xxx (` outside the #define lines
        self.n_calls = len(re.findall(r"maple_\w+\s*\(", "\n".join(ln for ln in code.split("\n") if not re.match(r"\s*#\s*define\b", ln))))
        code = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif[^\n]*$", "", code, flags=re.S | re.M)   # extern "C" { / }
        assert not re.search(r"\\\n", code), "a continued preprocessor line: teach the parser"
        code = "\n".join(ln for ln in code.split("\n") if not ln.lstrip().startswith("#"))
        self.protos, self.structs, self.enum = {}, {}, {}
        for stmt in self.statements(code):
            self.statement(" ".join(stmt.split()))

    @staticmethod
    def statements(code):
        depth, cur = 0, []
        for ch in code:
            depth += (ch == "{") - (ch == "}")
            assert depth >= 0, "unbalanced braces"
            if ch == ";" and depth == 0:
                yield "".join(cur)
                cur = []
            else:
                cur.append(ch)
        assert depth == 0 and not "".join(cur).strip(), f"text after the last statement: {''.join(cur).strip()[:80]!r}"

    def statement(self, s):
        m = re.fullmatch(r"typedef struct \{(.*)\} (maple_\w+)", s)
        if m:
            self.structs[m.group(2)] = self.fields(m.group(2), m.group(1))
            return
        m = re.fullmatch(r"enum \{(.*)\}", s)
        if m:
            for item in m.group(1).split(","):
                k = re.fullmatch(r"\s*(MAPLE_\w+) = (-?\d+)\s*", item)
                assert k, f"enum item not understood: {item!r}"
                self.enum[k.group(1)] = int(k.group(2))
            return
        if s == "typedef struct maple_ctx maple_ctx":
            return
        m = re.fullmatch(r"(.*?)\b(maple_\w+) ?\((.*)\)", s)
        assert m, f"statement not understood: {s[:100]!r}"
        ret, name, params = norm(m.group(1)), m.group(2), m.group(3).strip()
        assert ret in RETURN_TYPES, f"{name}: return type {ret!r} not understood"
        assert name not in self.protos, f"{name} declared twice"
        out = []
        for p in ([] if params == "void" else params.split(",")):
            k = re.fullmatch(r"\s*(.*[\s*])(\w+)\s*", p)
            assert k and "(" not in p and "[" not in p, f"{name}: parameter {p!r} not understood"
            out.append((norm(k.group(1)), k.group(2)))
        self.protos[name] = (ret, out)

    @staticmethod
    def fields(struct, body):
        """[(field, C scalar type, array length or None)] in order; 'double a[16], b' declares two"""
        out = []
        for decl in body.split(";"):
            if not decl.strip():
                continue
            m = re.fullmatch(r"\s*(\w+)\s+(.*)", decl)
            assert m and m.group(1) in abi.SCALARS, f"{struct}: field declaration {decl!r} not understood"
            for d in m.group(2).split(","):
                k = re.fullmatch(r"\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d)
                assert k, f"{struct}: declarator {d!r} not understood"
                out.append((k.group(1), m.group(1), int(k.group(2)) if k.group(2) else None))
        return out


def parse(header):
    return Header(open(os.path.join(INCLUDE, header)).read())


def check_prototypes(hdr, table, header):
    """every prototype of the header is in the table with the same types, and the other way round"""
    assert len(hdr.protos) == hdr.n_calls, f"{header}: {hdr.n_calls} maple_*( in the text, {len(hdr.protos)} prototypes parsed"
    for name, (ret, params) in hdr.protos.items():
        assert name in table, f"{name} is declared in include/{header} but not in maple_amd/abi.py"
        t_ret, t_params = table[name]
        assert norm(t_ret) == ret, f"{name}: returns {ret!r} in include/{header}, {t_ret!r} in the table"
        assert len(t_params) == len(params), f"{name}: {len(params)} parameters in include/{header}, {len(t_params)} in the table"
        for i, ((ctype, pname), t) in enumerate(zip(params, t_params)):
            assert norm(t) == ctype, f"{name}: parameter {i} ({pname}) is {ctype!r} in include/{header}, {t!r} in the table"
    for name in table:
        assert name in hdr.protos, f"{name} is in the table of maple_amd/abi.py but not declared in include/{header}"


def check_struct(name, fields, cls):
    """the ctypes class restates the header's struct: the same fields in the same order with the matching types"""
    assert len(cls._fields_) == len(fields), f"{name}: {len(fields)} fields in the header, {len(cls._fields_)} in {cls.__name__}"
    for i, ((fname, ctype, count), (pname, ptype)) in enumerate(zip(fields, cls._fields_)):
        assert pname == fname, f"{name}: field {i} is {fname} in the header, {pname} in {cls.__name__}"
        want = abi.SCALARS[ctype] * count if count else abi.SCALARS[ctype]
        assert ptype is want, f"{name}.{fname}: {ctype}{f'[{count}]' if count else ''} in the header, {ptype.__name__} in {cls.__name__}"


# ---- header against table -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("header", list(HEADERS))
def test_table_matches_header(header):
    hdr = parse(header)
    assert hdr.protos
    check_prototypes(hdr, HEADERS[header], header)


def test_product_and_debug_tables_are_disjoint_and_named_apart():
    assert not set(abi.SIGNATURES) & set(abi.DEBUG_SIGNATURES)
    assert all(n.startswith("maple_debug_") for n in abi.DEBUG_SIGNATURES)
    assert not any(n.startswith("maple_debug_") for n in abi.SIGNATURES)


def test_every_declared_type_maps_to_ctypes():
    for name, (ret, params) in {**abi.SIGNATURES, **abi.DEBUG_SIGNATURES}.items():
        assert abi.ctype(ret) in (C.c_int, C.c_char_p), name
        for p in params:
            t = abi.ctype(p)
            if norm(p).endswith("*"):
                pointee = norm(p)[:-1].replace("const", "").strip()
                assert t is (C.POINTER(abi.STRUCTS[pointee]) if pointee in abi.STRUCTS else C.c_void_p), (name, p)
            else:
                assert t is abi.SCALARS[p], (name, p)
    with pytest.raises(KeyError):
        abi.ctype("long double")


def test_parser_refuses_what_it_does_not_know():
    ok = "int maple_a(maple_ctx *ctx, const int32_t *x);"
    assert Header(ok).protos == {"maple_a": ("int", [("maple_ctx *", "ctx"), ("const int32_t *", "x")])}
    for bad in ("#ifdef X\nextern int y;\n#endif\n" + ok,            # a statement that is no prototype
                "unsigned maple_b(void);",                           # an unknown return type
                "endif int maple_b(void);",                          # the rest of a directive swallowed into the return type
                "int maple_c(int (*cb)(int));",                      # a parameter the table could not state
                "typedef struct { int32_t *p; } maple_s;",           # a field the struct check could not state
                ok + ok,                                             # twice
                ok + "\nint maple_d(void)"):                         # no semicolon
        with pytest.raises(AssertionError):
            Header(bad)
    # a prototype the statements lose (here to the preprocessor) is still counted in the text, so the sum check fails
    lost = Header(ok + "\n#endif int maple_b(void);")
    assert lost.n_calls == 2 and len(lost.protos) == 1
    with pytest.raises(AssertionError, match="2 maple_.* in the text, 1 prototypes parsed"):
        check_prototypes(lost, {"maple_a": ("int", ("maple_ctx *", "const int32_t *"))}, "x.h")


# ---- structs ----------------------------------------------------------------------------------------------------------------------------
def header_structs():
    out = {}
    for header in HEADERS:
        out.update(parse(header).structs)
    return out


def test_struct_classes_restate_the_header():
    structs = header_structs()
    assert sorted(structs) == sorted(abi.STRUCTS) and len(structs) == 6
    for name, fields in structs.items():
        check_struct(name, fields, abi.STRUCTS[name])


def test_struct_layout_is_the_compilers(tmp_path):
    structs = header_structs()
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "maple_hip_debug.h"', "int main(void) {"]
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
        cls = abi.STRUCTS[name]
        assert C.sizeof(cls) == got[name, "sizeof"], f"sizeof({name}): {got[name, 'sizeof']} in C, {C.sizeof(cls)} in {cls.__name__}"
        for f, _, _ in fields:
            assert getattr(cls, f).offset == got[name, f], f"offsetof({name}, {f}): {got[name, f]} in C, {getattr(cls, f).offset} in {cls.__name__}"


# ---- constants --------------------------------------------------------------------------------------------------------------------------
def test_constants_are_the_headers():
    hdr = parse("maple_hip.h")
    assert hdr.version is not None and abi.ABI_VERSION == hdr.version
    errs = {k[len("MAPLE_"):]: v for k, v in hdr.enum.items() if k.startswith("MAPLE_ERR_")}
    assert len(errs) == 5 and hdr.enum["MAPLE_OK"] == 0
    mine = {k: v for k, v in vars(abi.MapleError).items() if k.startswith("ERR_")}
    assert mine == errs
    from maple_amd import runtime
    assert runtime.MapleError is abi.MapleError
    assert runtime.EXPORTS == list(abi.SIGNATURES) and runtime.DEBUG_EXPORTS == list(abi.DEBUG_SIGNATURES)


# ---- the checks above fail, and say where, when the two sides differ (on a header and a table of this test's own) ------------------------
TOY_HEADER = """typedef struct maple_ctx maple_ctx;
typedef struct { uint32_t structSize; double eff; int32_t fastPass; int32_t chunk; } maple_toy;
int maple_open(maple_ctx **out, const maple_toy *p);   /* a comment ( with maple_not_a_call( inside */
int maple_release(maple_ctx *ctx, int64_t mark);
"""
TOY_TABLE = {"maple_open": ("int", ("maple_ctx **", "const maple_toy *")), "maple_release": ("int", ("maple_ctx *", "int64_t"))}


class Toy(C.Structure):
    _fields_ = [("structSize", C.c_uint32), ("eff", C.c_double), ("fastPass", C.c_int32), ("chunk", C.c_int32)]


def test_a_difference_is_named():
    hdr = Header(TOY_HEADER)
    check_prototypes(hdr, TOY_TABLE, "toy.h")
    check_struct("maple_toy", hdr.structs["maple_toy"], Toy)
    with pytest.raises(AssertionError, match=r"maple_release: parameter 1 \(mark\) is 'int64_t' in include/toy.h, 'int32_t' in the table"):
        check_prototypes(hdr, {**TOY_TABLE, "maple_release": ("int", ("maple_ctx *", "int32_t"))}, "toy.h")
    with pytest.raises(AssertionError, match=r"maple_open: parameter 0 \(out\) is 'maple_ctx \*\*' in include/toy.h, 'maple_ctx \*' in the table"):
        check_prototypes(hdr, {**TOY_TABLE, "maple_open": ("int", ("maple_ctx *", "const maple_toy *"))}, "toy.h")
    with pytest.raises(AssertionError, match=r"maple_open: parameter 1 \(p\) is 'const maple_toy \*' in include/toy.h, 'maple_toy \*' in the table"):
        check_prototypes(hdr, {**TOY_TABLE, "maple_open": ("int", ("maple_ctx **", "maple_toy *"))}, "toy.h")
    with pytest.raises(AssertionError, match="maple_release: 2 parameters in include/toy.h, 1 in the table"):
        check_prototypes(hdr, {**TOY_TABLE, "maple_release": ("int", ("maple_ctx *",))}, "toy.h")
    with pytest.raises(AssertionError, match="maple_release is declared in include/toy.h but not in maple_amd/abi.py"):
        check_prototypes(hdr, {"maple_open": TOY_TABLE["maple_open"]}, "toy.h")
    with pytest.raises(AssertionError, match="maple_new_thing is declared in include/toy.h but not in maple_amd/abi.py"):
        check_prototypes(Header(TOY_HEADER + "int maple_new_thing(maple_ctx *ctx);\n"), TOY_TABLE, "toy.h")
    with pytest.raises(AssertionError, match="maple_no_such is in the table of maple_amd/abi.py but not declared in include/toy.h"):
        check_prototypes(hdr, {**TOY_TABLE, "maple_no_such": ("int", ())}, "toy.h")

    class Swapped(C.Structure):
        _fields_ = [Toy._fields_[i] for i in (0, 1, 3, 2)]
    with pytest.raises(AssertionError, match="maple_toy: field 2 is fastPass in the header, chunk in Swapped"):
        check_struct("maple_toy", hdr.structs["maple_toy"], Swapped)

    class Narrow(C.Structure):
        _fields_ = [("structSize", C.c_int32)] + Toy._fields_[1:]
    with pytest.raises(AssertionError, match=r"maple_toy.structSize: uint32_t in the header, c_int"):
        check_struct("maple_toy", hdr.structs["maple_toy"], Narrow)

    class Short(C.Structure):
        _fields_ = Toy._fields_[:3]
    with pytest.raises(AssertionError, match="maple_toy: 4 fields in the header, 3 in Short"):
        check_struct("maple_toy", hdr.structs["maple_toy"], Short)


# ---- bind on a stub library ---------------------------------------------------------------------------------------------------------------
def stub(tmp_path, tag, version, leave_out=()):
    names = [n for n in list(abi.SIGNATURES) if n != "maple_abi_version" and n not in leave_out]
    src, so = tmp_path / f"stub_{tag}.c", tmp_path / f"libstub_{tag}.so"
    src.write_text(f"int maple_abi_version(void) {{ return {version}; }}\n" + "".join(f"int {n}(void) {{ return 0; }}\n" for n in names))
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    return C.CDLL(str(so))


def test_bind_refuses_another_abi_version(tmp_path):
    with pytest.raises(abi.MapleError) as e:
        abi.bind(stub(tmp_path, "old", abi.ABI_VERSION - 1))
    assert re.search(rf"\b{abi.ABI_VERSION - 1}\b", str(e.value)) and re.search(rf"\b{abi.ABI_VERSION}\b", str(e.value))


def test_bind_names_a_missing_symbol_or_goes_without_it(tmp_path):
    gone = "maple_tree_optimize_blens"
    with pytest.raises(abi.MapleError, match=rf"does not export {gone} \(include/maple_hip\.h\)"):
        abi.bind(stub(tmp_path, "a", abi.ABI_VERSION, leave_out=[gone]))
    lib = stub(tmp_path, "b", abi.ABI_VERSION, leave_out=[gone])
    abi.bind(lib, require_all=False)
    abi.bind(lib, require_all=False)                                      # twice is harmless
    for n, (ret, params) in abi.SIGNATURES.items():
        if n != gone:
            assert getattr(lib, n).restype is abi.ctype(ret) and getattr(lib, n).argtypes == [abi.ctype(p) for p in params], n
    assert lib.maple_last_error.restype is C.c_char_p and lib.maple_set_tuning.argtypes == [C.c_void_p, C.POINTER(abi.MapleTuning)]
    with pytest.raises(abi.MapleError, match=r"does not export maple_debug_\w+ \(include/maple_hip_debug\.h\)"):
        abi.bind(stub(tmp_path, "c", abi.ABI_VERSION), debug=True)
    full = stub(tmp_path, "d", abi.ABI_VERSION)
    abi.bind(full)
    assert all(getattr(full, n).argtypes is not None for n in abi.SIGNATURES)


# ---- the CPU twin, handed to Device as a raw CDLL (what bench.py and tests/test_cpu_twin.py do) ---------------------------------------
def test_device_binds_a_library_handed_in_raw():
    import list_edges as le
    from maple_amd.runtime import Device
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-C", oracle, "-s"])
    lib = C.CDLL(os.path.join(oracle, "libmaple_cpu.so"))
    lib.maple_last_error.restype = C.c_char_p
    dev = Device(le.reference(), le.ROOT_FREQS, lib=lib)
    exported = [n for n in abi.SIGNATURES if hasattr(lib, n)]
    assert 20 <= len(exported) < len(abi.SIGNATURES)
    for n in exported:
        ret, params = abi.SIGNATURES[n]
        assert getattr(lib, n).argtypes == [abi.ctype(p) for p in params] and getattr(lib, n).restype is abi.ctype(ret), n
    with pytest.raises(C.ArgumentError):
        lib.maple_set_fatal_policy(dev.h, "1")                             # int: without argtypes a str goes over as a pointer
    with pytest.raises(C.ArgumentError):
        lib.maple_lists_sizes(dev.h, "3", None, None, None)                 # int32_t
    dev.set_fatal_policy(True)
    dev.close()
