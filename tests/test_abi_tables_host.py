"""The binding's tables against the headers they are read from (gnn-fpga_amd/_abi.py), with the C compiler as the second
reader: every signature and struct layout as clang sees the four headers, the parser's refusals, and the names.  No GPU."""
import ctypes
import json
import os
import re
import subprocess
from ctypes import POINTER, c_char_p, c_void_p

import pytest

from gnn_fpga_amd import _abi, _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(REPO, "include")
HEADERS = {"SIGNATURES": "gnn_hip.h", "ITER_SIGNATURES": "gnn_hip_iter.h", "FX_SIGNATURES": "gnn_hip_fixed.h",
           "FXEV_SIGNATURES": "gnn_hip_fixed_events.h"}          # in include order
STRICT_C = ["-std=c11", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE]

# the published rule, restated on clang's type strings
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double}
TYPED = {("gnn_plan_limits", "out4"): POINTER(ctypes.c_int32), ("gnn_plan_route", "out"): POINTER(ctypes.c_int32),
         ("gnn_profile_end", "names"): POINTER(c_char_p), ("gnn_profile_end", "ms"): POINTER(ctypes.c_float)}


def _clang():
    """The clang of the installation the Makefile's HIPCC comes from; its absence fails the test (the build needs it)."""
    hipcc = os.environ.get("HIPCC") or re.search(r"^HIPCC\s*\?=\s*(\S+)", open(os.path.join(
        REPO, "gnn-fpga_amd", "csrc", "Makefile")).read(), re.M)[1]
    root = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    found = [p for p in (os.path.join(root, "lib", "llvm", "bin", "clang"), os.path.join(root, "llvm", "bin", "clang"))
             if os.path.exists(p)]
    assert found, "no clang beside %s" % hipcc
    return found[0]


def _class_name(c_name):
    return "".join(p.capitalize() for p in c_name[:-2].split("_"))


def _header(name):
    text = open(os.path.join(INCLUDE, name)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.fixture(scope="module")
def compiled():
    """clang's reading: {table: {function: (return type, [(parameter, type)])}}, {struct typedef: [(field, type)]}."""
    functions, structs, seen = {}, {}, set()
    for table, header in HEADERS.items():
        out = subprocess.run([_clang(), "-x", "c", "-fsyntax-only", "-Xclang", "-ast-dump=json"] + STRICT_C +
                             [os.path.join(INCLUDE, header)], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr          # the headers stay plain C11, free of warnings
        decls = json.loads(out.stdout)["inner"]
        records = {d["id"]: d for d in decls if d["kind"] == "RecordDecl"}
        functions[table] = {}
        for d in decls:
            if d["kind"] == "FunctionDecl" and d["name"].startswith("gnn_") and d["name"] not in seen:
                seen.add(d["name"])
                params = [(p["name"], p["type"]["qualType"]) for p in d.get("inner", []) if p["kind"] == "ParmVarDecl"]
                functions[table][d["name"]] = (d["type"]["qualType"].split("(")[0].strip(), params)
            if d["kind"] == "TypedefDecl" and d["name"].startswith("gnn_"):
                record = records[d["inner"][0]["decl"]["id"]]
                assert all(f["kind"] == "FieldDecl" and not f.get("isBitfield") for f in record["inner"]), d["name"]
                structs[d["name"]] = [(f["name"], f["type"]["qualType"]) for f in record["inner"]]
    return functions, structs


def _expected(qual, structs, ret=False):
    array = re.fullmatch(r"(.*?)\s*\[(\d+)\]", qual)
    if array:
        return _expected(array[1], structs) * int(array[2])
    if ret and qual == "const char *":
        return c_char_p
    if qual.endswith("*"):
        base = qual.rstrip("* ")
        const, base = base.startswith("const "), re.sub(r"^const ", "", base)
        if base in structs:
            return POINTER(getattr(_abi, _class_name(base))) if const else c_void_p
        assert base in SCALARS or base in ("void", "char"), qual
        return c_void_p
    return SCALARS[qual] if qual in SCALARS else getattr(_abi, _class_name(qual))


def _same(a, b):
    if isinstance(a, type) and issubclass(a, ctypes.Array):
        return isinstance(b, type) and issubclass(b, ctypes.Array) and a._length_ == b._length_ and \
            _same(a._type_, b._type_)
    return a is b


def test_signatures_are_the_compilers(compiled):
    functions, structs = compiled
    assert sum(map(len, functions.values())) == 91 and len(structs) == 20
    typed, by_reference, device_structs = dict(TYPED), 0, []
    for table, declared in functions.items():
        bound = getattr(_abi, table)
        assert getattr(_lib, table) is bound
        assert sorted(bound) == sorted(declared)
        for name, (ret, params) in declared.items():
            restype, argtypes = bound[name]
            assert restype is _expected(ret, structs, ret=True), name
            assert len(argtypes) == len(params), name
            for got, (param, qual) in zip(argtypes, params):
                want = typed.pop((name, param), None) or _expected(qual, structs)
                assert got is want, (name, param, qual, got)
                by_reference += re.sub(r"^const | \*$", "", qual) in structs and qual.startswith("const ")
                if re.sub(r" \*$", "", qual) in structs:
                    device_structs.append(name)
    assert not typed
    assert by_reference == 66
    assert sorted(device_structs) == ["gnn_event_graphs_sizes", "gnn_graph_build_sizes", "gnn_hit_samples_sizes",
                                      "gnn_muon_graph_sizes", "gnn_plan_build_sizes", "gnn_plan_build_sizes_graphs",
                                      "gnn_select_hits_sizes"]


def test_struct_fields_and_layouts_are_the_compilers(compiled, tmp_path):
    _, structs = compiled
    lines = ["#include <stddef.h>", "#include <stdio.h>"] + ['#include "%s"' % h for h in HEADERS.values()]
    lines.append("int main(void) {")
    for c_name, fields in structs.items():
        cls = getattr(_abi, _class_name(c_name))
        assert getattr(_lib, cls.__name__) is cls and issubclass(cls, ctypes.Structure)
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields], c_name
        for (field, got), (_, qual) in zip(cls._fields_, fields):
            assert _same(got, _expected(qual, structs)), (c_name, field, qual, got)
        lines.append('    printf("%s %%zu\\n", sizeof(%s));' % (c_name, c_name))
        lines += ['    printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (c_name, f, c_name, f) for f, _ in fields]
    lines += ["    return 0;", "}", ""]
    source, program = tmp_path / "layout.c", tmp_path / "layout"
    source.write_text("\n".join(lines))
    subprocess.run([_clang()] + STRICT_C + [str(source), "-o", str(program)], check=True)
    compiler = dict(line.split() for line in subprocess.run([str(program)], capture_output=True, text=True,
                                                            check=True).stdout.splitlines())
    binding = {}
    for c_name, fields in structs.items():
        cls = getattr(_abi, _class_name(c_name))
        binding[c_name] = str(ctypes.sizeof(cls))
        binding.update(("%s.%s" % (c_name, f), str(getattr(cls, f).offset)) for f, _ in fields)
    assert binding == compiler


@pytest.mark.parametrize("snippet, quoted", [
    ("unsigned gnn_x(void);", "unsigned"),
    ("typedef struct gnn_b { int32_t a : 3; } gnn_b_t;", "a : 3"),
    ("#define GNN_F(x) (x)", "GNN_F(x) (x)"),
    ("static inline int gnn_y(void) { return 0; }", "static inline int gnn_y(void) { return 0; }"),
    ("typedef int gnn_z_t;", "typedef int gnn_z_t;"),
    ("int gnn_ok(void);\nint gnn_w(int32_t);", "int gnn_w(int32_t);"),
    ("enum { GNN_A = 4, GNN_B };", "GNN_A = 4"),
    ("typedef struct { float v[GNN_UNKNOWN]; } gnn_v_t;", "GNN_UNKNOWN"),
    ("typedef struct { gnn_later_t s; } gnn_u_t;", "gnn_later_t"),
    ("#define GNN_HALF 0.5", "GNN_HALF 0.5"),
])
def test_parser_refuses_what_it_does_not_read(snippet, quoted):
    with pytest.raises(_abi.GnnHipError, match=re.escape(quoted)):
        _abi.read_abi([("SIGNATURES", snippet)], {})


def test_parser_refuses_a_typed_pointer_the_headers_do_not_declare():
    text = "int gnn_x(int32_t *out);"
    assert _abi.read_abi([("SIGNATURES", text)], {("gnn_x", "out"): POINTER(ctypes.c_int32)})["SIGNATURES"] == \
        {"gnn_x": (ctypes.c_int, [POINTER(ctypes.c_int32)])}
    for key in (("gnn_x", "nope"), ("gnn_nope", "out")):
        with pytest.raises(_abi.GnnHipError, match=key[1] if key[0] == "gnn_x" else key[0]):
            _abi.read_abi([("SIGNATURES", text)], {key: POINTER(ctypes.c_int32)})


def test_names_and_constants_are_the_headers():
    defines, enumerators, classes = {}, {}, []
    for table, header in HEADERS.items():
        text = _header(header)
        names = set(re.findall(r"\b(gnn_[a-z0-9_]+)\s*\(", text))
        assert set(getattr(_lib, table)) == names, table
        classes += re.findall(r"\}\s*(gnn_\w+_t)\s*;", text)
        defines.update((n, int(v)) for n, v in re.findall(r"#define\s+(GNN_\w+)\s+\(?(-?\d+)\)?\s", text))
        for body in re.findall(r"\benum\s*\{(.*?)\}", text, flags=re.S):
            enumerators.update((n.strip(), i) for i, n in enumerate(body.split(",")))
    assert len(classes) == 20 and len(defines) == 31 and len(enumerators) == 26
    for c_name in classes:
        assert issubclass(getattr(_lib, _class_name(c_name)), ctypes.Structure), c_name
    for name, value in {**defines, **enumerators}.items():
        assert getattr(_lib, name) == value and type(getattr(_lib, name)) is int, name
    assert _lib.SELECT_HITS_MAX_LAYERS == defines["GNN_SELECT_HITS_MAX_LAYERS"]
    # the plan builder's status bits and the graph-local hit cap: what plan_hip.py decodes and decides with
    status = {k: v for k, v in defines.items() if k.startswith("GNN_PLAN_ST_")}
    assert sorted(status.values()) == [1, 2, 4, 8, 16, 32, 64, 128]
    assert (status["GNN_PLAN_ST_ENDPOINT"], status["GNN_PLAN_ST_FAST_MISS"]) == (64, 128)
    assert defines["GNN_PLAN_GRAPH_CAP_HITS"] == 19456
    assert len(_lib.ROUTE_FIELDS) == enumerators["GNN_ROUTE_FIELDS"]


def test_missing_headers_and_another_abi_version_are_refused(monkeypatch, tmp_path):
    monkeypatch.setattr(_abi, "INCLUDE_DIR", str(tmp_path / "include"))
    with pytest.raises(_lib.GnnHipError, match="reads its signatures.*from the headers.*%s" % re.escape(str(tmp_path))):
        list(_abi._header_texts())
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_abi, "GNN_ABI_VERSION", _lib.GNN_ABI_VERSION + 1)
    with pytest.raises(_lib.GnnHipError, match="ABI %d .* ABI %d" % (_lib.GNN_ABI_VERSION + 1, _lib.GNN_ABI_VERSION)):
        _lib.load()
