"""The C ABI of libgnn_hip.so, read once at import from the four headers under include/: the signature tables (one per
header, name -> (restype, argtypes)), a ctypes.Structure per `typedef struct ... gnn_x_y_t` (as GnnXY) and every integer
`#define GNN_*` and enumerator under its header name.  No torch, no library: _lib.py re-exports all of it.

The type rule, stated here and nowhere else:
  - int, int32_t, int64_t, size_t, float, double: the ctypes scalar; a `const char *` return: c_char_p;
  - a pointer to a scalar or to void: c_void_p (device pointers and the stream travel as integers);
  - a pointer to a const struct: POINTER(Struct), a host struct passed by reference; to a non-const struct: c_void_p
    (the sizes_out arguments, which point into device memory);
  - TYPED_POINTERS: the host scalar pointers that keep their typed form.

The parser is a few regular expressions, not a C front end.  It reads integer #defines, anonymous enums with implicit
values, typedef'd structs and `RET gnn_name(args);` prototypes, and refuses everything else, quoting it: a header that
outgrows it must fail loudly.
"""
import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_void_p

INCLUDE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
HEADERS = (("SIGNATURES", "gnn_hip.h"), ("ITER_SIGNATURES", "gnn_hip_iter.h"), ("FX_SIGNATURES", "gnn_hip_fixed.h"),
           ("FXEV_SIGNATURES", "gnn_hip_fixed_events.h"))          # table name, header; in include order

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
           "float": ctypes.c_float, "double": ctypes.c_double}
TYPED_POINTERS = {("gnn_plan_limits", "out4"): POINTER(ctypes.c_int32),
                  ("gnn_plan_route", "out"): POINTER(ctypes.c_int32),
                  ("gnn_profile_end", "names"): POINTER(c_char_p),
                  ("gnn_profile_end", "ms"): POINTER(ctypes.c_float)}


class GnnHipError(RuntimeError):
    pass


_DEFINE = re.compile(r"#\s*define\s+(GNN_\w+)\s+(?:(-?\d+)|\(\s*(-?\d+)\s*\))")
_SKIPPED = re.compile(r"#\s*(?:ifn?def\s+\w+|endif|include\s*\S+|define\s+\w+)")          # guards and includes
_ENUM = re.compile(r"\s*enum\s*\{([^{}]*)\}\s*;")
_STRUCT = re.compile(r"\s*typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(gnn_\w+)_t\s*;")
_PROTO = re.compile(r"\s*((?:const\s+)?\w+\s*\**)\s*\b(gnn_\w+)\s*\(([^(){}]*)\)\s*;")
_TYPE = re.compile(r"(const\s+)?(\w+)\s*(\**)")
_PARAM = re.compile(r"(const\s+)?(\w+)(?:\s*(\*+)\s*|\s+)(\w+)")
_FIELDS = re.compile(r"(const\s+)?(\w*)(.*)", re.S)          # matches any statement; what follows decides
_DECLARATOR = re.compile(r"(\**)\s*(\w+)\s*(?:\[([^\]]*)\])?")


def read_abi(headers, typed_pointers):
    """[(table name, header text)] in include order -> {name: signature table | Structure class | int}."""
    ns, structs, typed = {}, {}, dict(typed_pointers)

    def publish(name, value):
        if name in ns:
            raise GnnHipError("the headers declare %s twice" % name)
        ns[name] = value

    def ctype(const, base, stars, quote):
        if base in structs:
            if not stars:
                return structs[base]
            return POINTER(structs[base]) if const else c_void_p
        if base in SCALARS or (stars and base in ("void", "char")):
            return c_void_p if stars else SCALARS[base]
        raise GnnHipError("unknown type %r in %r" % (base, quote))

    def array_size(expr, quote):
        py = re.sub(r"[A-Za-z_]\w*", lambda m: str(ns[m[0]]) if isinstance(ns.get(m[0]), int) else "?", expr)
        if not re.fullmatch(r"[\d\s+\-*()]+", py) or "**" in py:
            raise GnnHipError("array size is no integer expression over known constants in %r" % quote)
        return eval(py)        # digits, + - * and parentheses only

    def struct(body, name):
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            const, base, declarators = _FIELDS.fullmatch(stmt).groups()
            for m in (_DECLARATOR.fullmatch(d.strip()) for d in declarators.split(",")):
                if not m:
                    raise GnnHipError("struct %s_t: not a field this binding reads: %r" % (name, stmt))
                t = ctype(const, base, m[1], stmt)
                fields.append((m[2], t if m[3] is None else t * array_size(m[3], stmt)))
        cls = type("".join(p.capitalize() for p in name.split("_")), (ctypes.Structure,), {"_fields_": fields})
        structs[name + "_t"] = cls
        publish(cls.__name__, cls)

    def prototype(ret, name, args, quote):
        argtypes = []
        for arg in [] if args.strip() == "void" else args.split(","):
            m = _PARAM.fullmatch(arg.strip())
            if not m:
                raise GnnHipError("not a parameter this binding reads: %r in %r" % (arg.strip(), quote))
            argtypes.append(typed.pop((name, m[4]), None) or ctype(m[1], m[2], m[3], quote))
        if re.fullmatch(r"const\s+char\s*\*", ret):
            return c_char_p, argtypes
        return ctype(*_TYPE.fullmatch(ret).groups(), quote), argtypes

    for table_name, text in headers:
        table, body = {}, []
        publish(table_name, table)
        for line in re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split("\n"):
            if not line.lstrip().startswith("#"):
                body.append(line)
            elif _DEFINE.fullmatch(line.strip()):
                name, plain, parenthesised = _DEFINE.fullmatch(line.strip()).groups()
                publish(name, int(plain or parenthesised))
            elif not _SKIPPED.fullmatch(line.strip()):
                raise GnnHipError("%s: not a preprocessor line this binding reads: %r" % (table_name, line.strip()))
        text = "\n".join(body)
        m = re.fullmatch(r'(.*?)extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
        text, pos = (m[1] + m[2] if m else text), 0
        while text[pos:].strip():
            if m := _ENUM.match(text, pos):
                for value, name in enumerate(m[1].split(",")):
                    if not re.fullmatch(r"\s*[A-Za-z_]\w*\s*", name):
                        raise GnnHipError("%s: enumerators take implicit values: %r" % (table_name, m[0].strip()))
                    publish(name.strip(), value)
            elif m := _STRUCT.match(text, pos):
                struct(m[1], m[2])
            elif m := _PROTO.match(text, pos):
                if m[2] in table:
                    raise GnnHipError("the headers declare %s twice" % m[2])
                table[m[2]] = prototype(m[1].strip(), m[2], m[3], m[0].strip())
            else:
                raise GnnHipError("%s: what is left is no declaration this binding reads: %r"
                                  % (table_name, text[pos:].strip()[:200]))
            pos = m.end()
    if typed:
        raise GnnHipError("TYPED_POINTERS names what the headers do not declare: %s" % sorted(typed))
    return ns


def _header_texts():
    if not os.path.isdir(INCLUDE_DIR):
        raise GnnHipError("the binding reads its signatures, struct layouts and constants from the headers, and %s "
                          "is missing" % INCLUDE_DIR)
    for table_name, header in HEADERS:
        with open(os.path.join(INCLUDE_DIR, header)) as f:
            yield table_name, f.read()


_declared = read_abi(_header_texts(), TYPED_POINTERS)
globals().update(_declared)
__all__ = ["GnnHipError"] + list(_declared)
