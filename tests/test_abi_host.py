"""CPU: the ctypes binding (mac-network_amd/_lib.py: TABLE and the Structure classes) held to include/macx.h.

Prototypes: every `ret macx_name(args);` of the header is parsed and compared with TABLE -- arity, and the class of the return type
and of every parameter (pointer | int | uint32 | size_t | float), position by position.
Layouts: a C program generated from the header's `typedef struct`s is compiled with the host C compiler and prints sizeof and every
field's offsetof / sizeof; the output is compared with the ctypes twins.
Neither loads libmacx.so: the table is plain data."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macx.h")

C_CLASS = {"int": "int", "int32_t": "int", "uint32_t": "uint32", "size_t": "size_t", "float": "float"}
CTYPES_CLASS = {C.c_int: "int", C.c_int32: "int", C.c_uint32: "uint32", C.c_size_t: "size_t", C.c_float: "float"}
C_FIELD = {"int32_t": "int32", "uint32_t": "uint32", "uint64_t": "uint64", "float": "float"}
CTYPES_FIELD = {C.c_int32: "int32", C.c_uint32: "uint32", C.c_uint64: "uint64", C.c_float: "float", C.c_void_p: "pointer"}


def header_code():
    """macx.h without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def c_class(decl):
    """class of a C return type or parameter declaration (`const macx_opts*`, `int step`, `size_t`): unknown types raise"""
    if "*" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in C_CLASS, "cannot classify the C type in %r" % decl
    return C_CLASS[words[0]]


def ctypes_class(t):
    if t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer)):
        return "pointer"
    assert t in CTYPES_CLASS, "cannot classify the ctypes type %r" % (t,)
    return CTYPES_CLASS[t]


def header_prototypes():
    """{name: (class of the return type, [class of each parameter])} of every function the header declares"""
    code = re.sub(r"\b(struct\s+\w+|enum)\s*\{[^{}]*\}", " ", header_code())          # no struct / enum bodies
    code = code.replace('extern "C" {', " ")
    protos = {}
    for stmt in code.split(";"):
        m = re.match(r"\s*([\w\s\*]+?)\b(macx_[a-z_0-9]+)\s*\(([^()]*)\)\s*$", stmt, flags=re.S)
        if m is None:
            assert not re.search(r"\bmacx_[a-z_0-9]+\s*\(", stmt), "unparsed declaration: %r" % stmt.strip()
            continue
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        assert name not in protos, "%s declared twice" % name
        params = [] if params in ("", "void") else params.split(",")
        protos[name] = (c_class(ret), [c_class(p) for p in params])
    return protos


def prototype_mismatches(table):
    """lines `name: what differs` between the header's prototypes and a {name: (restype, argtypes)} table"""
    protos, out = header_prototypes(), []
    for name in sorted(set(protos) & set(table)):
        (ret, params), (restype, argtypes) = protos[name], table[name]
        if argtypes is None:
            out.append("%s: no argtypes" % name)
            continue
        if ctypes_class(restype) != ret:
            out.append("%s: returns %s, the binding says %s" % (name, ret, ctypes_class(restype)))
        if len(argtypes) != len(params):
            out.append("%s: %d parameters, the binding has %d" % (name, len(params), len(argtypes)))
            continue
        for i, (p, a) in enumerate(zip(params, argtypes)):
            if ctypes_class(a) != p:
                out.append("%s: parameter %d is %s, the binding says %s" % (name, i, p, ctypes_class(a)))
    return out


def test_prototypes_match_header(macx):
    table = macx._lib.TABLE
    assert macx._lib.EXPORTS == tuple(table)
    protos = header_prototypes()
    assert set(protos) == set(macx._lib.EXPORTS)
    # ... and the parser skipped nothing: the looser name search of test_host.py finds the same set
    loose = set(re.findall(r"\b(macx_[a-z_0-9]+)\s*\(", open(HEADER).read())) - {"macx_opts", "macx_shapes"}
    assert set(protos) == loose
    assert prototype_mismatches(table) == []
    # the header's order, so that a new export has one obvious place
    order = {n: i for i, n in enumerate(re.findall(r"\b(macx_[a-z_0-9]+)\s*\(", header_code()))}
    assert sorted(table, key=order.__getitem__) == list(table)
    assert table["macx_workspace_bytes"][0] is C.c_size_t      # (once reset to c_int by a catch-all loop: 2 GiB came back negative)


def header_structs():
    """{struct name: [(field, kind)]} of every `typedef struct` of the header, fields in order; kind: int32 | uint32 | uint64 |
    float | pointer, with `[n]` behind it for an array"""
    structs = {}
    for name, body, alias in re.findall(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", header_code()):
        assert name == alias and name not in structs
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)\s*(\[\d+\])?$", first.strip())
            assert m is not None, "%s: cannot parse the field declaration %r" % (name, decl)
            base, star = m.group(1), m.group(2)
            assert star or base in C_FIELD, "%s: cannot classify the field type in %r" % (name, decl)
            kind = "pointer" if star else C_FIELD[base]
            fields.append((m.group(3), kind + (m.group(4) or "")))
            for d in more:                      # `int32_t a, b;`: further declarators of the same base type
                m = re.match(r"(\*?)\s*(\w+)\s*(\[\d+\])?$", d.strip())
                assert m is not None and not m.group(1) and not star, "%s: cannot parse %r" % (name, decl)
                fields.append((m.group(2), kind + (m.group(3) or "")))
        structs[name] = fields
    return structs


def ctypes_kind(t):
    if isinstance(t, type) and issubclass(t, C.Array):
        return "%s[%d]" % (ctypes_kind(t._type_), t._length_)
    assert t in CTYPES_FIELD, "cannot classify the ctypes field type %r" % (t,)
    return CTYPES_FIELD[t]


def ctypes_structs(lib):
    """{header name: Structure class} of every ctypes Structure mac-network_amd/_lib.py defines (MacxOutShapes <-> macx_out_shapes)"""
    out = {}
    for cls in vars(lib).values():
        if isinstance(cls, type) and issubclass(cls, C.Structure) and cls.__module__ == lib.__name__:
            name = re.sub(r"(?<!^)([A-Z])", r"_\1", cls.__name__).lower()
            assert name not in out
            out[name] = cls
    return out


def compiled_layouts(structs, tmp_path, cc):
    """{`struct` / `struct.field`: (offset, size)} as the host C compiler lays the header's structs out"""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "macx.h"', "int main(void) {"]
    for name, fields in structs.items():
        lines.append('  printf("%s 0 %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in fields:
            lines.append('  printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layouts.c", tmp_path / "layouts"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout
    return {key: (int(off), int(size)) for key, off, size in (line.split() for line in out.splitlines())}


def test_struct_layouts_match_header(macx, tmp_path):
    lib = macx._lib
    structs, twins = header_structs(), ctypes_structs(lib)
    assert structs and set(structs) == set(twins)              # every header struct has exactly one ctypes twin, and the reverse
    for name, fields in structs.items():                       # names in order, and what kind of thing each field is
        assert [(f, ctypes_kind(t)) for f, t in twins[name]._fields_] == fields, name
    assert tuple(f for f, _ in structs["macx_params"]) == lib.PARAM_FIELDS == tuple(f for f, _ in structs["macx_param_grads"])
    cc = os.environ.get("CC") or next((c for c in ("cc", "gcc", "clang") if shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler on this machine: sizes and offsets not compared")
    want = compiled_layouts(structs, tmp_path, cc)
    assert len(want) == len(structs) + sum(len(f) for f in structs.values())
    for name, fields in structs.items():
        cls = twins[name]
        assert (0, C.sizeof(cls)) == want[name], "sizeof(%s)" % name
        for f, _ in fields:
            d = getattr(cls, f)
            assert (d.offset, d.size) == want[name + "." + f], "%s.%s (offset, size)" % (name, f)
