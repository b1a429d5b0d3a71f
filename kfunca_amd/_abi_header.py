"""Reader of include/kfunca_hip.h: the header is the one statement of the device C ABI, and hip_abi derives its ctypes signatures,
Structures, constants and export list from what read() returns instead of re-stating them.

This is no C parser. It reads the subset the header is written in - comments, preprocessor lines, anonymous enums with explicit values,
`typedef struct kf_x {...} kf_x;` of scalars, pointers and arrays, and prototypes `ret name(params);` - and raises HeaderError, with the
offending text, on anything else: a declaration that was skipped silently would be a call with default (C int) arguments.
"""
from __future__ import annotations

import ctypes as C
import re
from typing import NamedTuple

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float,
           "double": C.c_double}
# [const] base [*[const]]... [name] [[bound]]...: a parameter, or (without a name) a return type
_DECL = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?\s*((?:\[\s*\w*\s*\])*)")
_FIELD = re.compile(r"(\*?)\s*(\w+)\s*((?:\[\s*\w+\s*\])*)")


class HeaderError(ValueError):
    pass


class Header(NamedTuple):
    prototypes: dict  # {name: (restype, [argtypes])}
    structs: dict     # {name: C.Structure subclass}; its _fields_ is the ordered (field, ctype) list
    constants: dict   # {name: int}: every enumerator and every integer #define
    exports: list     # sorted prototype names


def _int(text, what):
    try:
        return int(text, 0)
    except ValueError:
        raise HeaderError(f"{what} is not an integer literal: {text!r}") from None


def _ctype(text, structs, where):
    """The ctypes type of a parameter or return type. Pointers: char -> c_char_p, a kf_* struct -> POINTER(its Structure), every other
    one -> c_void_p (the header cannot say whether a float * is a device address or a host out-parameter; c_void_p takes both)."""
    m = _DECL.fullmatch(text.strip())
    if not m:
        raise HeaderError(f"cannot read {text.strip()!r} in {where}")
    base, stars, _, dims = m.groups()
    if base not in SCALARS and base not in structs and base not in ("void", "char"):
        raise HeaderError(f"unknown type {base!r} in {text.strip()!r} of {where}")
    depth = stars.count("*") + dims.count("[")
    if depth == 0:
        if base not in SCALARS:
            raise HeaderError(f"{base!r} passed by value in {text.strip()!r} of {where}")
        return SCALARS[base]
    if depth == 1 and base == "char":
        return C.c_char_p
    if depth == 1 and base in structs:
        return C.POINTER(structs[base])
    return C.c_void_p


def _fields(body, constants, where):
    """The (field, ctype) list of a struct body: pointers are c_void_p, `t a[N][M]` is (t * M) * N."""
    scalars = dict(SCALARS, char=C.c_char)
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(.*)", stmt, re.S)
        if not m or (m.group(1) not in scalars and m.group(1) != "void"):
            raise HeaderError(f"unknown type in field {stmt!r} of {where}")
        for decl in m.group(2).split(","):
            d = _FIELD.fullmatch(decl.strip())
            if not d or not (d.group(1) or m.group(1) in scalars):
                raise HeaderError(f"cannot read field {decl.strip()!r} ({stmt!r}) of {where}")
            ct = C.c_void_p if d.group(1) else scalars[m.group(1)]
            for bound in reversed(re.findall(r"\w+", d.group(3))):
                if not bound.isdigit() and bound not in constants:
                    raise HeaderError(f"unknown array bound {bound!r} in field {decl.strip()!r} of {where}")
                ct = ct * (int(bound) if bound.isdigit() else constants[bound])
            out.append((d.group(2), ct))
    return out


def read(text: str) -> Header:
    constants, structs, prototypes = {}, {}, {}
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        m = re.fullmatch(r"\s*#\s*define\s+(\w+)\s+(\S.*?)\s*", line)   # (a #define without a value is the include guard)
        if m:
            constants[m.group(1)] = _int(m.group(2), f"#define {m.group(1)}")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    m = re.fullmatch(r'\s*extern\s+"C"\s*\{(.*)\}\s*', text, re.S)
    text = m.group(1) if m else text

    def enum(m):
        for e in filter(None, (s.strip() for s in m.group(1).split(","))):
            name, eq, value = e.partition("=")
            if not eq or not re.fullmatch(r"\w+", name.strip()):
                raise HeaderError(f"enumerator without an explicit value: {e!r}")
            constants[name.strip()] = _int(value.strip(), f"enumerator {name.strip()}")
        return ""

    def struct(m):
        tag, body, name = m.groups()
        if tag != name:
            raise HeaderError(f"typedef struct {tag} is named {name}")
        structs[name] = type(name, (C.Structure,), {"_fields_": _fields(body, constants, f"struct {name}")})
        return ""

    text = re.sub(r"\benum\s*\{([^{}]*)\}\s*;", enum, text)
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\(([^()]*)\)", stmt, re.S)
        if not m or not m.group(1).strip() or not m.group(3).strip():
            raise HeaderError(f"not a prototype `ret name(params)`: {' '.join(stmt.split())!r}")
        ret, name, params = m.groups()
        params = [] if params.strip() == "void" else params.split(",")
        prototypes[name] = (_ctype(ret, structs, f"the return type of {name}"), [_ctype(p, structs, name) for p in params])
    return Header(prototypes, structs, constants, sorted(prototypes))
