"""Reader of ``include/pgca_hip.h``, the one place where the C ABI is declared.

The header is parsed once at import (no compiler, no shared library) into four tables:

* ``PROTOTYPES``  entry name -> ``Prototype``: return type and parameters as C type strings and names, with the
                  ctypes ``restype`` / ``argtypes`` they map to
* ``STRUCTS``     ``pgca_*`` struct name -> ``ctypes.Structure`` whose ``_fields_`` are the members in order
* ``CONSTANTS``   every ``#define PGCA_* <integer>`` and every enumerator -> int
* ``SCALARS``     the C scalar types in use -> ctypes type (the fixed mapping)

Any data pointer maps to ``c_void_p``, ``const pgca_<struct>*`` to ``POINTER`` of the struct, ``const char*`` to
``c_char_p``.  A ``pgca_*(`` in the header that is not one of the parsed prototypes, or a type outside the mapping, is
an ``ImportError`` here: a declaration this reader cannot read does not go missing quietly.
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List, NamedTuple, Tuple

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pgca_hip.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float}
_POINTEES = set(SCALARS) | {"void", "uint8_t"}   # what a data pointer may point at


class Prototype(NamedTuple):
    ret: str                          # C return type
    params: List[Tuple[str, str]]     # (C type, name), e.g. ("const float*", "x")
    restype: type
    argtypes: list


def _ctype(t: str):
    if t in SCALARS:
        return SCALARS[t]
    if t == "const char*":
        return C.c_char_p
    m = re.fullmatch(r"(?:const )?(\w+)\*", t)
    if m and m.group(1) in STRUCTS:
        return C.POINTER(STRUCTS[m.group(1)])
    if m and m.group(1) in _POINTEES:
        return C.c_void_p
    raise ImportError(f"{HEADER}: no ctypes mapping for the C type '{t}'")


def _declaration(text: str) -> Tuple[str, List[str]]:
    """``"const float* x"`` -> ``("const float*", ["x"])``; ``"int32_t M, N, K"`` -> ``("int32_t", ["M", "N", "K"])``."""
    m = re.fullmatch(r"(.+?[\s*])\s*(\w+(?:\s*,\s*\w+)*)", " ".join(text.split()))
    if not m:
        raise ImportError(f"{HEADER}: cannot read the declaration '{text}'")
    return re.sub(r"\s*\*", "*", m.group(1).strip()), re.split(r"\s*,\s*", m.group(2))


with open(HEADER, "r", encoding="utf-8") as _f:
    TEXT = re.sub(r"/\*.*?\*/|//[^\n]*", "", _f.read(), flags=re.S)   # the header without its comments

CONSTANTS: Dict[str, int] = {k: int(v) for k, v in re.findall(r"^#define\s+(PGCA_\w+)\s+(-?\d+)\s*$", TEXT, flags=re.M)}
for _body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", TEXT):
    for _item in filter(None, (" ".join(i.split()) for i in _body.split(","))):
        _m = re.fullmatch(r"(PGCA_\w+) = (-?\d+)", _item)
        if not _m:
            raise ImportError(f"{HEADER}: cannot read the enumerator '{_item}'")
        CONSTANTS[_m.group(1)] = int(_m.group(2))

STRUCTS: Dict[str, type] = {}
for _name, _body in re.findall(r"typedef\s+struct\s+(pgca_\w+)\s*\{(.*?)\}\s*\1\s*;", TEXT, flags=re.S):
    _fields = []
    for _decl in filter(None, (d.strip() for d in _body.split(";"))):
        _t, _names = _declaration(_decl)
        _fields += [(n, _ctype(_t)) for n in _names]
    STRUCTS[_name] = type(_name, (C.Structure,), {"_fields_": _fields})

PROTOTYPES: Dict[str, Prototype] = {}
for _ret, _name, _args in re.findall(r"^([\w \t*]+?)\s*\b(pgca_\w+)\s*\(([^)]*)\)\s*;", TEXT, flags=re.M):
    _ret = re.sub(r"\s*\*", "*", " ".join(_ret.split()))
    _params = [(t, n[0]) for t, n in (_declaration(a) for a in _args.split(",") if a.strip() != "void")]
    PROTOTYPES[_name] = Prototype(_ret, _params, _ctype(_ret), [_ctype(t) for t, _ in _params])

_unread = set(re.findall(r"\b(pgca_\w+)\s*\(", TEXT)) - set(PROTOTYPES)
if _unread or not PROTOTYPES or not STRUCTS:
    raise ImportError(f"{HEADER}: declarations this reader cannot parse: {sorted(_unread) or 'none found at all'}")
