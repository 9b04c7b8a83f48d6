"""ctypes loader for libcq_halo2.so.  Fails loudly if the HIP extension is missing: there is
no CPU fallback anywhere in this package."""
from __future__ import annotations

import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libcq_halo2.so")
HEADER = os.path.join(HERE, "..", "include", "cq_halo2.h")

_lib = None


class CqError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"cq_halo2 error {code}: {msg}")
        self.code = code


def load() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} not found: build it with `python -m sha2_on_cq_halo2_amd.build` "
                "(hipcc, gfx950).  This package has no CPU fallback."
            )
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def _header_text() -> str:
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)      # comments
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)        # preprocessor lines
    return src


def header_symbols():
    """Every function name declared in include/cq_halo2.h."""
    return sorted(p.name for p in header_prototypes())


class Prototype:
    """One `extern "C"` prototype of include/cq_halo2.h: C return type and parameter types as written there."""

    def __init__(self, name, ret, params):
        self.name, self.ret, self.params = name, ret, params

    def __repr__(self):
        return f"{self.ret} {self.name}({', '.join(self.params)})"


def header_prototypes():
    """Parses the header (the ABI's single source of truth): the ctypes signatures below are DERIVED from it, so the
    Python binding cannot drift from the C declarations -- and the compiler holds the definitions in csrc/capi*.hip to
    the same declarations (they include the header under `extern "C"`)."""
    src = _header_text()
    src = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", "", src, flags=re.S)  # struct bodies
    src = re.sub(r"typedef[^;{]*;", "", src)                                       # opaque / function-pointer typedefs
    src = src.replace('extern "C" {', "")
    out = []
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(cq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        plist = [] if params in ("", "void") else [re.sub(r"\s+", " ", p.strip()) for p in params.split(",")]
        out.append(Prototype(name, re.sub(r"\s+", " ", ret), plist))
    return out


class Declarations:
    """Everything of include/cq_halo2.h that is not a prototype, in header order, as written there."""

    def __init__(self, consts, opaque, structs, fnptrs):
        self.consts = consts    # [(name, value text)] of every `#define CQ_<NAME> <integer>`
        self.opaque = opaque    # [name] of every `typedef struct cq_x cq_x;`
        self.structs = structs  # [(name, [field declaration])]
        self.fnptrs = fnptrs    # [(name, return type, [parameter declaration])]


_declarations = None


def header_declarations() -> Declarations:
    """The header's constants, opaque handles, structs and function-pointer typedefs: the one parse that the ctypes
    binding (`struct`, `callback`, `constants`) and tools/gen_rust_ffi.py both read."""
    global _declarations
    if _declarations is None:
        raw, text = open(HEADER).read(), _header_text()
        consts = [(m.group(1), m.group(2)) for m in re.finditer(r"^#define\s+(CQ_[A-Z0-9_]+)\s+\(?(-?\d+)u?\)?", raw, flags=re.M)
                  if m.group(1) != "CQ_HALO2_H"]
        opaque = re.findall(r"typedef\s+struct\s+(cq_\w+)\s+\1\s*;", text)
        structs = [(m.group(2), [f.strip() for f in m.group(1).split(";") if f.strip()])
                   for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(cq_\w+)\s*;", text, flags=re.S)]
        fnptrs = [(m.group(2), m.group(1).strip(), [p.strip() for p in m.group(3).split(",")])
                  for m in re.finditer(r"typedef\s+([\w\s\*]+?)\(\s*\*\s*(cq_\w+)\s*\)\s*\(([^()]*)\)\s*;", text)]
        _declarations = Declarations(consts, opaque, structs, fnptrs)
    return _declarations


def header_fnptr_typedefs():
    """Names of the function-pointer typedefs (callbacks crossing the ABI)."""
    return {name for name, _, _ in header_declarations().fnptrs}


def constants():
    """{name: value} of every `#define CQ_<NAME> <integer>` of the header."""
    return {name: int(value) for name, value in header_declarations().consts}


_SCALARS = {"int": C.c_int, "uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64,
            "size_t": C.c_size_t, "double": C.c_double, "uint8_t": C.c_uint8}
_types = {}  # struct(), callback(): name -> ctypes class


def _ctype_of_decl(decl: str):
    """(ctypes class, name) of one struct field or callback parameter, `[const] T [const] {* [const]} [name] [ [N] ]`:
    scalars and fixed arrays keep their width; `T*` is POINTER(T) for a scalar or struct T, so Python can index it; void*,
    callbacks and pointers to pointers are machine addresses."""
    m = re.search(r"\[\s*(\d+)\s*\]\s*$", decl)
    toks = [t for t in re.findall(r"\*|\w+", decl[: m.start()] if m else decl) if t != "const"]
    base, stars = toks[0], toks.count("*")
    name = toks[-1] if len(toks) > 1 + stars else None
    decls = header_declarations()
    if base in _SCALARS:
        ty = _SCALARS[base]
    elif base in dict(decls.structs):
        ty = struct(base)
    elif (base in header_fnptr_typedefs() and not stars) or (stars and (base == "void" or base in decls.opaque)):
        ty, stars = C.c_void_p, max(stars - 1, 0)
    else:
        raise TypeError(f"cq_halo2.h: type not understood in {decl!r}")
    if stars:
        ty = C.POINTER(ty if stars == 1 else C.c_void_p)
    return (ty * int(m.group(1)) if m else ty), name


def struct(name: str):
    """The ctypes.Structure of the header's struct `name`: its fields in header order."""
    if name not in _types:
        fields = [_ctype_of_decl(f)[::-1] for f in dict(header_declarations().structs)[name]]
        _types[name] = type(name, (C.Structure,), {"_fields_": fields})
    return _types[name]


def callback(name: str):
    """The CFUNCTYPE of the header's function-pointer typedef `name`."""
    if name not in _types:
        ret, params = {n: (r, p) for n, r, p in header_declarations().fnptrs}[name]
        _types[name] = C.CFUNCTYPE(ctype_of_return(ret), *[_ctype_of_decl(p)[0] for p in params if p != "void"])
    return _types[name]


def ctype_of_param(decl: str, fnptrs) -> object:
    """ctypes class of one C parameter declaration: every pointer, array parameter and callback is a machine address
    (c_void_p accepts ints, None, byref(), arrays and CFUNCTYPE instances); scalars keep their width."""
    if "*" in decl or "[" in decl:
        return C.c_void_p
    words = [w for w in decl.replace("const", " ").split() if w]
    ty = words[0] if len(words) == 1 else " ".join(words[:-1])  # drop the parameter name
    if ty in fnptrs:
        return C.c_void_p
    if ty not in _SCALARS:
        raise TypeError(f"cq_halo2.h: parameter type not understood: {decl!r}")
    return _SCALARS[ty]


def ctype_of_return(ret: str):
    ret = ret.replace("const", " ").strip()
    ret = re.sub(r"\s+", " ", ret).replace(" *", "*")
    if ret == "void":
        return None
    if ret == "char*":
        return C.c_char_p
    if ret.endswith("*"):
        return C.c_void_p
    if ret not in _SCALARS:
        raise TypeError(f"cq_halo2.h: return type not understood: {ret!r}")
    return _SCALARS[ret]


def signatures():
    """{name: (restype, [argtypes])} for every prototype of the header."""
    fnptrs = header_fnptr_typedefs()
    return {p.name: (ctype_of_return(p.ret), [ctype_of_param(d, fnptrs) for d in p.params]) for p in header_prototypes()}


def _declare(lib):
    for name, (restype, argtypes) in signatures().items():
        fn = getattr(lib, name)  # AttributeError: the header declares a symbol the library does not export
        fn.restype = restype
        fn.argtypes = argtypes
