"""hdn_amd._lib.SIGNATURES against include/hdn_hip.h, for every entry point: the same names, and for each name the same return class, the same number of
arguments and the same class at every position (pointer, int, long long, float, double).  ctypes converts by the binding, not by the header, so a wrong
entry is a silently mis-passed argument; this holds the hand-kept mirror to the declarations without an exemption list.  No GPU, no library load."""
import ctypes
import os
import re

from hdn_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hdn_hip.h")
_POINTER_BASES = (ctypes._Pointer, ctypes.c_void_p, ctypes.c_char_p)
_SCALARS = {ctypes.c_int: "int", ctypes.c_uint: "int", ctypes.c_longlong: "long long", ctypes.c_float: "float", ctypes.c_double: "double"}


def _header():
    with open(HEADER) as f:
        text = f.read()
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)


def _c_class(decl):
    """The class of one C parameter or return type (`const float* x`, `long long n`, `unsigned int* count`, ...)."""
    if "*" in decl:
        return "pointer"
    words = [w for w in re.findall(r"[A-Za-z_]\w*", decl) if w != "const"]
    for cls, spelling in (("long long", ["long", "long"]), ("double", ["double"]), ("float", ["float"]), ("int", ["unsigned", "int"]), ("int", ["int"]),
                          ("int", ["unsigned"])):
        if words[:len(spelling)] == spelling:
            return cls
    raise AssertionError(f"unknown C type in {decl!r}")


def _ctypes_class(t):
    if t in _SCALARS:
        return _SCALARS[t]
    assert isinstance(t, type) and issubclass(t, _POINTER_BASES), f"unknown ctypes type {t!r}"
    return "pointer"


def _declarations():
    """name -> (return class, [argument classes]) of every hdn_* function the header declares (a declaration may span lines)."""
    out = {}
    for ret, name, params in re.findall(r"\b(int|long long|const char\s*\*)\s*(hdn_\w+)\s*\(([^()]*)\)\s*;", _header()):
        assert name not in out, f"{name} is declared twice"
        params = " ".join(params.split())
        out[name] = (_c_class(ret), [] if params in ("", "void") else [_c_class(p) for p in params.split(",")])
    return out


def test_the_parser_sees_every_declaration():
    """Every `hdn_xxx(` of the comment-free header is one parsed declaration: none is lost to a return type or a layout the pattern does not know."""
    names = re.findall(r"\b(hdn_\w+)\s*\(", _header())
    assert sorted(names) == sorted(_declarations()) and len(names) == len(set(names)) > 100


def test_binding_and_header_declare_the_same_names():
    decl = _declarations()
    assert sorted(set(decl) - set(_lib.SIGNATURES)) == [], "declared in the header, not bound"
    assert sorted(set(_lib.SIGNATURES) - set(decl)) == [], "bound, not declared in the header"


def test_every_binding_has_the_declared_return_and_argument_classes():
    decl = _declarations()
    wrong = []
    for name, (res, args) in _lib.SIGNATURES.items():
        d_res, d_args = decl[name]
        if _ctypes_class(res) != d_res:
            wrong.append(f"{name}: returns {d_res}, bound as {res.__name__}")
        if len(args) != len(d_args):
            wrong.append(f"{name}: {len(d_args)} arguments declared, {len(args)} bound")
            continue
        for i, (a, d) in enumerate(zip(args, d_args)):
            if _ctypes_class(a) != d:
                wrong.append(f"{name}: argument {i} is {d}, bound as {a.__name__}")
    assert wrong == []


def test_abi_version_of_the_header_is_the_bindings():
    m = re.search(r"^#define HDN_ABI_VERSION (\d+)\s*$", _header(), flags=re.M)
    assert m is not None and int(m.group(1)) == _lib.ABI_VERSION
