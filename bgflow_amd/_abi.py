"""The C ABI as include/bgflow_amd.h declares it, parsed once: the linker's export list (build.py) and the ctypes signatures
(_lib.py) both come from here.  No torch, nothing but the standard library."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bgflow_amd.h")

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
            "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}


def abi_signatures(header=HEADER, text=None):
    """the C-ABI prototypes of include/bgflow_amd.h (or of the header ``text``) as ``name -> (restype, [argtypes])`` in ctypes terms:
    every pointer parameter is c_void_p, a ``const char*`` return c_char_p, the fixed-width scalars their ctypes twins.  Anything
    else -- an unknown type, a prototype that does not end in ``);`` -- is an error naming the prototype, never a guess."""
    if text is None:
        with open(header) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", "", text, flags=re.S)

    def scalar(decl, name, named):
        tok = [t for t in decl.split() if t != "const"]
        if "[" in decl:                        # an array parameter is a pointer in the ABI: not written that way in this header
            tok = []
        if named and len(tok) > 1:
            tok = tok[:-1]                     # the parameter's own name
        if len(tok) != 1 or tok[0] not in _SCALARS:
            raise ValueError(f"include/bgflow_amd.h: {name}: no ctypes type for '{decl.strip()}'")
        return _SCALARS[tok[0]]

    sigs = {}
    for m in re.finditer(r"^([A-Za-z_][\w \t\*]*?)\b(bgk_\w+)\s*\(", text, flags=re.M):
        ret, name = m.group(1), m.group(2)
        body = re.compile(r"([^(){};]*)\)\s*;").match(text, m.end())
        if body is None:
            raise ValueError(f"include/bgflow_amd.h: {name}: cannot split the prototype")
        if name in sigs:
            raise ValueError(f"include/bgflow_amd.h: {name} is declared twice")
        params = body.group(1).split(",") if body.group(1).strip() not in ("", "void") else []
        if "*" in ret:
            if "".join(ret.split()) != "constchar*":
                raise ValueError(f"include/bgflow_amd.h: {name}: no ctypes type for the return type '{ret.strip()}'")
            res = ctypes.c_char_p
        else:
            res = scalar(ret, name, named=False)
        sigs[name] = (res, [ctypes.c_void_p if "*" in p else scalar(p, name, named=True) for p in params])
    return sigs
