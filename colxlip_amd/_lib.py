"""ctypes binding of libclipx_hip.so (the C ABI declared in include/clipx.h).

The product path has no CPU or PyTorch-eager fallback: if the shared library is
missing, `lib()` raises.  Signatures are parsed from the header so the binding can
never drift from `include/clipx.h`.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libclipx_hip.so")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "clipx.h")

F32, BF16 = 0, 1
ACT_NONE, ACT_GELU, ACT_QUICKGELU = 0, 1, 2

_CTYPES = {
    "int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "size_t": ctypes.c_size_t,
    "uint64_t": ctypes.c_uint64,
}
_lib = None


def header_prototypes(header: str = _HEADER):
    """[(name, restype, [argtypes])] for every function declared in clipx.h."""
    with open(header) as f:
        src = f.read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    protos = []
    for m in re.finditer(r"(const char\*|int|size_t)\s+(clipx_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        argtypes = []
        for a in [x.strip() for x in args.replace("\n", " ").split(",")]:
            if a in ("void", ""):
                continue
            if "*" in a:
                argtypes.append(ctypes.c_void_p)
            else:
                base = a.split()[-2] if len(a.split()) > 1 else a
                argtypes.append(_CTYPES[base])
        restype = {"const char*": ctypes.c_char_p, "int": ctypes.c_int, "size_t": ctypes.c_size_t}[ret]
        protos.append((name, restype, argtypes))
    return protos


def lib_path() -> str:
    return _LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"{_LIB_PATH} is missing: build the HIP extension first "
                "(python -m colxlip_amd.build).  There is no CPU fallback for the hot path.")
        L = ctypes.CDLL(_LIB_PATH)
        for name, restype, argtypes in header_prototypes():
            fn = getattr(L, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = L
    return _lib


class ClipxError(RuntimeError):
    pass


def check(rc: int):
    if rc != 0:
        raise ClipxError(f"clipx error {rc}: {lib().clipx_last_error().decode()}")
