"""ctypes binding of librendernet_hip.so (include/rendernet_hip.h).

The product path has NO fallback: if the HIP library is missing or a symbol is absent, importing
this module's `lib()` raises.  Tensors are torch CUDA(=HIP) tensors; only their device pointers
and the current stream cross the ABI.

The header is the one statement of the ABI: `SIGNATURES` and the `RN_*` integers are parsed from it at
import (no library and no device needed).  To add an entry:
  1. declare it in include/rendernet_hip.h, with a `#define RN_X <integer>` for each constant it names;
  2. define it `extern "C"` in rendernet_amd/csrc/;
  3. call it: `lib().rn_x(...)`, its return code through `check`.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RN_HIP_LIBRARY") or os.path.join(_HERE, "lib", "librendernet_hip.so")   # override: A/B builds

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "rendernet_hip.h")


class RenderNetHipError(RuntimeError):
    pass


_c_int, _c_vp, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float
_SCALARS = {"int": _c_int, "float": _c_f, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "unsigned long long": ctypes.c_uint64}
_DECLARATION = re.compile(r"([A-Za-z_][\w\s*]*?)\b(rn_\w+)\s*\(([^()]*)\)\s*;")
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)(.*)$", re.M)
_INTEGER = re.compile(r"-?(0[xX][0-9a-fA-F]+|0|[1-9][0-9]*)")
_SHIFT = re.compile(r"\(\s*([0-9]+)\s*<<\s*([0-9]+)\s*\)")


def _ctype(decl, entry, is_return=False):
    """The ctypes type of one parameter (`const float* x`, `int B`, `long long`) or of a return type."""
    words = decl.replace("*", " * ").split()
    if is_return and words == ["const", "char", "*"]:
        return ctypes.c_char_p
    words = [w for w in words if w != "const"]
    if "*" in words and not is_return:
        return _c_vp                       # every pointer, host or device, crosses the ABI as an address
    if not is_return and " ".join(words) not in _SCALARS and re.fullmatch(r"[A-Za-z_]\w*", words[-1] if words else ""):
        words = words[:-1]                 # the parameter's name
    if " ".join(words) in _SCALARS:
        return _SCALARS[" ".join(words)]
    raise RenderNetHipError("header entry %s: no ctypes type for `%s`" % (entry, " ".join(decl.split())))


def parse_header(text):
    """(signatures, constants, skipped) of a C header: name -> (restype, [argtypes]) of every `<ret> rn_name(<params>);`,
    name -> value of every `#define RN_X <integer>`, and the names of the #defines that are something else."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, skipped = {}, []
    for name, body in _DEFINE.findall(text):
        body, shift = body.strip(), _SHIFT.fullmatch(body.strip())
        if name.startswith("RN_") and _INTEGER.fullmatch(body):
            constants[name] = int(body, 0)
        elif name.startswith("RN_") and shift:
            constants[name] = int(shift.group(1)) << int(shift.group(2))
        else:
            skipped.append(name)
    code = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    signatures, at = {}, set()
    for m in _DECLARATION.finditer(code):
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        signatures[name] = (_ctype(ret, name, is_return=True), [_ctype(p, name) for p in params])
        at.add(m.start(2))
    for m in re.finditer(r"\brn_\w+", code):
        if m.start() not in at:
            raise RenderNetHipError("header entry %s: not of the form `<ret> rn_name(<params>);`" % m.group())
    return signatures, constants, skipped


with open(HEADER_PATH) as _f:
    SIGNATURES, _CONSTANTS = parse_header(_f.read())[:2]         # name -> (restype, argtypes) of every entry; the RN_* integers
globals().update(_CONSTANTS)

_lib = None
_F32 = [None]          # torch.float32, filled in by lib() (torch is imported lazily)


def lib():
    """Load (once) and return the ctypes library.  Raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RenderNetHipError(
                "librendernet_hip.so not found at %s -- build it with `python -m rendernet_amd.build` "
                "(there is no CPU fallback for the render path)" % LIB_PATH)
        import torch  # first: the library must bind to the HIP runtime torch ships, not a second copy
        _F32[0] = torch.float32
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().rn_last_error()
        raise RenderNetHipError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


def ivec(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def ptr(t):
    """Device pointer of a contiguous float32 CUDA tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RenderNetHipError("expected a CUDA/HIP tensor, got device %s" % t.device)
    if _F32[0] is None:
        lib()
    if t.dtype is not _F32[0] or not t.is_contiguous():
        raise RenderNetHipError("expected a contiguous float32 tensor")
    return ctypes.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
