"""ctypes binding of libhosrender.so (the C ABI declared in include/hosrender.h).

There is deliberately no fallback: if the shared library has not been built, or a tensor handed
to an op is not a contiguous fp32 HIP tensor, this module raises.  The product path never
routes through oracle/ or any CPU implementation.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
from ctypes import c_char_p, c_float, c_int, c_int64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HOS_LIB_PATH", os.path.join(_HERE, "lib", "libhosrender.so"))   # override: timing experiments only


class HosLibraryError(RuntimeError):
    pass


_P, _I, _F, _L = c_void_p, c_int, c_float, c_int64
_SCALARS = {"int": _I, "int32_t": _I, "unsigned int": _I, "float": _F, "int64_t": _L, "long long": _L}
HEADER = os.path.join(os.path.dirname(_HERE), "include", "hosrender.h")


@functools.lru_cache(maxsize=None)
def parse_header(path: str) -> dict:
    """{name: (restype, [argtypes])} of every `ret hos_name(params);` a C header declares.  The header is the only description of
    the ABI: a pointer is c_void_p (`const char*` c_char_p), a `typedef void* X;` makes X one, the integer and float scalars map by
    width; anything else -- a statement that is no declaration, a type not listed here -- raises instead of defaulting to int."""
    try:
        text = open(path).read()
    except OSError as e:
        raise HosLibraryError(f"cannot read {path}: {e} (the prototypes of the C ABI are derived from it)") from e
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r'^\s*#.*$|extern\s+"C"\s*\{|\}', " ", text, flags=re.M)
    handles = set()

    def ctype(spelling, where):
        base = " ".join(spelling.replace("*", " ").replace("const", " ").split())
        if "*" in spelling:
            return c_char_p if (base, spelling.count("*")) == ("char", 1) else _P
        if base in handles:
            return _P
        if base not in _SCALARS:
            raise HosLibraryError(f"{path}: no ctypes mapping for `{spelling.strip()}` in `{where}`")
        return _SCALARS[base]

    out = {}
    for stmt in (" ".join(x.split()) for x in text.split(";")):
        m = re.fullmatch(r"typedef void ?\* ?(\w+)", stmt)
        if m:
            handles.add(m.group(1))
        elif stmt:
            m = re.fullmatch(r"([\w\s\*]+?)\b(hos_[a-z0-9_]+) ?\(([^()]*)\)", stmt)
            if not m:
                raise HosLibraryError(f"{path}: cannot parse `{stmt}`")
            params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
            out[m.group(2)] = (ctype(m.group(1), stmt), [ctype(re.sub(r"\w+\s*$", "", p), stmt) for p in params])
    return out


def abi_version(path: str) -> int:
    m = re.search(r"^\s*#\s*define\s+HOS_ABI_VERSION\s+(\d+)", open(path).read(), flags=re.M)
    if not m:
        raise HosLibraryError(f"{path} does not define HOS_ABI_VERSION")
    return int(m.group(1))


def open_library(lib_path: str, header: str, versioned: bool = True) -> ctypes.CDLL:
    """Load `lib_path` with the prototypes `header` declares.  Raises HosLibraryError if either file is missing, a declared entry
    point is not exported, or (versioned) hos_version() is not the header's HOS_ABI_VERSION."""
    protos = parse_header(header)
    if not os.path.exists(lib_path):
        raise HosLibraryError(
            f"{lib_path} not found: build it with `make` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "hosnerf_amd has no CPU fallback.")
    try:
        lib = ctypes.CDLL(lib_path)
    except OSError as e:  # pragma: no cover
        raise HosLibraryError(f"cannot load {lib_path}: {e}") from e
    for name, (restype, argtypes) in protos.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HosLibraryError(f"{lib_path} does not export {name}; rebuild the library") from e
        fn.argtypes, fn.restype = argtypes, restype
    if versioned:
        want = abi_version(header)
        if lib.hos_version() != want:
            raise HosLibraryError(f"{lib_path} is ABI revision {lib.hos_version()}, {header} declares {want}: rebuild the library")
    return lib


def argtypes_of(header: str) -> dict:
    """name -> argtypes as `header` declares them; empty if it cannot be parsed, which is load()'s error to report, not import's."""
    try:
        return {name: argtypes for name, (_, argtypes) in parse_header(header).items()}
    except HosLibraryError:
        return {}


PROTOTYPES = argtypes_of(HEADER)
_lib = None


def load() -> ctypes.CDLL:
    """Load the library once; raise HosLibraryError with a build hint if it is missing or of another ABI revision."""
    global _lib
    if _lib is None:
        _lib = open_library(LIB_PATH, HEADER)
    return _lib


def check(code: int, what: str):
    if code != 0:
        msg = load().hos_error_string(int(code))
        raise HosLibraryError(f"{what} failed with code {code}: {msg.decode() if msg else '?'}")


def require_gpu():
    if not torch.cuda.is_available():
        raise HosLibraryError("no HIP device visible: hosnerf_amd ops run on MI355X only (no CPU fallback)")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t, dtype=torch.float32) -> int:
    """Device pointer of a contiguous HIP tensor of the expected dtype (None -> NULL)."""
    if t is None:
        return 0
    if not isinstance(t, torch.Tensor):
        raise HosLibraryError(f"expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise HosLibraryError("hosnerf_amd ops take HIP (device='cuda') tensors only -- there is no CPU path")
    if t.dtype != dtype:
        raise HosLibraryError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise HosLibraryError("expected a contiguous tensor")
    return t.data_ptr()


def call(name: str, *args):
    """Invoke an entry point on the current stream (appended as the last argument) and check it."""
    lib = load()
    code = getattr(lib, name)(*args, stream_ptr())
    check(code, name)
