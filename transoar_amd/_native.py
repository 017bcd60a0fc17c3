"""The one ctypes binding of the C ABI: every library is bound from its public header.

``bind("tokens", abi=7)`` loads libtransoar_tokens.so and sets restype / argtypes of every function that
include/transoar_tokens.h declares.  The .hip sources include the same header, so the compiler has checked the
signatures read here; no module writes one by hand.  ``launch`` is the one call path of the stream-ordered entry points.

There is deliberately NO fallback: if a gfx950 library is missing or does
not export the ABI, importing its binder raises.  A missing build must never
turn into a silently slower (or CPU) path.
"""
import contextlib
import ctypes
import os
import re

# torch bundles its own libamdhip64.so.7 / libhsa-runtime64; it has to be in the
# process BEFORE a library is dlopen'ed, so that both resolve to the same
# HIP runtime (loading /opt/rocm's copy first leaves torch and the kernels on
# two different runtimes: "no ROCm-capable device is detected").
import torch

_PKG = os.path.dirname(os.path.abspath(__file__))
_INCLUDE = os.path.join(os.path.dirname(_PKG), "include")

F32, F64, BF16, F16 = 0, 1, 2, 3
FORCE_GENERIC = 1
ABI_VERSION = 7


class NativeLibraryError(ImportError):
    pass


# the closed set of value types the headers use; any pointer parameter is a c_void_p (a device or host address)
_CTYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "unsigned": ctypes.c_uint, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_SYMBOL = r"\btransoar_[a-z_0-9]+"
_PROTOTYPE = re.compile(r"([\w\s*]+?)(" + _SYMBOL + r")\s*\(([^()]*)\)\s*;")


def _ctype(decl, where, is_return=False):
    words = decl.replace("*", " * ").split()
    if is_return and words == ["const", "char", "*"]:
        return ctypes.c_char_p
    if is_return and words == ["void"]:
        return None
    if "*" in words and not is_return:
        return ctypes.c_void_p
    words = [w for w in words if w != "const"]
    if not is_return and len(words) > 1:
        words.pop()                          # the parameter's name
    if " ".join(words) not in _CTYPES:
        raise NativeLibraryError("%s: type '%s' is not one the binding knows" % (where, decl.strip()))
    return _CTYPES[" ".join(words)]


def parse_header(text, header="<header>"):
    """C header text -> {function name: (restype, argtypes)} of every ``ret transoar_xxx(params);`` it declares."""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for ret, name, params in _PROTOTYPE.findall(text):
        where = "%s: %s" % (header, name)
        params = [] if params.strip() == "void" else params.split(",")
        protos[name] = (_ctype(ret, where, is_return=True), [_ctype(p, where) for p in params])
    if len(protos) != len(set(re.findall(_SYMBOL + r"\s*\(", text))):        # no prototype is skipped silently
        raise NativeLibraryError("%s: a transoar_ function is declared in a form the binding cannot read" % header)
    return protos


def bind(name, abi=None, header=None):
    """Load libtransoar_<name>.so and give every function of include/transoar_<name>.h its restype and argtypes;
    with `abi`, transoar_<name>_abi_version() must return it."""
    path = os.path.join(_PKG, "libtransoar_%s.so" % name)
    header = header or os.path.join(_INCLUDE, "transoar_%s.h" % name)
    if not os.path.exists(path):
        raise NativeLibraryError("%s is not built: run `python transoar_amd/_build.py` in the repository root; "
                                 "there is no fallback implementation." % path)
    if not os.path.exists(header):
        raise NativeLibraryError("%s, the header %s is bound from, is missing" % (header, path))
    with open(header) as f:
        protos = parse_header(f.read(), header)
    lib = ctypes.CDLL(path)
    for fn, (restype, argtypes) in protos.items():
        try:
            getattr(lib, fn).restype = restype
        except AttributeError:
            raise NativeLibraryError("%s does not export %s, which %s declares: rebuild" % (path, fn, header))
        getattr(lib, fn).argtypes = argtypes
    if abi is not None:
        got = getattr(lib, "transoar_%s_abi_version" % name)()
        if got != abi:
            raise NativeLibraryError("%s has ABI version %d, expected %d: rebuild" % (path, got, abi))
    return lib


lib = bind("msda3d", abi=ABI_VERSION)
LIB_PATH = os.path.join(_PKG, "libtransoar_msda3d.so")


def check(code, what):
    if code != 0:
        raise RuntimeError("%s failed: %s (code %d)" % (
            what, lib.transoar_msda3d_strerror(code).decode(), code))


def ptr(t):
    return None if t is None else t.data_ptr()


_NO_SWITCH = contextlib.nullcontext()


def launch(fn, like, *args, ok=()):
    """fn(*args, stream) on like's device and its current stream.  -> the return code when it is 0 or one of `ok`
    (codes the caller handles itself); any other code raises."""
    # like is almost always on the current device: no device guard to pay for then (a few microseconds per launch,
    # hundreds of launches per eager step)
    same = like.device.index == torch.cuda.current_device()
    with _NO_SWITCH if same else torch.cuda.device(like.device):
        rc = fn(*args, torch.cuda.current_stream().cuda_stream)
    if rc != 0 and rc not in ok:
        if fn.__name__.startswith("transoar_msda3d_"):          # the library with a strerror
            check(rc, fn.__name__)
        raise RuntimeError("%s failed with code %d" % (fn.__name__, rc))
    return rc


PROF_KINDS = ("fwd", "bwd_query", "cell_count", "scan", "cell_fill", "pull", "fwd_generic", "bwd_generic",
              "value_tile", "value_cells")


def profile_enable(on):
    lib.transoar_msda3d_profile_enable(1 if on else 0)


def profile_read():
    """-> {kind: (total_ms, launches)} for the kernels recorded since the last read."""
    ms = (ctypes.c_double * len(PROF_KINDS))()
    n = (ctypes.c_long * len(PROF_KINDS))()
    check(lib.transoar_msda3d_profile_read(ms, n), "transoar_msda3d_profile_read")
    return {k: (ms[i], n[i]) for i, k in enumerate(PROF_KINDS)}
