"""ctypes binding of libdagr_hip.so (the C ABI declared in include/dagr_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails, a
RuntimeError is raised (the reference raises RuntimeError through AT_ASSERTM for bad inputs,
``src/dagr/graph/ev_graph.cu:9-12``).  PyTorch only supplies device memory and streams here; every
argument crossing this boundary is a raw pointer or an integer.
"""
import ctypes
import os

from ._header import Header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libdagr_hip.so")

HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "dagr_hip.h")

c_void_p = ctypes.c_void_p


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise RuntimeError(f"dagr_amd: {HEADER_PATH} not found -- the ctypes binding is derived from the C header, "
                           "which ships with the repository next to the package.")
    with open(HEADER_PATH) as f:
        return Header(f.read())


# include/dagr_hip.h is the single source of truth of the ABI: it is read once, here, at import, and the structures, the
# enumerators and the argument types of every entry point below are what it declares (_header.py has the type mapping).
# tests/test_binding_cpu.py checks the derived layouts against the C compiler's and the names against the built library.
_HEADER = _read_header()
ENUMS = _HEADER.enums                   # enumerator -> int, e.g. ENUMS["DAGR_FLOPS_CONV"]
STRUCTS = _HEADER.structs               # C name -> ctypes.Structure, e.g. STRUCTS["dagr_pool_desc"] is PoolDesc
SIGNATURES = _HEADER.functions          # name -> (restype, argtypes)
DEFINES = _HEADER.defines               # integer #defines, e.g. DEFINES["DAGR_TRACK_MAX_TRACKS"]
# PoolDesc, GraphDesc, HeadScale, ConvJob, L0Inputs, AsyncUpdateArgs, FlopsModule, AugParams: dagr_<x_y> is class XY
globals().update({cls.__name__: cls for cls in STRUCTS.values()})

_lib = None


def lib():
    """Load libdagr_hip.so once; fail loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"dagr_amd: {LIB_PATH} not found -- build it with `make` (or __graft_entry__.build()). "
                "There is no CPU fallback for the event-graph hot path.")
        handle = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().dagr_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"libdagr_hip {what} failed (status {rc}): {msg}")


def ptr(t):
    """Raw device/host pointer of a torch tensor (or None)."""
    return None if t is None else c_void_p(t.data_ptr())


def cur_stream(device=None):
    """hipStream_t of torch's current stream, as void*."""
    import torch
    return c_void_p(torch.cuda.current_stream(device).cuda_stream)
