"""ctypes binding of libbgflow_amd.so (the C ABI declared in include/bgflow_amd.h).

The product path has NO fallback: if the library is missing, cannot be loaded, or a kernel is
asked to run on a non-HIP tensor, a RuntimeError is raised.
"""
import ctypes
import os

import torch

from ._abi import abi_signatures

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BGK_LIB") or os.path.join(_HERE, "libbgflow_amd.so")   # BGK_LIB: A/B builds (tools/)
_lib = None

# name -> (restype, [argtypes]) of every prototype of include/bgflow_amd.h, parsed from the header itself (the parse that also
# writes the library's export list): there is no second, hand-kept copy of the ABI
_SIGNATURES = abi_signatures()
ABI_SYMBOLS = tuple(_SIGNATURES)


def lib():
    """Load libbgflow_amd.so (built by ``python -m bgflow_amd.build`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: the MI355X kernels are not built. Run `python -m bgflow_amd.build` "
                "(hipcc, gfx950). bgflow_amd has no CPU fallback.")
        try:
            handle = ctypes.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError(f"cannot load {LIB_PATH}: {e}. bgflow_amd has no CPU fallback.") from e
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)   # AttributeError = ABI mismatch, fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        msg = lib().bgk_last_error().decode(errors="replace")
        if status == -1 and "Minimal bin" in msg:
            raise ValueError(msg)
        raise RuntimeError(f"{what} failed (status {status}): {msg}")


def require_hip(*tensors):
    """Every operand of a kernel must be an f32 tensor on a HIP device (no CPU path)."""
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "bgflow_amd kernels run on MI355X (HIP) tensors only; got a tensor on "
                f"'{t.device}'. There is no CPU fallback in this package.")
        if t.dtype not in (torch.float32, torch.int32):
            raise RuntimeError(f"bgflow_amd kernels are float32; got {t.dtype}")


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def cond_segments(parts):
    """host tables (device pointers, row strides, widths) of 1..3 conditioning tensors for the *_mc entry points; the returned
    tuple keeps the ctypes arrays and the (possibly re-laid-out) tensors alive for the duration of the call"""
    rows = [rowmajor(t) for t in parts]
    n = len(rows)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _ in rows])
    lds = (ctypes.c_int64 * n)(*[ld for _, ld in rows])
    widths = (ctypes.c_int32 * n)(*[t.shape[1] for t, _ in rows])
    return ptrs, lds, widths, n, rows


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def rowmajor(t):
    """Return a 2-d view with unit column stride (copy only if needed) and its row stride."""
    assert t.dim() == 2, "expected [batch, features]"
    if t.stride(1) != 1 and t.shape[1] > 1:
        t = t.contiguous()
    if t.shape[1] == 1 and t.stride(1) != 1:
        t = t.contiguous()
    ld = t.stride(0) if t.shape[0] > 1 else t.shape[1]
    if t.shape[0] > 1 and ld < t.shape[1]:   # broadcast / expanded rows
        t = t.contiguous()
        ld = t.stride(0)
    return t, ld
