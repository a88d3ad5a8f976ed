"""Device buffers and streams for the tests that hand the library memory or a
stream the caller owns (gs_load_peers_device, gs_set_stream): hipMalloc,
hipMemcpy, hipFree, hipStreamCreate and hipStreamDestroy of the HIP runtime
the library itself loaded (found in /proc/self/maps, so the pointers and
streams belong to the runtime instance the library uses), as context managers
that release what they made when the block fails.
"""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

H2D, D2H = 1, 2  # hipMemcpyHostToDevice, hipMemcpyDeviceToHost

_hip = None


def hip():
    """The loaded HIP runtime (the library must have been loaded first)."""
    global _hip
    if _hip is None:
        with open("/proc/self/maps") as f:
            path = next((line.split()[-1] for line in f if "libamdhip64" in line), None)
        if path is None:
            raise OSError("no HIP runtime in this process: load libgossip_hip.so first")
        L = C.CDLL(path)
        L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.hipFree.argtypes = [C.c_void_p]
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        L.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        L.hipStreamDestroy.argtypes = [C.c_void_p]
        _hip = L
    return _hip


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: hipError {rc}")


@contextlib.contextmanager
def device_copy(*arrays):
    """Device copies of the host arrays; yields their addresses (ints) in
    order, and frees every one of them on the way out."""
    L, bufs = hip(), []
    try:
        for a in arrays:
            a = np.ascontiguousarray(a)
            d = C.c_void_p()
            _ok(L.hipMalloc(C.byref(d), max(a.nbytes, 1)), "hipMalloc")
            bufs.append(d)
            if a.nbytes:
                _ok(L.hipMemcpy(d, a.ctypes.data, a.nbytes, H2D), "hipMemcpy")
        yield [int(d.value) for d in bufs]
    finally:
        for d in bufs:
            L.hipFree(d)


def read_back(ptr, shape, dtype):
    """A device buffer's contents as a host array."""
    out = np.zeros(shape, dtype=dtype)
    if out.nbytes:
        _ok(hip().hipMemcpy(out.ctypes.data, C.c_void_p(ptr), out.nbytes, D2H), "hipMemcpy")
    return out


@contextlib.contextmanager
def stream():
    """A stream the caller owns; yields its handle (an int)."""
    L, s = hip(), C.c_void_p()
    _ok(L.hipStreamCreate(C.byref(s)), "hipStreamCreate")
    try:
        yield int(s.value)
    finally:
        L.hipStreamDestroy(s)
