"""The two kinds of array a mirror call takes, and what differs between them — nothing else does.

A numpy array goes to the synchronous `*_host` form of an entry pair and comes back as numpy (`HOST`); a torch tensor is device memory
and goes to the asynchronous device form on a stream (`device_kind`).  A kind allocates the outputs, turns an array into the C argument,
checks an input and makes the call, so that a method of the mirror is written once: checks, one output dict, one call, return.
dtypes are named as strings for both: "float64", "int32", "uint8", "uint32", "int16".
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check

_CTYPE = {np.dtype(n): t for n, t in (("float64", C.c_double), ("int32", C.c_int32), ("uint8", C.c_uint8), ("uint32", C.c_uint32), ("int16", C.c_int16))}
_POINTER = {d: C.POINTER(t) for d, t in _CTYPE.items()}
_ONE = {d: t * 1 for d, t in _CTYPE.items()}


def _torch():
    import torch  # deferred: importing the package must not need a GPU

    return torch


def _stream_handle(stream):
    if stream is None:
        return C.c_void_p(_torch().cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


def _fits(shape, pattern):
    """shape against a pattern: a tuple with None for any extent, or an int = that many elements in any shape (-1: any number)"""
    if not isinstance(pattern, tuple):
        return pattern < 0 or int(np.prod(shape)) == pattern
    if len(shape) != len(pattern):
        return False
    for s, p in zip(shape, pattern):  # (a loop, not all() over a generator: the planner's per-vertex calls come through here)
        if p is not None and p != s:
            return False
    return True


class _Host:
    """numpy arrays and the `*_host` forms"""

    def empty(self, shape, dtype):
        return np.empty(shape, dtype=dtype)

    def zeros(self, shape, dtype):
        return np.zeros(shape, dtype=dtype)

    def full(self, shape, dtype, value):
        return np.full(shape, value, dtype=dtype)

    def copy_of(self, a):
        return a.copy()

    def arg(self, a, empty_is_null=False):
        """what a POINTER(<a's type>) parameter takes: a one-element ctypes array on a's own buffer (it keeps `a` alive, and costs a quarter
        of ndarray.ctypes), or the typed pointer itself where the buffer cannot be exported so — no elements, read-only"""
        if a is None or (empty_is_null and a.size == 0):
            return None
        try:
            return _ONE[a.dtype].from_buffer(a)
        except (TypeError, ValueError, BufferError):
            return a.ctypes.data_as(_POINTER[a.dtype])

    def expect(self, a, dtype, shape, what):
        """converts to a contiguous array of that dtype, then checks the shape; an element count flattens"""
        a = np.ascontiguousarray(a, dtype=dtype)
        if not _fits(a.shape, shape):
            raise ValueError("%s: expected %s of shape %s, got %s" % (what, dtype, shape, a.shape))
        return a if isinstance(shape, tuple) else a.reshape(-1)

    def call(self, device_entry, host_entry, *args, stream=None):
        check(getattr(_lib.lib(), host_entry)(*args), host_entry)


class _Device:
    """torch tensors on `device` and the device forms, asynchronous on a stream"""

    def __init__(self, device):
        torch = _torch()
        self.device = device
        self._new = (torch.empty, torch.zeros, torch.full)
        # torch has no arithmetic on uint32: an int32 tensor holds the same bits
        self._dtype = {n: getattr(torch, "int32" if n == "uint32" else n) for n in ("float64", "int32", "uint8", "uint32", "int16")}

    def empty(self, shape, dtype):
        return self._new[0](shape, dtype=self._dtype[dtype], device=self.device)

    def zeros(self, shape, dtype):
        return self._new[1](shape, dtype=self._dtype[dtype], device=self.device)

    def full(self, shape, dtype, value):
        return self._new[2](shape, value, dtype=self._dtype[dtype], device=self.device)

    def copy_of(self, a):
        return a.clone()

    def arg(self, a, empty_is_null=False):
        if a is None or (empty_is_null and a.numel() == 0):
            return None
        return a.data_ptr()

    def expect(self, a, dtype, shape, what):
        """never copies: the tensor as it is, or ValueError"""
        if not (getattr(a, "is_cuda", False) and a.dtype == self._dtype[dtype] and a.is_contiguous() and _fits(a.shape, shape)):
            raise ValueError("%s: expected a contiguous %s tensor of shape %s on the device" % (what, dtype, shape))
        return a

    def call(self, device_entry, host_entry, *args, stream=None):
        check(getattr(_lib.lib(), device_entry)(*args, _stream_handle(stream)), device_entry)


HOST = _Host()
_DEVICES = {}


def device_kind(device):
    """the kind of a torch device (one object per device, made on first use)"""
    kind = _DEVICES.get(device)
    if kind is None:
        kind = _DEVICES[device] = _Device(device)
    return kind


def kind_of(a):
    """the kind an argument selects: a numpy array the host's, anything else is taken as a tensor — the kind of its device"""
    return HOST if isinstance(a, np.ndarray) else device_kind(a.device)


def kind_on(ctx, host):
    """for a call without an array argument: `HOST`, or the kind of the context's device"""
    return HOST if host else device_kind(_torch().device("cuda", ctx.device))
