"""The host kind of closed_chain_motion_planner_amd/_arrays.py alone: what every numpy form of the mirror rests on.  No library, no device."""
import ctypes as C

import numpy as np
import pytest

from closed_chain_motion_planner_amd._arrays import HOST, kind_of


def test_expect_converts_to_contiguous_float64():
    for given in ([[0.0] * 14, [1.0] * 14], np.ones((2, 14), dtype=np.float32), np.ones((2, 28))[:, ::2]):
        a = HOST.expect(given, "float64", (None, 14), "rows")
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (2, 14) and a.flags["C_CONTIGUOUS"]
    same = np.zeros((3, 14))
    assert HOST.expect(same, "float64", (None, 14), "rows") is same  # what already fits is not copied


def test_expect_rejects_a_wrong_shape():
    F = 3
    with pytest.raises(ValueError):
        HOST.expect(np.zeros((3, 13)), "float64", (None, 14), "rows")
    with pytest.raises(ValueError):
        HOST.expect(np.zeros(F + 1, dtype=np.int32), "int32", (F,), "path_len")
    with pytest.raises(ValueError):
        HOST.expect(np.zeros((F, 1), dtype=np.int32), "int32", (F,), "path_len")
    with pytest.raises(ValueError):
        HOST.expect(np.zeros(13), "float64", 14, "joints")


def test_expect_an_element_count_flattens():
    a = HOST.expect(np.arange(6, dtype=np.int64).reshape(2, 3), "int32", 6, "flags")
    assert a.dtype == np.int32 and a.shape == (6,) and a.tolist() == [0, 1, 2, 3, 4, 5]
    assert HOST.expect([[1, 2], [3, 4]], "int32", -1, "uv").shape == (4,)


def test_arg_none_and_empty():
    assert HOST.arg(None) is None and HOST.arg(None, empty_is_null=True) is None
    empty = np.zeros((0, 14))
    assert isinstance(HOST.arg(empty), C.POINTER(C.c_double))  # a pointer, not NULL
    assert HOST.arg(empty, empty_is_null=True) is None
    assert HOST.arg(np.zeros((1, 14)), empty_is_null=True) is not None


def _address(p):
    return C.cast(p, C.c_void_p).value


@pytest.mark.parametrize("dtype, ctype", [("int32", C.c_int32), ("uint8", C.c_uint8), ("float64", C.c_double), ("uint32", C.c_uint32), ("int16", C.c_int16)])
def test_arg_is_what_a_host_signature_takes(dtype, ctype):
    """ctypes' own argument conversion for POINTER(<the array's type>) accepts it, and for no other width; it points at the array's data —
    also for the arrays whose buffer cannot be exported writable (read-only, a view with strides), which go as plain typed pointers"""
    a = np.arange(5).astype(dtype)
    frozen = a.copy()
    frozen.setflags(write=False)
    for arr in (a, frozen, np.arange(10).astype(dtype)[::2]):
        p = HOST.arg(arr)
        assert C.POINTER(ctype).from_param(p) is not None and _address(p) == arr.ctypes.data
        for t in (C.c_int32, C.c_uint8, C.c_double):
            if C.sizeof(t) != C.sizeof(ctype):
                with pytest.raises((TypeError, C.ArgumentError)):
                    C.POINTER(t).from_param(p)
    p = HOST.arg(a)
    del a  # the argument keeps the array alive
    assert C.cast(p, C.POINTER(ctype))[4] == 4


def test_empty_zeros_full_copy_of():
    for dtype in ("float64", "int32", "uint8", "uint32", "int16"):
        e, z, f = HOST.empty((2, 3), dtype), HOST.zeros((2, 3), dtype), HOST.full((2, 3), dtype, 7)
        for a in (e, z, f):
            assert a.dtype == np.dtype(dtype) and a.shape == (2, 3) and a.flags["C_CONTIGUOUS"]
        assert (z == 0).all() and (f == 7).all()
    assert HOST.empty(4, "int32").shape == (4,) and HOST.zeros((0, 14), "float64").size == 0
    assert (HOST.full((2, 4), "int32", -1) == -1).all() and np.isnan(HOST.full((1, 2, 8), "float64", float("nan"))).all()
    a = np.arange(4.0)
    b = HOST.copy_of(a)
    b[0] = 9.0
    assert a[0] == 0.0 and b.dtype == a.dtype and b.shape == a.shape


def test_an_ndarray_selects_the_host_kind():
    assert kind_of(np.zeros(3)) is HOST and kind_of(np.zeros((0, 8), dtype=np.float32)) is HOST
