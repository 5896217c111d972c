"""The connection step's C ABI without a device: declarations, exports, what ccmp_ctx_describe says about the two call kinds, and
argument checks that come before any device is touched."""
import ctypes as C
import os
import re

from conftest import ROOT

from closed_chain_motion_planner_amd import _lib

HEADER = open(os.path.join(ROOT, "include", "ccmp.h")).read()


def test_header_declares_the_entry_points_and_call_kinds(ccmp_built):
    for name in ("ccmp_knn_batch", "ccmp_knn_host", "ccmp_connect_batch", "ccmp_connect_host"):
        assert re.search(r"\bint %s\(ccmp_ctx \*ctx," % name, HEADER), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert re.search(r"CCMP_CALL_KNN = 7\b", HEADER) and re.search(r"CCMP_CALL_CONNECT = 8\b", HEADER)
    assert re.search(r"#define CCMP_KNN_MAX_K 16\b", HEADER)
    assert re.search(r"CCMP_KNN_ALL = 0, CCMP_KNN_NOT_SELF = 1, CCMP_KNN_EARLIER = 2", HEADER)
    assert (_lib.CALL_KNN, _lib.CALL_CONNECT, _lib.KNN_MAX_K) == (7, 8, 16)
    assert _lib.lib().ccmp_version() == 600


def _kernel_of(line):
    """the traversal kernel a CCMP_CALL_GEODESIC line names"""
    names = re.findall(r"geodesic_[a-z0-9_]*kernel[a-z_]*", line)
    assert names, line
    return names


def test_describe_names_the_kernels(ccmp_built):
    for n in (1, 5, 4096, 65536):
        knn = _lib.describe(None, _lib.CALL_KNN, n)
        con = _lib.describe(None, _lib.CALL_CONNECT, n)
        few = n <= 8
        for line in (knn, con):
            assert ("knn_few_kernel" in line) == few and ("knn_many_kernel" in line) == (not few), line
            assert ("partitioned form" in line) == few
            assert re.search(r"x \d+ blocks", line) and re.search(r"\d+ partitions of \d+ nodes", line), line
            assert "knn_merge_kernel" in line  # 65536 nodes are more than one partition at every Q
        assert "tiles of 256 nodes" in knn or few
        assert knn.startswith("knn Q=%d " % n) and con.startswith("connect Q=%d " % n)
        # the traversal part: the line of 5 n geodesic edges, kernels included
        geo = _lib.describe(None, _lib.CALL_GEODESIC, 5 * n)
        assert geo in con, (geo, con)
        assert all(name in con for name in _kernel_of(geo))
        assert "connect_gather_kernel" in con and "connect_fix_kernel" in con and "geodesic" not in knn


def test_describe_unknown_kind_and_null_context(ccmp_built):
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    assert L.ccmp_ctx_describe(None, 99, 16, buf, len(buf)) == -1
    assert L.ccmp_ctx_describe(None, 9, 16, buf, len(buf)) == -1
    # the returned length is the whole line's, whatever the buffer holds
    full = _lib.describe(None, _lib.CALL_CONNECT, 4096)
    assert L.ccmp_ctx_describe(None, _lib.CALL_CONNECT, 4096, buf, len(buf)) == len(full) and buf.value.decode() == full[:63]
    one = (C.c_double * 14)()
    idx = (C.c_int32 * 16)()
    P = _lib.CcmpProblem()
    assert L.ccmp_knn_batch(None, one, 1, one, 1, 1, 0, 0, idx, None, None) == -1
    assert L.ccmp_knn_host(None, one, 1, one, 1, 1, 0, 0, idx, None) == -1
    assert L.ccmp_connect_batch(None, C.byref(P), None, 0.0, one, 1, one, 1, 1, 0, 0, 1, 4, 0, idx, None, one, idx, None, None, None, None, None) == -1
    assert L.ccmp_connect_host(None, C.byref(P), None, 0.0, one, 1, one, 1, 1, 0, 0, 1, 4, 0, idx, None, one, idx, None, None, None, None) == -1
