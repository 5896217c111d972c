"""The roadmap store's C ABI without a device: declarations, exports, the two call kinds of ccmp_ctx_describe, and what the entry
points answer where no context can exist (there is no host path: a store needs a context, and a context needs a device)."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

from closed_chain_motion_planner_amd import _lib

HEADER = open(os.path.join(ROOT, "include", "ccmp.h")).read()
ENTRIES = ("create", "destroy", "size", "reserve", "append", "set_joints", "truncate", "read", "knn", "connect", "append_host", "set_joints_host", "read_host",
           "knn_host", "connect_host")


def test_header_declares_the_entry_points_and_call_kinds(ccmp_built):
    for e in ENTRIES:
        name = "ccmp_roadmap_" + e
        assert re.search(r"\b%s\((const )?ccmp_(roadmap \*rm|ctx \*ctx)[,)]" % name, HEADER), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert re.search(r"\bdouble ccmp_pose_distance\(const double a\[8\], const double b\[8\]\);", HEADER)
    assert re.search(r"\bvoid ccmp_pose_from_t_wo\(const double t_wo\[12\], double pose\[8\]\);", HEADER)
    assert "ccmp_pose_distance" in _lib.EXPORTS and "ccmp_pose_from_t_wo" in _lib.EXPORTS
    assert re.search(r"CCMP_CALL_ROADMAP_KNN = 10\b", HEADER) and re.search(r"CCMP_CALL_ROADMAP_CONNECT = 11\b", HEADER)
    assert re.search(r"CCMP_METRIC_JOINT = 0, CCMP_METRIC_OBJECT = 1\b", HEADER)
    assert (_lib.CALL_ROADMAP_KNN, _lib.CALL_ROADMAP_CONNECT, _lib.METRIC_JOINT, _lib.METRIC_OBJECT) == (10, 11, 0, 1)
    # kind 9 stays unknown (tests/test_knn_connect_cabi.py pins it), and so is the first kind behind the new ones
    buf = C.create_string_buffer(64)
    assert _lib.lib().ccmp_ctx_describe(None, 9, 16, buf, len(buf)) == -1 and _lib.lib().ccmp_ctx_describe(None, 12, 16, buf, len(buf)) == -1
    assert "there is no device-resident, appendable node store" not in HEADER
    assert _lib.lib().ccmp_version() == 600  # an addition: the version stays


def test_existing_call_kinds_keep_their_text(ccmp_built):
    """kinds 7 and 8 describe the joint kernels as before"""
    knn = _lib.describe(None, _lib.CALL_KNN, 300)
    assert knn.startswith("knn Q=300 ") and "knn_many_kernel" in knn and "pose" not in knn and "tiles of 256 nodes" in knn


def test_describe_prints_a_plan(ccmp_built):
    for n in (1, 8, 9, 4096, 16384):
        knn = _lib.describe(None, _lib.CALL_ROADMAP_KNN, n)
        con = _lib.describe(None, _lib.CALL_ROADMAP_CONNECT, n)
        few = n <= 8
        for line in (knn, con):
            assert ("knn_pose_few_kernel" in line) == few and ("knn_pose_many_kernel" in line) == (not few), line
            assert re.search(r"x \d+ blocks", line) and re.search(r"\d+ partitions of \d+ poses", line), line
            assert "knn_merge_kernel" in line and "object metric" in line
            assert "min_partition=1024" in line
        assert few or "tiles of 512 poses" in knn
        assert knn.startswith("roadmap_knn Q=%d" % n) and con.startswith("roadmap_connect Q=%d" % n)
        geo = _lib.describe(None, _lib.CALL_GEODESIC, 5 * n)
        assert geo in con and "geodesic" not in knn
        assert "pose_from_joints_kernel" in con and "connect_gather_kernel" in con and "connect_fix_kernel" in con
    buf = C.create_string_buffer(32)
    full = _lib.describe(None, _lib.CALL_ROADMAP_KNN, 64)
    assert _lib.lib().ccmp_ctx_describe(None, _lib.CALL_ROADMAP_KNN, 64, buf, len(buf)) == len(full) and buf.value.decode() == full[:31]


def test_device_entries_answer_enodev_here(ccmp_built):
    """A store lives on a context's device.  On a machine without one none can be created and every entry point says why —
    CCMP_ENODEV, never a host path; with a device a NULL store is an argument error (CCMP_EINVAL)."""
    import torch

    L = _lib.lib()
    want = -1 if torch.cuda.is_available() else -5  # CCMP_EINVAL / CCMP_ENODEV
    assert L.ccmp_roadmap_create(None, 4) is None
    one = (C.c_double * 14)()
    idx = (C.c_int32 * 16)()
    first = C.c_size_t(7)
    P = _lib.CcmpProblem()
    assert L.ccmp_roadmap_size(None) == 0
    L.ccmp_roadmap_destroy(None)
    assert L.ccmp_roadmap_reserve(None, 10) == want
    assert L.ccmp_roadmap_append(None, C.byref(P), one, None, 1, C.byref(first), None) == want
    assert L.ccmp_roadmap_append_host(None, C.byref(P), one, None, 1, C.byref(first)) == want
    assert L.ccmp_roadmap_set_joints(None, 0, one, None) == want and L.ccmp_roadmap_set_joints_host(None, 0, one) == want
    assert L.ccmp_roadmap_truncate(None, 0) == want
    assert L.ccmp_roadmap_read(None, 0, 1, one, None, None) == want and L.ccmp_roadmap_read_host(None, 0, 1, one, None) == want
    assert L.ccmp_roadmap_knn(None, 1, one, 1, 1, 0, 0, idx, None, None) == want
    assert L.ccmp_roadmap_knn_host(None, 1, one, 1, 1, 0, 0, idx, None) == want
    assert L.ccmp_roadmap_connect(None, C.byref(P), None, 0.0, 1, one, None, 1, 1, 0, 0, 1, 4, 0, idx, None, one, idx, None, None, None, None, None) == want
    assert L.ccmp_roadmap_connect_host(None, C.byref(P), None, 0.0, 1, one, None, 1, 1, 0, 0, 1, 4, 0, idx, None, one, idx, None, None, None, None) == want
    if not torch.cuda.is_available():  # and the context itself: the Python mirror has nothing to stand on
        from closed_chain_motion_planner_amd import CcmpError, Context

        with pytest.raises(CcmpError) as e:
            Context(0)
        assert e.value.code == -5
