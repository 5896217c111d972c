"""The object-checker C ABI without a device: declarations, exports, the new call kind of ccmp_ctx_describe, what the device and host
forms answer where no context can exist, and the argument checks (the *_ref forms are the host path: tests/test_object_ref.py)."""
import ctypes as C
import os
import re

import numpy as np
from conftest import ROOT
from object_cases import box_mesh, workspace

from closed_chain_motion_planner_amd import _lib
from closed_chain_motion_planner_amd.object import boxes_from

HEADER = open(os.path.join(ROOT, "include", "ccmp.h")).read()
ENTRIES = ("ccmp_pose_interpolate", "ccmp_object_create", "ccmp_object_destroy", "ccmp_object_num_triangles", "ccmp_object_valid_batch",
           "ccmp_object_valid_host", "ccmp_object_valid_ref", "ccmp_object_propose_batch", "ccmp_object_propose_host", "ccmp_object_propose_ref")
EINVAL, ENODEV = -1, -5
_dp = C.POINTER(C.c_double)


def test_header_declares_the_entry_points(ccmp_built):
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, HEADER), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert re.search(r"CCMP_CALL_OBJECT_PROPOSE = 15\b", HEADER) and _lib.CALL_OBJECT_PROPOSE == 15
    assert _lib.lib().ccmp_version() == 600  # an addition: the version stays
    assert (_lib.OBJECT_MAX_TRIANGLES, _lib.OBJECT_MAX_ATTEMPTS, _lib.MAX_BOXES) == tuple(
        int(re.search(r"#define CCMP_%s (\d+)" % n, HEADER).group(1)) for n in ("OBJECT_MAX_TRIANGLES", "OBJECT_MAX_ATTEMPTS", "MAX_BOXES"))
    assert _lib.OBJECT_MAX_TRIANGLES == 16384 and _lib.OBJECT_MAX_ATTEMPTS == 16


def test_describe_answers_kind_15_and_not_14(ccmp_built):
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    for kind in (9, 12, 14, 16, 99):
        assert L.ccmp_ctx_describe(None, kind, 16, buf, len(buf)) == -1, kind
    for n in (1, 4096):
        line = _lib.describe(None, _lib.CALL_OBJECT_PROPOSE, n)
        assert line.startswith("object_propose G=%d " % n) and "object_propose_kernel x %d blocks of 256 lanes" % n in line and "object_valid_kernel" in line
    full = _lib.describe(None, _lib.CALL_OBJECT_PROPOSE, 64)
    assert L.ccmp_ctx_describe(None, _lib.CALL_OBJECT_PROPOSE, 64, buf, len(buf)) == len(full) and buf.value.decode() == full[:63]


def _args():
    tri = np.ascontiguousarray(box_mesh(0.05, 0.05, 0.05))
    bx = boxes_from(workspace())
    pose = np.array([[0.65, 0.0, 1.5, 0, 0, 0, 1, 0]], dtype=np.float64)
    return tri, bx, pose


def test_device_and_host_forms_answer_enodev_here(ccmp_built):
    """There is no quiet host path behind the device entry points: without a device they say CCMP_ENODEV (with one, a NULL context is an
    argument error)."""
    import torch

    L = _lib.lib()
    want = EINVAL if torch.cuda.is_available() else ENODEV
    tri, bx, pose = _args()
    valid, mask, which, out = (C.c_uint8 * 2)(), (C.c_uint32 * 2)(), (C.c_int32 * 2)(), (C.c_double * 16)()
    lo, hi = (C.c_double * 3)(-9, -9, -9), (C.c_double * 3)(9, 9, 9)
    p = pose.ctypes.data_as(_dp)
    h = C.c_void_p()
    assert L.ccmp_object_create(None, tri.ctypes.data_as(_dp), len(tri), bx, len(bx), C.byref(h)) == want and not h
    assert L.ccmp_object_valid_batch(None, None, p, 1, 0.0, valid, mask, None) == want
    assert L.ccmp_object_valid_host(None, None, p, 1, 0.0, valid, mask) == want
    assert L.ccmp_object_propose_batch(None, None, p, p, 0, 1, 0.3, 0.2, lo, hi, 2, 0, 0, 0.0, out, which, None, None, None) == want
    assert L.ccmp_object_propose_host(None, None, p, p, 0, 1, 0.3, 0.2, lo, hi, 2, 0, 0, 0.0, out, which, None, None) == want
    assert L.ccmp_object_num_triangles(None) == 0
    L.ccmp_object_destroy(None)


def test_argument_checks(ccmp_built):
    """Every check runs before anything else: the *_ref forms and ccmp_object_create (whose argument checks come before its context) say
    CCMP_EINVAL for M = 0, M over the cap, 9 boxes, a NaN vertex, attempts 0 and 17, a sigma over the rotation limit."""
    L = _lib.lib()
    tri, bx, pose = _args()
    valid, which, out = (C.c_uint8 * 2)(), (C.c_int32 * 2)(), (C.c_double * 16)()
    lo, hi = (C.c_double * 3)(-9, -9, -9), (C.c_double * 3)(9, 9, 9)
    p, t = pose.ctypes.data_as(_dp), tri.ctypes.data_as(_dp)

    def valid_ref(tri_p, M, boxes, nb, inflate=0.0):
        return L.ccmp_object_valid_ref(tri_p, M, boxes, nb, p, 1, inflate, 1, valid, None)

    def create(tri_p, M, boxes, nb):
        h = C.c_void_p()
        rc = L.ccmp_object_create(None, tri_p, M, boxes, nb, C.byref(h))
        assert not h
        return rc

    def propose_ref(attempts=2, sigma=0.2, to_stride=0, t_=0.3):
        return L.ccmp_object_propose_ref(t, len(tri), bx, len(bx), p, p, to_stride, 1, t_, sigma, lo, hi, attempts, 0, 0, 0.0, out, which, None, None)

    assert valid_ref(t, len(tri), bx, len(bx)) == 0 and propose_ref() == 0  # the well-formed call
    big = np.zeros((_lib.OBJECT_MAX_TRIANGLES + 1, 9))
    nine = boxes_from(workspace() + workspace()[:3])
    bad = tri.copy()
    bad[7, 4] = np.nan
    bad_box = boxes_from(workspace())
    bad_box[2].half[1] = float("inf")
    for fn in (valid_ref, create):
        assert fn(t, 0, bx, len(bx)) == EINVAL
        assert fn(big.ctypes.data_as(_dp), len(big), bx, len(bx)) == EINVAL
        assert fn(t, len(tri), nine, 9) == EINVAL and fn(t, len(tri), bx, 0) == EINVAL
        assert fn(bad.ctypes.data_as(_dp), len(bad), bx, len(bx)) == EINVAL
        assert fn(t, len(tri), bad_box, len(bad_box)) == EINVAL
    assert valid_ref(big.ctypes.data_as(_dp), _lib.OBJECT_MAX_TRIANGLES, bx, len(bx)) == 0  # the cap itself is allowed
    assert valid_ref(t, len(tri), bx, len(bx), inflate=float("nan")) == EINVAL and valid_ref(t, len(tri), bx, len(bx), inflate=-0.01) == EINVAL
    assert propose_ref(attempts=0) == EINVAL and propose_ref(attempts=17) == EINVAL and propose_ref(attempts=16) == 0
    limit = 1.44 * np.sqrt(3.0) / 2.0  # rotDev = 2 sigma / sqrt(3) > 1.44 is refused
    assert propose_ref(sigma=limit * 1.001) == EINVAL and propose_ref(sigma=limit * 0.999) == 0 and propose_ref(sigma=0.0) == 0
    assert propose_ref(sigma=-0.1) == EINVAL and propose_ref(sigma=float("nan")) == EINVAL and propose_ref(t_=float("inf")) == EINVAL
    assert propose_ref(to_stride=4) == EINVAL and propose_ref(to_stride=8) == 0
    hi_bad = (C.c_double * 3)(9, -10, 9)
    assert L.ccmp_object_propose_ref(t, len(tri), bx, len(bx), p, p, 0, 1, 0.3, 0.2, lo, hi_bad, 2, 0, 0, 0.0, out, which, None, None) == EINVAL
    assert L.ccmp_object_propose_ref(t, len(tri), bx, len(bx), None, p, 0, 1, 0.3, 0.2, lo, hi, 2, 0, 0, 0.0, out, which, None, None) == EINVAL
    assert L.ccmp_object_propose_ref(t, len(tri), bx, len(bx), None, None, 0, 0, 0.3, 0.2, lo, hi, 2, 0, 0, 0.0, None, None, None, None) == 0  # G == 0
