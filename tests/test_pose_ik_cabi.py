"""The pose-IK C ABI without a device: declarations, exports, the new call kind of ccmp_ctx_describe, and what the device and host
forms answer where no context can exist (ccmp_pose_ik_ref is the host path and is tested in tests/test_pose_ik_host.py)."""
import ctypes as C
import os
import re

from conftest import ROOT

from closed_chain_motion_planner_amd import _lib

HEADER = open(os.path.join(ROOT, "include", "ccmp.h")).read()
ENTRIES = ("ccmp_ik_opts_default", "ccmp_pose_ik_batch", "ccmp_pose_ik_host", "ccmp_pose_ik_ref", "ccmp_roadmap_grow", "ccmp_roadmap_grow_host")


def test_header_declares_the_entry_points(ccmp_built):
    for name in ENTRIES:
        assert re.search(r"\b(int|void) %s\(" % name, HEADER), name
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert re.search(r"CCMP_CALL_POSE_IK = 13\b", HEADER) and _lib.CALL_POSE_IK == 13
    assert _lib.lib().ccmp_version() == 600  # an addition: the version stays
    o = _lib.CcmpIkOpts()
    _lib.lib().ccmp_ik_opts_default(C.byref(o))
    assert (o.restarts, o.max_rounds, o.eps, o.lambda_, o.err_clamp, o.sigma) == (14, 64, 1e-5, 0.05, 0.5, 0.3)
    _lib.lib().ccmp_ik_opts_default(None)
    assert (_lib.IK_MAX_SEEDS, _lib.IK_MAX_RESTARTS, _lib.IK_MAX_ROUNDS) == tuple(
        int(re.search(r"#define CCMP_IK_MAX_%s (\d+)" % n, HEADER).group(1)) for n in ("SEEDS", "RESTARTS", "ROUNDS"))


def test_describe_answers_kind_13_only(ccmp_built):
    L = _lib.lib()
    buf = C.create_string_buffer(64)
    for kind in (9, 12, 14, 99):
        assert L.ccmp_ctx_describe(None, kind, 16, buf, len(buf)) == -1, kind
    for n in (1, 4096):
        line = _lib.describe(None, _lib.CALL_POSE_IK, n)
        lanes = n * 5 * 15
        assert line.startswith("pose_ik T=%d " % n) and "ik_solve_kernel x %d blocks" % (2 * ((lanes + 63) // 64)) in line and "ik_select_kernel" in line
        assert "%d candidates" % (2 * lanes) in line
    full = _lib.describe(None, _lib.CALL_POSE_IK, 64)
    assert L.ccmp_ctx_describe(None, _lib.CALL_POSE_IK, 64, buf, len(buf)) == len(full) and buf.value.decode() == full[:63]


def test_device_and_host_forms_answer_enodev_here(ccmp_built):
    """There is no quiet host path behind the device entry points: without a device they say CCMP_ENODEV (with one, a NULL context or
    store is an argument error)."""
    import torch

    L = _lib.lib()
    want = -1 if torch.cuda.is_available() else -5  # CCMP_EINVAL / CCMP_ENODEV
    P = _lib.CcmpProblem()
    pose, seeds, q = (C.c_double * 8)(), (C.c_double * 14)(), (C.c_double * 14)()
    ok, which, idx = (C.c_uint8 * 1)(), (C.c_int32 * 1)(), (C.c_int32 * 1)()
    assert L.ccmp_pose_ik_batch(None, C.byref(P), None, pose, seeds, 1, 1, 0, 0, q, ok, which, None, None, None) == want
    assert L.ccmp_pose_ik_host(None, C.byref(P), None, pose, seeds, 1, 1, 0, 0, q, ok, which, None, None) == want
    assert L.ccmp_roadmap_grow(None, C.byref(P), None, 0.0, None, pose, 1, 1, 0, 0, 0, 0, 0, 4, 0, idx, None, q, ok, which, q, idx, ok, None, None, None, None) == want
    assert L.ccmp_roadmap_grow_host(None, C.byref(P), None, 0.0, None, pose, 1, 1, 0, 0, 0, 0, 0, 4, 0, idx, None, q, ok, which, q, idx, ok, None, None, None) == want
