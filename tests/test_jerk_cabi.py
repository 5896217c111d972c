"""The C ABI of the jerk-bounded setpoints (include/ccmp.h: ccmp_path_jerk_setpoints, its host and _ref forms, ccmp_jerk_setpoints_*,
ccmp_jerk_opts): declarations and exports, the argument checks that come before any device, the two-call sizing of the _ref form, the
documented answers without a device, and that the documents name the call and say what it is not.  No device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_jerk_opts_default", "ccmp_path_jerk_setpoints", "ccmp_path_jerk_setpoints_host", "ccmp_jerk_setpoints_info", "ccmp_jerk_setpoints_copy",
         "ccmp_jerk_setpoints_copy_host", "ccmp_jerk_setpoints_destroy", "ccmp_jerk_setpoints_ref", "ccmp_jerk_next_window_ref"]


@pytest.fixture(scope="module")
def L(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    return _lib.lib()


def test_header_declares_and_the_library_exports(L):
    import closed_chain_motion_planner_amd as pkg
    from closed_chain_motion_planner_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ccmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for k, name in enumerate(("OK", "EMPTY", "NONFINITE", "UNORDERED", "POINT", "FULL", "WINDOW")):
        assert re.search(r"CCMP_JERK_%s = %d\b" % (name, k), code), name
    assert (_lib.JERK_OK, _lib.JERK_FULL, _lib.JERK_WINDOW) == (0, 5, 6)
    assert pkg.JERK_STATUS == pkg.SETPOINT_STATUS + ("window",)
    assert pkg.JERK_PEAKS == ("speed", "acceleration", "jerk", "dp", "angle", "clearance")
    assert pkg.PANDA_JERK_LIMITS == (7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0)
    assert all(a / j == 0.002 for a, j in zip(pkg.PANDA_ACCELERATION_LIMITS, pkg.PANDA_JERK_LIMITS))
    assert re.search(r"ccmp_jerk_opts\s*\{\s*double period;[^}]*int max_ticks;[^}]*int window;[^}]*int max_window;[^}]*double aim;[^}]*int tile_ticks;", code)
    o = _lib.CcmpJerkOpts(9.0, 9, 9, 9, 9.0, 9)
    L.ccmp_jerk_opts_default(C.byref(o))
    assert (o.period, o.max_ticks, o.window, o.max_window, o.aim, o.tile_ticks) == (0.001, 65536, 0, 64, 0.95, 0)
    L.ccmp_jerk_opts_default(None)  # a no-op
    assert callable(pkg.jerk_setpoints_ref) and hasattr(pkg.KinematicChainConstraint, "jerk_setpoint_paths")
    sig = inspect.signature(pkg.KinematicChainConstraint.jerk_setpoint_paths)
    assert [sig.parameters[k].default for k in ("period", "max_ticks", "window", "max_window", "aim", "scene", "margin", "stream")] == [0.001, 65536, 0, 64, 0.95, None, 0.0, None]
    sig = inspect.signature(pkg.Roadmap.executable_solution)
    assert [sig.parameters[k].default for k in ("jmax", "jerk_window", "jerk_max_window")] == [None, 0, 64]
    # the rule is one text: both units include it and are built with contraction off
    src = os.path.join(ROOT, "closed_chain_motion_planner_amd")
    for unit in ("ccmp_kernels_jerk.hip", "ccmp_jerk.cpp"):
        assert '#include "ccmp_jerk.h"' in open(os.path.join(src, "csrc", unit)).read()
    build = open(os.path.join(src, "build.py")).read()
    assert re.search(r'\("ccmp_kernels_jerk\.hip", \[[^\]]*"-ffp-contract=off"', build) and re.search(r'\("ccmp_jerk\.cpp", \[[^\]]*"-ffp-contract=off"', build)
    assert '(r"jerk_", 0)' in build
    rule = re.sub(r"/\*.*?\*/", "", open(os.path.join(src, "csrc", "ccmp_jerk.h")).read(), flags=re.S)
    assert "fma" not in rule.lower()


def test_no_kernel_of_the_unit_uses_scratch(ccmp_built):
    from closed_chain_motion_planner_amd import build

    report = build.resource_report()
    kernels = {k["name"]: k for k in report["ccmp_kernels_jerk.hip"]}
    assert set(kernels) == {"jerk_measure_kernel", "jerk_decide_kernel", "jerk_sample_kernel", "jerk_peak_kernel"}
    for name, k in kernels.items():
        assert k["scratch"] == 0 and k["scratch_bound"] == 0 and k.get("lds", 0) <= 65536, (name, k)


def _args(ctx, F=1, R=3, opts=None, host=False):
    d, i32, lim = (C.c_double * (8 * 14))(), (C.c_int32 * 8)(), (C.c_double * 14)(*([1.0] * 14))
    from closed_chain_motion_planner_amd import _lib

    out = C.c_void_p()
    a = [ctx, C.byref(_lib.CcmpProblem()), None, 0.0, d, i32, d, F, R, lim, lim, lim, opts, C.byref(out)]
    return a if host else a + [None]


def test_no_context_answers_the_documented_codes(L):
    """no quiet host path: without a device (no context can exist) the device forms say CCMP_ENODEV; with one a NULL context is
    CCMP_EINVAL — before any other check, F == 0 included"""
    import torch

    want = EINVAL if torch.cuda.is_available() else ENODEV
    for F in (1, 0):
        assert L.ccmp_path_jerk_setpoints(*_args(None, F)) == want
        assert L.ccmp_path_jerk_setpoints_host(*_args(None, F, host=True)) == want
    assert L.ccmp_jerk_setpoints_info(None, None, None) == EINVAL
    assert L.ccmp_jerk_setpoints_copy(*([None] * 15)) == want and L.ccmp_jerk_setpoints_copy_host(*([None] * 14)) == want
    L.ccmp_jerk_setpoints_destroy(None)  # a no-op


def _ref_args(opts=None):
    """three identical rows at time 0 (a POINT) behind path_first = [0, 3]"""
    d, lim = (C.c_double * (8 * 14))(), (C.c_double * 14)(*([1.0] * 14))
    pf = (C.c_int32 * 8)(0, 3)
    return [d, pf, d, 1, 3, lim, lim, lim, opts, (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_int32 * 8)(), None, None, None, None, None]


def test_the_ref_form_checks_its_arguments_and_needs_no_device(L):
    from closed_chain_motion_planner_amd import _lib

    lim = (C.c_double * 14)(*([1.0] * 14))
    assert L.ccmp_jerk_setpoints_ref(None, None, None, 0, 0, lim, lim, lim, None, (C.c_int32 * 2)(), None, None, None, None, None, None, None, None) == 0  # F == 0
    base = _ref_args()
    assert L.ccmp_jerk_setpoints_ref(*base) == 0
    assert list(base[9])[:2] == [0, 1] and base[10][0] == 4 and base[11][0] == 0 and base[12][0] == 0  # a POINT: one tick, window 0
    for k in (0, 1, 2, 5, 6, 7, 9, 10, 11, 12):  # NULL rows, path_first, time, vmax, amax, jmax, tick_first, status, window, passes
        bad = list(base)
        bad[k] = None
        assert L.ccmp_jerk_setpoints_ref(*bad) == EINVAL, k
    for which in (5, 6, 7):
        for v in (0.0, -1.0, float("inf"), float("nan")):
            bad = list(base)
            bad[which] = (C.c_double * 14)(*([1.0] * 13 + [v]))
            assert L.ccmp_jerk_setpoints_ref(*bad) == EINVAL, (which, v)
    J = _lib.CcmpJerkOpts
    for o in (J(0.0, 65536, 0, 64, 0.95, 0), J(float("nan"), 65536, 0, 64, 0.95, 0), J(0.001, 1, 0, 64, 0.95, 0), J(0.001, 65536, -1, 64, 0.95, 0),
              J(0.001, 65536, 65, 64, 0.95, 0), J(0.001, 65536, 0, 0, 0.95, 0), J(0.001, 65536, 0, 257, 0.95, 0), J(0.001, 65536, 0, 64, 0.0, 0),
              J(0.001, 65536, 0, 64, 1.25, 0), J(0.001, 65536, 0, 64, float("nan"), 0), J(0.001, 65536, 0, 64, 0.95, -1)):
        bad = list(base)
        bad[8] = C.byref(o)
        assert L.ccmp_jerk_setpoints_ref(*bad) == EINVAL, (o.period, o.max_ticks, o.window, o.max_window, o.aim, o.tile_ticks)
    for o in (J(0.001, 65536, 256, 256, 1.0, 0), J(0.001, 2, 1, 1, 0.5, 4096)):  # the ends of the ranges are inside them
        ok = list(base)
        ok[8] = C.byref(o)
        assert L.ccmp_jerk_setpoints_ref(*ok) == 0
    for pf in ((0, 9), (-1, 3), (2, 1)):  # beyond total_rows, negative, decreasing
        bad = list(base)
        bad[1] = (C.c_int32 * 8)(*pf)
        assert L.ccmp_jerk_setpoints_ref(*bad) == EINVAL, pf


def test_two_call_sizing(L):
    """NULL arrays first: tick_first, status, window and passes alone size the second call, which fills what it is given and no more"""
    from closed_chain_motion_planner_amd import _lib

    rows = np.zeros((4, 14))
    rows[:, 0] = [0.0, 0.001, 0.003, 0.004]
    time = np.array([0.0, 0.01, 0.02, 0.0295])  # n = ceil(29.5) = 30
    pf = np.array([0, 4, 4, 4], dtype=np.int32)
    pf[2] = 4  # path 1: empty; path 2: empty
    lim = [(C.c_double * 14)(*v) for v in ([2.0] * 14, [15.0] * 14, [5000.0] * 14)]
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32 if x.dtype == np.int32 else C.c_double))
    tf, st, w, ps = (np.full(5, -77, dtype=np.int32) for _ in range(4))
    head = [p(rows), p(pf), p(time), 3, 4, *lim, None, p(tf), p(st), p(w), p(ps)]
    assert L.ccmp_jerk_setpoints_ref(*head, None, None, None, None, None) == 0
    M = int(tf[3])
    assert tf[4] == -77 and st[3] == -77 and st[:3].tolist() == [0, 1, 1] and M == 30 + int(w[0]) and w[0] >= 1 and tf[:4].tolist() == [0, M, M, M]
    q, qd = np.full((M + 1, 14), -7.0), np.full((M + 1, 14), -7.0)
    tau, peak, tick = np.full(M + 1, -7.0), np.full(10, -7.0), np.full(10, -77, dtype=np.int32)
    assert L.ccmp_jerk_setpoints_ref(*head, p(q), None, p(tau), p(peak), None) == 0  # each destination is optional on its own
    assert (q[M] == -7.0).all() and (qd == -7.0).all() and tau[M] == -7.0 and peak[9] == -7.0 and (tick == -77).all()
    assert q[0, 0] == 0.0 and q[M - 1, 0] == 0.004 and tau[1] == 0.001 and 0.0 < peak[2] <= 1.0 and (peak[3:9] == 0.0).all()
    assert L.ccmp_jerk_setpoints_ref(*head, None, p(qd), None, None, p(tick)) == 0
    assert (qd[0] == 0.0).all() and (qd[M - 1] == 0.0).all() and (qd[M] == -7.0).all() and tick[9] == -77 and tick[3:9].tolist() == [-1] * 6
    o = _lib.CcmpJerkOpts(0.001, 30, 0, 64, 0.95, 0)  # n + 1 = 31 ticks do not fit 30: FULL, no tick
    head[8] = C.byref(o)
    assert L.ccmp_jerk_setpoints_ref(*head, None, None, None, None, None) == 0 and st[0] == 5 and tf[3] == 0


def test_the_documents_name_the_call_and_say_what_it_is_not():
    for name in ("README.md", "DESIGN.md", os.path.join("include", "ccmp.h")):
        assert "ccmp_path_jerk_setpoints" in open(os.path.join(ROOT, name)).read(), name
    flat = lambda *path: " ".join(re.sub(r"\n\s*\*", "\n", open(os.path.join(ROOT, *path)).read()).split())  # (without a comment's leading asterisks)
    design = flat("DESIGN.md")
    assert "5.20" in design and "no longer out of scope" in design
    rule = flat("closed_chain_motion_planner_amd", "csrc", "ccmp_jerk.h")
    for text in (design, flat("README.md"), rule, flat("include", "ccmp.h")):
        low = text.lower()
        assert "third difference of positions" in low and "jerk-optimal" in low and "cut corners" in low and "ticks of the stated period" in low
    assert "W*" in rule and "strictly increases" in rule
    assert "jerk" in open(os.path.join(ROOT, "tools", "README.md")).read()
    profile = open(os.path.join(ROOT, "profiles", "jerk.md")).read().lower()
    assert "wall clock" in profile and "wine_bottle" in profile and "dumbbell" in profile
