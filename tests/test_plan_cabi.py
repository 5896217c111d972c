"""The C ABI of the planner's loop (include/ccmp.h: ccmp_plan_*): declarations and exports, the defaults of ccmp_plan_default_opts,
CCMP_ENODEV from the handle's entries on a machine without a device, and the argument checks of the *_ref forms.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_plan_default_opts", "ccmp_plan_create", "ccmp_plan_run", "ccmp_plan_state_read", "ccmp_plan_destroy", "ccmp_plan_check_ref", "ccmp_plan_prefix_ref",
         "ccmp_plan_connected_ref"]


@pytest.fixture(scope="module")
def L(ccmp_built):
    from closed_chain_motion_planner_amd import _lib

    return _lib.lib()


def test_header_declares_and_the_library_exports(L):
    from closed_chain_motion_planner_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "ccmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for text in ("#define CCMP_PLAN_MAX_STARTS 8", "#define CCMP_PLAN_MAX_GOALS 8", "#define CCMP_PLAN_MAX_WIDTH 256", "#define CCMP_PLAN_LADDER 9",
                 "CCMP_PLAN_OPEN = 0", "CCMP_PLAN_SOLVED = 1", "CCMP_PLAN_BUDGET = 2", "CCMP_PLAN_FULL = 3", "CCMP_PLAN_INVALID_GOAL = 4"):
        assert text in code, text
    assert (_lib.PLAN_OPEN, _lib.PLAN_SOLVED, _lib.PLAN_BUDGET, _lib.PLAN_FULL, _lib.PLAN_INVALID_GOAL) == (0, 1, 2, 3, 4)
    assert "TWO STATED DIFFERENCES" in hdr and "not their interleaving" in hdr  # the header says what the loop is not


def test_the_other_test_of_the_exports_still_holds(L, ccmp_built):
    """tests/test_host_cabi.py::test_exports_every_declared_symbol reads the header and EXPORTS: the new names are in both"""
    import test_host_cabi

    test_host_cabi.test_exports_every_declared_symbol(L, ccmp_built)


def test_struct_sizes_and_defaults(L):
    from closed_chain_motion_planner_amd import _lib, plan_options

    assert C.sizeof(_lib.CcmpPlanCounters) == 48 and C.sizeof(_lib.CcmpPlanState) == 240 and C.sizeof(_lib.CcmpPlanReport) == 112
    assert C.sizeof(_lib.CcmpPlanOpts) == 96
    o = plan_options()
    assert (o.width, o.k, o.attempts, o.max_states) == (32, 5, 2, 64)
    assert (o.t, o.sigma, o.inflate) == (0.3, 0.2, 0.0)
    assert list(o.lo) == [-1e30] * 3 and list(o.hi) == [1e30] * 3 and o.max_vertices == 2**31 - 1
    L.ccmp_plan_default_opts(None)  # a NULL pointer is ignored
    assert plan_options(width=7, lo=(0, 1, 2)).width == 7 and list(plan_options(lo=(0, 1, 2)).lo) == [0.0, 1.0, 2.0]
    with pytest.raises(TypeError):
        plan_options(no_such_field=1)


def test_handle_entries_answer_enodev_here(L):
    """no quiet host path: without a device no store and no plan can exist, and the entries say CCMP_ENODEV; with one a NULL handle is
    CCMP_EINVAL"""
    import torch
    from closed_chain_motion_planner_amd import _lib, plan_options

    want = EINVAL if torch.cuda.is_available() else ENODEV
    h, o = C.c_void_p(), plan_options()
    p = _lib.CcmpProblem()
    assert L.ccmp_plan_create(None, C.byref(p), None, None, 0.0, None, C.byref(o), None, 0, 0, C.byref(h)) == want and not h
    r, s = _lib.CcmpPlanReport(), _lib.CcmpPlanState()
    assert L.ccmp_plan_run(None, 4, C.byref(r)) == want
    assert L.ccmp_plan_state_read(None, C.byref(s)) == want
    L.ccmp_plan_destroy(None)


def test_ref_forms_check_their_arguments(L):
    from closed_chain_motion_planner_amd import _lib

    s = _lib.CcmpPlanState()
    trig = (C.c_int32 * 4)()
    i32, d = (C.c_int32 * 8)(), (C.c_double * 8)()
    assert L.ccmp_plan_check_ref(None, 4, i32, d, d, i32, d, d, None, trig) == EINVAL
    assert L.ccmp_plan_check_ref(C.byref(s), 4, i32, d, d, i32, d, d, None, None) == EINVAL
    s.n_starts = 9
    assert L.ccmp_plan_check_ref(C.byref(s), 4, i32, d, d, i32, d, d, None, trig) == EINVAL
    s.n_starts, s.n_goals = 1, 1
    assert L.ccmp_plan_check_ref(C.byref(s), 4, None, d, d, i32, d, d, None, trig) == EINVAL
    assert L.ccmp_plan_check_ref(C.byref(s), 2**31, i32, d, d, i32, d, d, None, trig) == EINVAL
    assert L.ccmp_plan_check_ref(C.byref(s), 4, i32, d, d, i32, d, d, None, trig) == 0  # never CCMP_ENODEV
    u8 = (C.c_uint8 * 9)()
    assert L.ccmp_plan_prefix_ref(None, u8, u8, None) == EINVAL and L.ccmp_plan_prefix_ref(u8, u8, u8, None) == 0
    assert L.ccmp_plan_connected_ref(None, 3, C.byref(s)) == EINVAL and L.ccmp_plan_connected_ref(i32, 3, None) == EINVAL
    s.n_goals = 9
    assert L.ccmp_plan_connected_ref(i32, 3, C.byref(s)) == EINVAL
    s.n_goals = 1
    assert L.ccmp_plan_connected_ref(i32, 3, C.byref(s)) == 0 and s.status == _lib.PLAN_SOLVED and (s.solved_start, s.solved_goal) == (0, 0)


def test_mirror_exports():
    import closed_chain_motion_planner_amd as pkg

    for name in ("Plan", "PLAN_STATUS", "plan_check_ref", "plan_prefix_ref", "plan_connected_ref", "plan_options"):
        assert hasattr(pkg, name), name
    assert pkg.PLAN_STATUS == {0: "OPEN", 1: "SOLVED", 2: "BUDGET", 3: "FULL", 4: "INVALID_GOAL"}
    assert hasattr(pkg.Roadmap, "plan")
