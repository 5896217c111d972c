"""The C ABI of RRT-Connect on the store (include/ccmp.h: ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree*): declarations and exports, the
defaults of ccmp_rrtc_default_opts, the struct sizes, CCMP_ENODEV from the handle's entries on a machine without a device, the argument
checks of the *_ref forms, and the header's statement of what the unit is not.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_rrtc_default_opts", "ccmp_rrtc_create", "ccmp_rrtc_run", "ccmp_rrtc_state_read", "ccmp_rrtc_destroy", "ccmp_roadmap_nearest_in_tree",
         "ccmp_roadmap_nearest_in_tree_host", "ccmp_roadmap_nearest_in_tree_ref", "ccmp_rrtc_nearest_shape", "ccmp_rrtc_pick_ref", "ccmp_rrtc_pick_batch",
         "ccmp_rrtc_connected_ref"]


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
    for text in ("CCMP_RRTC_OPEN = 0", "CCMP_RRTC_SOLVED = 1", "CCMP_RRTC_BUDGET = 2", "CCMP_RRTC_FULL = 3", "CCMP_RRTC_NONE = -1", "CCMP_RRTC_TRAPPED = 0",
                 "CCMP_RRTC_ADVANCED = 1", "CCMP_RRTC_REACHED = 2", "CCMP_RRTC_UNSETTLED = 3", "CCMP_RRTC_CONNECT_NOTHING = 0", "CCMP_RRTC_CONNECT_ADDED = 1",
                 "CCMP_RRTC_CONNECT_JOINED = 2", "#define CCMP_RRTC_MAX_ROOTS 8"):
        assert text in code, text
    assert (_lib.RRTC_OPEN, _lib.RRTC_SOLVED, _lib.RRTC_BUDGET, _lib.RRTC_FULL) == (0, 1, 2, 3)
    assert (_lib.RRTC_NONE, _lib.RRTC_TRAPPED, _lib.RRTC_ADVANCED, _lib.RRTC_REACHED, _lib.RRTC_UNSETTLED) == (-1, 0, 1, 2, 3)


def test_the_header_states_the_differences_from_ompl(L):
    hdr = open(os.path.join(ROOT, "include", "ccmp.h")).read()
    at = hdr.index("STATED DIFFERENCES FROM OMPL'S RRTConnect")
    text = hdr[at:at + 3000]
    for mark in ("(a)", "(b)", "(c)", "(d)", "(e)", "(f)", "clipped at range", "UNSETTLED is skipped", "counter-based", "proxy scene", "not guaranteed"):
        assert mark in text, mark
    rule = open(os.path.join(ROOT, "closed_chain_motion_planner_amd", "csrc", "ccmp_rrtc.h")).read()
    assert "CCMP_HD" in rule and "rrtc_extend" in rule and "rrtc_connect" in rule


def test_the_other_test_of_the_exports_still_holds(L, ccmp_built):
    """tests/test_host_cabi.py::test_exports_every_declared_symbol reads the header and EXPORTS: the new names are in both"""
    import test_host_cabi

    test_host_cabi.test_exports_every_declared_symbol(L, ccmp_built)


def test_struct_sizes_and_defaults(L):
    from closed_chain_motion_planner_amd import _lib, rrtc_options

    assert C.sizeof(_lib.CcmpRrtcOpts) == 32 and C.sizeof(_lib.CcmpRrtcCounters) == 48
    assert C.sizeof(_lib.CcmpRrtcState) == 160 and C.sizeof(_lib.CcmpRrtcReport) == 104
    assert _lib.CcmpRrtcState.next_index.offset == 80 and _lib.CcmpRrtcState.best_gap.offset == 104 and _lib.CcmpRrtcState.counters.offset == 112  # no padding
    o = rrtc_options()
    assert (o.width, o.max_states, o.round_budget, o.range, o.max_vertices) == (32, 64, 0, 0.1, 2**31 - 1)
    L.ccmp_rrtc_default_opts(None)  # a NULL pointer is ignored
    assert rrtc_options(width=7, range=0.5).width == 7 and rrtc_options(range=0.5).range == 0.5
    with pytest.raises(TypeError):
        rrtc_options(no_such_field=1)


def test_handle_entries_answer_enodev_here(L):
    """no quiet host path: without a device no store and no planner can exist, and the entries say CCMP_ENODEV; with one a NULL handle is
    CCMP_EINVAL"""
    import torch
    from closed_chain_motion_planner_amd import _lib, rrtc_options

    want = EINVAL if torch.cuda.is_available() else ENODEV
    h, o = C.c_void_p(), rrtc_options()
    p = _lib.CcmpProblem()
    one = (C.c_int32 * 1)(0)
    assert L.ccmp_rrtc_create(None, C.byref(p), None, 0.0, C.byref(o), one, 1, one, 1, 0, 0, C.byref(h)) == want and not h
    r, s = _lib.CcmpRrtcReport(), _lib.CcmpRrtcState()
    assert L.ccmp_rrtc_run(None, 4, C.byref(r)) == want
    assert L.ccmp_rrtc_state_read(None, C.byref(s)) == want
    L.ccmp_rrtc_destroy(None)
    q, i, d = np.zeros((2, 14)), np.zeros(2, dtype=np.int32), np.zeros(2)
    assert L.ccmp_roadmap_nearest_in_tree_host(None, one, 1, q.ctypes.data_as(C.POINTER(C.c_double)), 2, i.ctypes.data_as(C.POINTER(C.c_int32)),
                                               d.ctypes.data_as(C.POINTER(C.c_double))) == want
    assert L.ccmp_roadmap_nearest_in_tree(None, None, 0, None, 0, None, None, None) == want
    assert L.ccmp_rrtc_pick_batch(None, 0, None, None, None, None, None, None, 0, 4, 0.1, None, None, None, None, None) == want


def test_ref_forms_check_their_arguments(L):
    from closed_chain_motion_planner_amd import _lib

    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    st, to, d = np.zeros((2, 4, 14)), np.zeros((2, 14)), np.zeros(2)
    ns, ok = np.full(2, 2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
    out, rix, row = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros((2, 14))
    a = lambda x, t: x.ctypes.data_as(t)
    args = lambda: [a(st, dp), a(ns, ip), a(ok, up), None, a(to, dp), a(d, dp), 2, 4, 0.1, a(out, ip), a(rix, ip), a(row, dp), None]
    assert L.ccmp_rrtc_pick_ref(0, *args()) == 0  # never CCMP_ENODEV
    assert L.ccmp_rrtc_pick_ref(2, *args()) == EINVAL
    for hole in (0, 1, 2, 4, 9, 10, 11):
        b = args()
        b[hole] = None
        assert L.ccmp_rrtc_pick_ref(0, *b) == EINVAL, hole
    b = args()
    b[5] = None  # d: step 2 needs it, step 3 does not
    assert L.ccmp_rrtc_pick_ref(0, *b) == EINVAL and L.ccmp_rrtc_pick_ref(1, *b) == 0
    b = args()
    b[7] = 0
    assert L.ccmp_rrtc_pick_ref(0, *b) == EINVAL
    b = args()
    b[6] = 0  # no lists: nothing is touched
    assert L.ccmp_rrtc_pick_ref(0, *b) == 0
    j, lab = np.zeros((3, 14)), np.zeros(3, dtype=np.int32)
    roots = np.array([0, 1, 3], dtype=np.int32)
    i2, d2 = np.zeros(2, dtype=np.int32), np.zeros(2)
    assert L.ccmp_roadmap_nearest_in_tree_ref(a(j, dp), a(lab, ip), 3, a(roots, ip), 2, a(to, dp), 2, a(i2, ip), a(d2, dp)) == 0
    assert L.ccmp_roadmap_nearest_in_tree_ref(a(j, dp), a(lab, ip), 3, a(roots, ip), 3, a(to, dp), 2, a(i2, ip), a(d2, dp)) == EINVAL  # root 3 is outside
    assert L.ccmp_roadmap_nearest_in_tree_ref(a(j, dp), a(lab, ip), 3, a(roots, ip), 9, a(to, dp), 2, a(i2, ip), a(d2, dp)) == EINVAL
    assert L.ccmp_roadmap_nearest_in_tree_ref(a(j, dp), a(lab, ip), 3, None, 1, a(to, dp), 2, a(i2, ip), a(d2, dp)) == EINVAL
    assert L.ccmp_roadmap_nearest_in_tree_ref(a(j, dp), None, 3, a(roots, ip), 1, a(to, dp), 2, a(i2, ip), a(d2, dp)) == EINVAL
    assert L.ccmp_roadmap_nearest_in_tree_ref(a(j, dp), a(lab, ip), 3, a(roots, ip), 1, a(to, dp), 2, None, a(d2, dp)) == EINVAL
    s = _lib.CcmpRrtcState()
    i32 = (C.c_int32 * 8)()
    assert L.ccmp_rrtc_connected_ref(None, 3, C.byref(s)) == EINVAL and L.ccmp_rrtc_connected_ref(i32, 3, None) == EINVAL
    s.n_starts, s.n_goals = 1, 9
    assert L.ccmp_rrtc_connected_ref(i32, 3, C.byref(s)) == EINVAL
    s.n_goals = 1
    assert L.ccmp_rrtc_connected_ref(i32, 3, C.byref(s)) == 0 and s.status == _lib.RRTC_SOLVED and (s.solved_start, s.solved_goal) == (0, 0)
    part, parts = C.c_uint(), C.c_uint()
    assert L.ccmp_rrtc_nearest_shape(None, 32, 1025, C.byref(part), C.byref(parts)) == 0 and part.value % 256 == 0 and parts.value * part.value >= 1025
    assert L.ccmp_rrtc_nearest_shape(None, 32, 1025, None, C.byref(parts)) == EINVAL


def test_the_shape_is_a_function_of_q_n_and_the_cu_count(L):
    """a 256-CU device: a small store is one partition, a large one is cut; many queries need fewer cuts"""
    from closed_chain_motion_planner_amd import rrtc_nearest_shape

    assert rrtc_nearest_shape(None, 1, 0) == (256, 1) and rrtc_nearest_shape(None, 1, 256) == (256, 1)
    assert rrtc_nearest_shape(None, 1, 257) == (256, 2) and rrtc_nearest_shape(None, 65, 1025) == (256, 5)
    assert rrtc_nearest_shape(None, 1, 10**6) == (4096, 245) and rrtc_nearest_shape(None, 256, 10**6)[1] == 4 and rrtc_nearest_shape(None, 2048, 10**6)[1] == 1


def test_mirror_exports():
    import closed_chain_motion_planner_amd as pkg

    for name in ("RRTConnect", "RRTC_STATUS", "rrtc_pick_ref", "rrtc_pick", "rrtc_connected_ref", "rrtc_options", "nearest_in_tree_ref", "rrtc_nearest_shape"):
        assert hasattr(pkg, name), name
    assert pkg.RRTC_STATUS == {0: "OPEN", 1: "SOLVED", 2: "BUDGET", 3: "FULL"}
    assert hasattr(pkg.Roadmap, "rrt_connect") and hasattr(pkg.Roadmap, "nearest_in_tree")
