"""The C ABI of the dense solution paths (include/ccmp.h: ccmp_path_densify and its handle, ccmp_dense_layout_ref, ccmp_dense_arc_ref):
declarations and exports, the documented answers without a device, and the argument checks of the two _ref forms.  No device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV, EOVERFLOW = -1, -5, -8
NAMES = ["ccmp_dense_opts_default", "ccmp_path_densify", "ccmp_path_densify_host", "ccmp_dense_paths_info", "ccmp_dense_paths_copy",
         "ccmp_dense_paths_copy_host", "ccmp_dense_paths_destroy", "ccmp_dense_layout_ref", "ccmp_dense_arc_ref"]


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
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert "#define CCMP_DENSE_DISTINCT 1" in code and _lib.DENSE_DISTINCT == 1 and pkg.DENSE_DISTINCT == 1
    assert L.ccmp_version() == 600
    assert "SYNCHRONOUS on its stream" in hdr  # the header says that the call waits
    o = _lib.CcmpDenseOpts(9, 9, 9, 9)
    L.ccmp_dense_opts_default(C.byref(o))
    assert (o.flags, o.chunk_states, o.round_budget, o.max_calls) == (0, 16, 128, 4096)
    assert callable(pkg.dense_layout_ref) and callable(pkg.dense_arc_ref)
    assert hasattr(pkg.KinematicChainConstraint, "densify_paths")
    assert all(hasattr(pkg.Roadmap, m) for m in ("dense_solution", "dense_approximate_solution"))
    adapter = open(os.path.join(ROOT, "include", "ccmp_ompl_adapter.hpp")).read()
    assert "interpolatePath" in adapter and "constructDenseSolution" in adapter


def test_no_context_answers_the_documented_codes(L):
    """no quiet host path: without a device (no context can exist) the calls say CCMP_ENODEV; with one a NULL context is CCMP_EINVAL —
    before any other check, F == 0 included — and no handle is made"""
    import torch

    want = EINVAL if torch.cuda.is_available() else ENODEV
    from closed_chain_motion_planner_amd import _lib

    i32 = (C.c_int32 * 8)()
    d = (C.c_double * (8 * 14))()
    P = _lib.CcmpProblem()
    h = C.c_void_p(0x1234)
    assert L.ccmp_path_densify(None, C.byref(P), None, 0.0, None, None, 1, 4, None, C.byref(h), None) == want and not h.value
    h = C.c_void_p(0x1234)
    assert L.ccmp_path_densify(None, C.byref(P), None, 0.0, None, None, 0, 4, None, C.byref(h), None) == want and not h.value
    h = C.c_void_p(0x1234)
    assert L.ccmp_path_densify_host(None, C.byref(P), None, 0.0, d, i32, 1, 4, None, C.byref(h)) == want and not h.value
    assert L.ccmp_dense_paths_copy(None, *([None] * 12)) == want
    assert L.ccmp_dense_paths_copy_host(None, *([None] * 11)) == want
    assert L.ccmp_dense_paths_info(None, None, None, None, None) == EINVAL
    L.ccmp_dense_paths_destroy(None)  # a no-op


def test_the_layout_ref_form_checks_its_arguments(L):
    ip = C.POINTER(C.c_int32)
    p = lambda a: a.ctypes.data_as(ip) if a is not None else None
    plen = np.array([3, 0, 1, 2], np.int32)
    ss = np.array([[2, 1], [0, 0], [0, 0], [5, 0]], np.int32)
    pf, sf = np.zeros(5, np.int32), np.zeros((4, 2), np.int32)
    rows = C.c_size_t(77)

    def call(plen=plen, F=4, ml=3, ss=ss, flags=0, pf=pf, sf=sf, rows=rows):
        return L.ccmp_dense_layout_ref(p(plen), F, ml, p(ss), flags, p(pf), p(sf), C.byref(rows) if rows is not None else None)

    assert call() == 0 and rows.value == 6 + 0 + 1 + 7 and pf.tolist() == [0, 6, 6, 7, 14] and sf.tolist() == [[1, 4], [-1, -1], [-1, -1], [8, -1]]
    assert call(flags=1) == 0 and rows.value == 4 + 0 + 1 + 6 and pf.tolist() == [0, 4, 4, 5, 11] and sf.tolist() == [[0, 2], [-1, -1], [-1, -1], [5, -1]]
    assert call(pf=None, sf=None) == 0 and rows.value == 14  # the optional outputs
    assert call(rows=None) == EINVAL and call(plen=None) == EINVAL and call(ss=None) == EINVAL
    assert call(flags=2) == EINVAL and call(flags=-1) == EINVAL
    assert call(ml=0) == EINVAL and call(ml=2) == EINVAL  # path_len 3 > max_len 2
    assert call(plen=np.array([3, -1, 1, 2], np.int32)) == EINVAL and call(plen=np.array([4, 0, 1, 2], np.int32)) == EINVAL
    assert call(ss=np.array([[2, 0], [0, 0], [0, 0], [5, 0]], np.int32)) == EINVAL  # a list holds its starting state at least
    assert call(F=0, plen=None, ss=None) == 0 and rows.value == 0 and pf[0] == 0  # no path: no row
    assert call(plen=np.array([1, 0, 1, 1], np.int32), ss=None) == 0 and rows.value == 3  # no segment anywhere: seg_states is not read
    big = np.array([[2**31 - 1, 2**31 - 1], [0, 0], [0, 0], [5, 0]], np.int32)
    assert call(ss=big) == EOVERFLOW  # rows are int32


def test_the_arc_ref_form_checks_its_arguments(L):
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rows = np.zeros((5, 14))
    rows[:, 0] = [0.0, 3.0, 3.0, 7.0, 7.5]
    pf = np.array([0, 3, 3, 5], np.int32)
    arc, length = np.full(5, -1.0), np.full(3, -1.0)

    def call(rows=rows, pf=pf, F=3, arc=arc, length=length):
        q = lambda a, t: a.ctypes.data_as(t) if a is not None else None
        return L.ccmp_dense_arc_ref(q(rows, dp), q(pf, ip), F, q(arc, dp), q(length, dp))

    assert call() == 0 and arc.tolist() == [0.0, 3.0, 3.0, 0.0, 0.5] and length.tolist() == [3.0, 0.0, 0.5]
    assert call(length=None) == 0
    assert call(pf=None) == EINVAL and call(rows=None) == EINVAL and call(arc=None) == EINVAL
    assert call(pf=np.array([0, 3, 2, 5], np.int32)) == EINVAL and call(pf=np.array([-1, 3, 3, 5], np.int32)) == EINVAL
    assert call(pf=np.array([0], np.int32), F=0, rows=None, arc=None, length=None) == 0
    assert call(pf=np.array([2, 2, 2, 2], np.int32), rows=None, arc=None) == 0 and length.tolist() == [0.0, 0.0, 0.0]  # empty paths alone


def test_interpolate_no_longer_remains_with_the_caller():
    """README, DESIGN, INTEGRATION and the header once ended on: what remains with the caller is PathGeometric::interpolate"""
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "ccmp.h"), os.path.join("include", "ccmp_ompl_adapter.hpp")):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert not re.search(r"remains with the caller is\W{0,4}PathGeometric::interpolate", text), name
        assert not re.search(r"PathGeometric::interpolate\W{0,4}(remains|stays) with the caller", text), name
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "5.14" in design and "ccmp_path_densify" in design
    assert os.path.exists(os.path.join(ROOT, "profiles", "dense_path.md"))
    assert "dense" in open(os.path.join(ROOT, "tools", "README.md")).read()
