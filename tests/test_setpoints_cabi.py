"""The C ABI of the setpoints and the execution audit (include/ccmp.h: ccmp_path_setpoints and its handle, ccmp_setpoints_ref,
ccmp_setpoint_tangents_ref): declarations and exports, the documented answers without a device, and that the documents name the call.
No device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_setpoint_opts_default", "ccmp_path_setpoints", "ccmp_path_setpoints_host", "ccmp_setpoints_info", "ccmp_setpoints_copy",
         "ccmp_setpoints_copy_host", "ccmp_setpoints_destroy", "ccmp_setpoints_ref", "ccmp_setpoint_tangents_ref"]


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
    assert L.ccmp_version() == 600
    for k, name in enumerate(("OK", "EMPTY", "NONFINITE", "UNORDERED", "POINT", "FULL")):
        assert re.search(r"CCMP_SETPOINTS_%s = %d\b" % (name, k), code) and getattr(_lib, "SETPOINTS_" + name) == k
    assert len(pkg.SETPOINT_STATUS) == 6 and pkg.SETPOINT_PEAKS == ("speed", "acceleration", "dp", "angle", "clearance")
    assert re.search(r"ccmp_setpoint_opts\s*\{\s*double period;[^}]*int max_ticks;", code)
    o = _lib.CcmpSetpointOpts(9.0, 9)
    L.ccmp_setpoint_opts_default(C.byref(o))
    assert (o.period, o.max_ticks) == (0.001, 65536)
    L.ccmp_setpoint_opts_default(None)  # a no-op
    assert callable(pkg.setpoints_ref) and callable(pkg.setpoint_tangents_ref)
    assert hasattr(pkg.KinematicChainConstraint, "setpoint_paths") and hasattr(pkg.Roadmap, "executable_solution")
    adapter = open(os.path.join(ROOT, "include", "ccmp_ompl_adapter.hpp")).read()
    assert "setpointPath" in adapter and "constructExecutableSolution" in adapter and "printSetpoints" in adapter


def test_no_context_answers_the_documented_codes(L):
    """no quiet host path: without a device (no context can exist) the calls say CCMP_ENODEV; with one a NULL context is CCMP_EINVAL —
    before any other check, F == 0 included — and no handle is made"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    want = EINVAL if torch.cuda.is_available() else ENODEV
    P = _lib.CcmpProblem()
    d, i32, lim = (C.c_double * (8 * 14))(), (C.c_int32 * 8)(), (C.c_double * 14)(*([1.0] * 14))
    for F in (1, 0):
        h = C.c_void_p(0x1234)
        assert L.ccmp_path_setpoints(None, C.byref(P), None, 0.0, None, None, None, F, 0, lim, lim, None, C.byref(h), None) == want and not h.value
        h = C.c_void_p(0x1234)
        assert L.ccmp_path_setpoints_host(None, C.byref(P), None, 0.0, d, i32, d, F, 0, lim, lim, None, C.byref(h)) == want and not h.value
    assert L.ccmp_setpoints_copy(None, *([None] * 13)) == want
    assert L.ccmp_setpoints_copy_host(None, *([None] * 12)) == want
    assert L.ccmp_setpoints_info(None, None, None) == EINVAL
    L.ccmp_setpoints_destroy(None)  # a no-op


def test_the_ref_forms_never_need_a_device(L):
    lim = (C.c_double * 14)(*([1.0] * 14))
    tf = (C.c_int32 * 1)(7)
    assert L.ccmp_setpoints_ref(None, None, None, 0, 0, lim, lim, None, tf, None, None, None, None, None, None, None) == 0 and tf[0] == 0  # F == 0
    assert L.ccmp_setpoint_tangents_ref(None, None, 0, None) == 0  # R == 0 touches nothing


def test_the_documents_name_the_call():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "ccmp.h"), os.path.join("tools", "README.md")):
        text = open(os.path.join(ROOT, name)).read()
        assert "setpoint" in text, name
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "ccmp.h")):
        assert "ccmp_path_setpoints" in open(os.path.join(ROOT, name)).read(), name
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    assert "5.18" in design and "not projected" in design.lower()
    for out_of_scope in ("jerk", "quintic", "TOPP-RA"):
        assert out_of_scope in design, out_of_scope
    integration = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "setpoints and audit -> execute" in integration or "setpoints and audit → execute" in integration
    hdr = " ".join(open(os.path.join(ROOT, "include", "ccmp.h")).read().split())
    assert "NOT projected" in hdr and "SYNCHRONOUS on its stream (it reads F status words and F tick counts" in hdr
    assert os.path.exists(os.path.join(ROOT, "profiles", "setpoints.md"))
