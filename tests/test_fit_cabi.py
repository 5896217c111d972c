"""The C ABI of the fitted time stamps (include/ccmp.h: ccmp_path_fit_timestamps, its host and _ref forms, ccmp_fit_opts): declarations and
exports, the argument checks that come before any device, the documented answers without a device, and that the documents name the call
and say what it is not.  No device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENODEV = -1, -5
NAMES = ["ccmp_fit_opts_default", "ccmp_path_fit_timestamps", "ccmp_path_fit_timestamps_host", "ccmp_path_fit_timestamps_ref"]


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
    assert re.search(r"CCMP_FIT_FITTED = 0\b", code) and re.search(r"CCMP_FIT_PASSES = 6\b", code)
    assert (_lib.FIT_FITTED, _lib.FIT_PASSES) == (0, 6)
    assert pkg.FIT_STATUS == ("fitted",) + pkg.SETPOINT_STATUS[1:] + ("passes",)
    assert re.search(r"ccmp_fit_opts\s*\{\s*double period;[^}]*int max_ticks;[^}]*double aim;[^}]*int max_passes;", code)
    o = _lib.CcmpFitOpts(9.0, 9, 9.0, 9)
    L.ccmp_fit_opts_default(C.byref(o))
    assert (o.period, o.max_ticks, o.aim, o.max_passes) == (0.001, 65536, 0.95, 8)
    L.ccmp_fit_opts_default(None)  # a no-op
    assert callable(pkg.fit_timestamps_ref) and hasattr(pkg.KinematicChainConstraint, "fit_timestamps")
    import inspect

    sig = inspect.signature(pkg.Roadmap.executable_solution)
    assert sig.parameters["fit"].default is False
    adapter = open(os.path.join(ROOT, "include", "ccmp_ompl_adapter.hpp")).read()
    assert "fitPath" in adapter and "ccmp_path_fit_timestamps" in adapter


def _args(ctx, F=1, R=3, opts=None):
    d, i32, lim = (C.c_double * (8 * 14))(), (C.c_int32 * 8)(), (C.c_double * 14)(*([1.0] * 14))
    out = (C.c_double * 8)()
    return [ctx, d, i32, d, F, R, lim, lim, opts, out, (C.c_int32 * 8)(), (C.c_int32 * 8)(), (C.c_double * 16)(), (C.c_double * 8)(), (C.c_double * 8)()]


def test_no_context_answers_the_documented_codes(L):
    """no quiet host path: without a device (no context can exist) the device forms say CCMP_ENODEV; with one a NULL context is
    CCMP_EINVAL — before any other check, F == 0 included"""
    import torch

    want = EINVAL if torch.cuda.is_available() else ENODEV
    for F in (1, 0):
        assert L.ccmp_path_fit_timestamps(*_args(None, F), None) == want
        assert L.ccmp_path_fit_timestamps_host(*_args(None, F)) == want


def test_the_ref_form_checks_its_arguments_and_needs_no_device(L):
    from closed_chain_motion_planner_amd import _lib

    assert L.ccmp_path_fit_timestamps_ref(None, None, None, 0, 0, *_args(None)[6:8], None, None, None, None, None, None, None) == 0  # F == 0 touches nothing
    base = _args(None)[1:]
    base[1][1] = 3  # path_first = [0, 3]
    assert L.ccmp_path_fit_timestamps_ref(*base) == 0  # three identical rows at time 0: a POINT
    assert base[9][0] == 4 and base[10][0] == 0
    for k in (0, 1, 2, 5, 6, 8, 9, 10, 11, 12):  # NULL rows, path_first, time, vmax, amax, time_out, status, passes, peak, duration
        bad = list(base)
        bad[k] = None
        assert L.ccmp_path_fit_timestamps_ref(*bad) == EINVAL, k
    ok = list(base)
    ok[13] = None  # factor is optional
    assert L.ccmp_path_fit_timestamps_ref(*ok) == 0
    for o in (_lib.CcmpFitOpts(0.001, 65536, 0.0, 8), _lib.CcmpFitOpts(0.001, 65536, 1.5, 8), _lib.CcmpFitOpts(0.001, 65536, 0.95, -1),
              _lib.CcmpFitOpts(0.0, 65536, 0.95, 8), _lib.CcmpFitOpts(0.001, 1, 0.95, 8)):
        bad = list(base)
        bad[7] = C.byref(o)
        assert L.ccmp_path_fit_timestamps_ref(*bad) == EINVAL, (o.period, o.max_ticks, o.aim, o.max_passes)
    bad = list(base)
    bad[1] = (C.c_int32 * 8)(0, 9)  # beyond total_rows
    assert L.ccmp_path_fit_timestamps_ref(*bad) == EINVAL


def test_the_documents_name_the_call_and_say_what_it_is_not():
    for name in ("README.md", "DESIGN.md", "INTEGRATION.md", os.path.join("include", "ccmp.h"), os.path.join("tools", "README.md")):
        assert "ccmp_path_fit_timestamps" in open(os.path.join(ROOT, name)).read() or name.endswith(os.path.join("tools", "README.md")), name
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    assert "5.19" in design
    for text in (design, " ".join(open(os.path.join(ROOT, "README.md")).read().split())):
        low = text.lower()
        assert "not topp-ra" in low and "no jerk limit" in low and "observed" in low and "aim = 1" in low and "ticks of the stated period" in low
    assert "fit" in open(os.path.join(ROOT, "tools", "README.md")).read()
    integration = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "time stamps -> fit -> setpoints and audit -> execute" in integration or "time stamps → fit → setpoints and audit → execute" in integration
    assert os.path.exists(os.path.join(ROOT, "profiles", "fit.md"))
