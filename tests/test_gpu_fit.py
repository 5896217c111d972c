"""Time stamps fitted to the limits at the controller's rate on the device (ccmp_path_fit_timestamps / _host: the fit_* kernels around the
setpoints unit's status and tangent launchers) through the C ABI and both mirror forms.  Expected values are never the code under test: the
plain-Python restatement of tests/fit_cases.py, computed once (fit_cases.reference) and shared.  Comparisons are bit for bit.  Calls through
the C ABI give every destination a guard element that must survive.

What the batch is for is asserted on the CPU in tests/test_fit_cases.py; the mutations tried against the rule are listed in
tests/test_fit_ref.py — the kernels compile the same header."""
import ctypes as C

import numpy as np
import pytest

import fit_cases as fc
import setpoint_cases as sc
from dense_path_cases import RECORDED
from fit_cases import FITTED, FULL, NAMES, PANDA_AMAX, PANDA_VMAX, PASSES, same_fit
from test_gpu_parity import _constraint

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
EINVAL = -1
GUARD_F64, GUARD_I32 = -7.0, -77
ORDER = ("time", "status", "passes", "peak", "duration", "factor")
INTS = ("status", "passes")


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    c = _constraint(OBJ, gpu_ctx, 1)
    c.problem.delta = RECORDED[OBJ]["delta"]
    return c


def _guarded(c, case, host=False, opts=True, factor=True, **over):
    """ccmp_path_fit_timestamps (or _host) through the C ABI: every destination one element longer than the result, pre-filled with a guard
    value (time_out and factor beyond the guard too: a row outside every path keeps it).  Returns (rc, outputs without the guard, every guard
    survived)."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    rows, first, time = case["rows"], case["path_first"], case["time"]
    F, R = len(first) - 1, len(rows)
    kw = dict(fc.options(case), **over)
    o = _lib.CcmpFitOpts(kw["period"], kw["max_ticks"], kw["aim"], kw["max_passes"])
    v, a = (C.c_double * 14)(*PANDA_VMAX), (C.c_double * 14)(*PANDA_AMAX)
    n = {"time": R, "status": F, "passes": F, "peak": 2 * F, "duration": F, "factor": R}
    if host:
        buf = {k: np.full(n[k] + 1, GUARD_I32 if k in INTS else GUARD_F64, dtype=np.int32 if k in INTS else np.float64) for k in ORDER}
        r, pf, t = (np.ascontiguousarray(x) for x in (rows, first, time))
        p = lambda x: x.ctypes.data_as(C.POINTER(C.c_int32 if x.dtype == np.int32 else C.c_double))
        code = L.ccmp_path_fit_timestamps_host(c.ctx.handle, p(r), p(pf), p(t), F, R, v, a, C.byref(o) if opts else None,
                                               *[p(buf[k]) if (factor or k != "factor") else None for k in ORDER])
        out = buf
    else:
        buf = {k: torch.full((n[k] + 1,), GUARD_I32 if k in INTS else GUARD_F64, dtype=torch.int32 if k in INTS else torch.float64, device="cuda") for k in ORDER}
        d_rows, d_first, d_time = _dev(rows), _dev(first), _dev(time)
        code = L.ccmp_path_fit_timestamps(c.ctx.handle, d_rows.data_ptr() if R else None, d_first.data_ptr(), d_time.data_ptr() if R else None, F, R, v, a,
                                          C.byref(o) if opts else None, *[buf[k].data_ptr() if (factor or k != "factor") else None for k in ORDER], None)
        torch.cuda.synchronize()
        out = {k: t.cpu().numpy() for k, t in buf.items()}
    intact = all(out[k][-1] == (GUARD_I32 if k in INTS else GUARD_F64) for k in ORDER)
    res = {k: out[k][:-1].copy() for k in ORDER}
    res["peak"] = res["peak"].reshape(-1, 2)
    return code, res, intact


def test_ragged_batch_everywhere(cons):
    """device and host forms of the C ABI and of the mirror against the restatement, and against each other"""
    ref = fc.reference()
    case, want = ref["case"], ref["want"]
    code, got, intact = _guarded(cons, case)
    assert code == 0 and intact
    same_fit(got, want, "C ABI")
    code, got_host, intact = _guarded(cons, case, host=True)
    assert code == 0 and intact
    same_fit(got_host, want, "C ABI, host form")
    same_fit(got_host, got, "host form against device form")
    dev = cons.fit_timestamps(_dev(case["rows"]), _dev(case["path_first"]), _dev(case["time"]), PANDA_VMAX, PANDA_AMAX, **fc.options(case))
    assert dev["time"].is_cuda
    same_fit(dev, want, "device mirror")
    host = cons.fit_timestamps(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, **fc.options(case))
    assert isinstance(host["time"], np.ndarray)
    same_fit(host, want, "host mirror")
    code, nofactor, intact = _guarded(cons, case, factor=False)  # factor is optional: its buffer keeps the guard throughout
    assert code == 0 and intact and (nofactor["factor"] == GUARD_F64).all()
    same_fit(nofactor, want, "no factor", keys=("time", "status", "passes", "peak", "duration"))
    print("ragged batch: status %s passes %s" % (got["status"].tolist(), got["passes"].tolist()))


def test_the_audit_of_the_fitted_stamps_reports_the_fits_peaks(cons):
    """the existing setpoint_paths, unchanged, on time_out: for every FITTED or PASSES path its speed and acceleration peaks ARE the fit's
    peak, bit for bit — the fit's ticks are the ticks the robot gets"""
    ref = fc.reference()
    case = ref["case"]
    fit = cons.fit_timestamps(_dev(case["rows"]), _dev(case["path_first"]), _dev(case["time"]), PANDA_VMAX, PANDA_AMAX, **fc.options(case))
    sp = cons.setpoint_paths(_dev(case["rows"]), _dev(case["path_first"]), fit["time"], PANDA_VMAX, PANDA_AMAX, period=case["period"], max_ticks=case["max_ticks"])
    status, peak, audit = fit["status"].cpu().numpy(), fit["peak"].cpu().numpy(), sp["peak"].cpu().numpy()
    ran = np.isin(status, (FITTED, PASSES))
    assert ran.sum() >= 8 and (sp["status"].cpu().numpy()[ran] == sc.OK).all()
    assert sc.same_f64(audit[ran][:, sc.SPEED], peak[ran][:, 0]) and sc.same_f64(audit[ran][:, sc.ACC], peak[ran][:, 1])
    assert (sp["stretch"].cpu().numpy()[status == FITTED] == 1.0).all()
    assert sp["status"].cpu().numpy()[NAMES.index("full_after")] == sc.FULL and status[NAMES.index("full_after")] == FULL


def test_two_launch_shapes_give_the_same_bits(cons):
    """the same paths in another order behind one more path: every tick interval in another group, wavefront and block, the measure and
    the dilate launches of every pass another size — and every path's answer the same bits; finished paths come back frozen"""
    ref = fc.reference()
    case, want = ref["case"], ref["want"]
    other, order = fc.reordered(case)
    code, got, intact = _guarded(cons, other)
    assert code == 0 and intact
    pf, qf = case["path_first"], other["path_first"]
    u = lambda a: np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
    for i, f in enumerate(order):
        assert got["status"][i + 1] == want["status"][f] and got["passes"][i + 1] == want["passes"][f], NAMES[f]
        assert np.array_equal(u(got["peak"][i + 1]), u(want["peak"][f])) and np.array_equal(u(got["duration"][i + 1]), u(want["duration"][f])), NAMES[f]
        for k in ("time", "factor"):
            assert np.array_equal(u(got[k][qf[i + 1]:qf[i + 2]]), u(want[k][pf[f]:pf[f + 1]])), (NAMES[f], k)
    f = NAMES.index("three")
    assert np.array_equal(u(got["time"][:3]), u(want["time"][pf[f]:pf[f + 1]])) and got["passes"][0] == want["passes"][f]
    # a pass budget of its own per call: with fewer passes the paths that were done earlier are the same bits, the others PASSES
    code, few, intact = _guarded(cons, case, max_passes=1)
    assert code == 0 and intact
    for f, name in enumerate(NAMES):
        a, b = pf[f], pf[f + 1]
        if want["passes"][f] <= 1 and want["status"][f] != PASSES:
            assert few["status"][f] == want["status"][f] and np.array_equal(u(few["time"][a:b]), u(want["time"][a:b])), name
        else:
            assert few["status"][f] == PASSES and few["passes"][f] == 1, name


def test_defaults_an_empty_call_and_ranges_that_are_never_read(cons):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, _lib

    ref = fc.reference()
    case = ref["case"]
    f = NAMES.index("three")
    a, b = case["path_first"][f], case["path_first"][f + 1]
    one = dict(case, rows=case["rows"][a:b], path_first=np.array([0, 3], dtype=np.int32), time=case["time"][a:b])
    want = fc.fit_py(one["rows"], one["path_first"], one["time"], PANDA_VMAX, PANDA_AMAX)  # 1 ms, 65 536 ticks, aim 0.95, eight passes
    for host in (False, True):
        code, got, intact = _guarded(cons, one, host=host, opts=False)
        assert code == 0 and intact
        same_fit(got, want, ("defaults", host))
    empty = dict(case, rows=np.zeros((0, 14)), path_first=np.array([0], dtype=np.int32), time=np.zeros(0))
    for host in (False, True):
        code, got, intact = _guarded(cons, empty, host=host)  # F == 0: nothing is written
        assert code == 0 and intact
    # path_first: the host form checks it; the device form never reads such a path, answers EMPTY and writes nothing of it
    for bad in ([-1, 3], [0, 4], [2, 1]):
        wrong = dict(one, path_first=np.array(bad, dtype=np.int32))
        code, _, intact = _guarded(cons, wrong, host=True)
        assert code == EINVAL and intact, bad
        with pytest.raises(CcmpError) as e:
            cons.fit_timestamps(one["rows"], wrong["path_first"], one["time"], PANDA_VMAX, PANDA_AMAX)
        assert e.value.code == EINVAL, bad
        code, got, intact = _guarded(cons, wrong)
        assert code == 0 and intact and got["status"].tolist() == [sc.EMPTY] and got["passes"].tolist() == [0] and got["duration"].tolist() == [0.0], bad
        assert (got["time"] == GUARD_F64).all() and (got["factor"] == GUARD_F64).all(), bad
    # a path in the middle of the rows: the rows around it keep the guard
    mid = dict(one, rows=np.vstack([one["rows"][:1], one["rows"], one["rows"][:1]]), path_first=np.array([1, 4], dtype=np.int32),
               time=np.concatenate([[5.0], one["time"], [6.0]]))
    for host in (False, True):
        code, got, intact = _guarded(cons, mid, host=host)
        assert code == 0 and intact and got["time"][0] == GUARD_F64 and got["time"][4] == GUARD_F64 and got["factor"][0] == GUARD_F64
        full = fc.fit_py(one["rows"], one["path_first"], one["time"], PANDA_VMAX, PANDA_AMAX, **fc.options(one))
        assert sc.same_f64(got["time"][1:4], full["time"]) and sc.same_f64(got["factor"][1:4], full["factor"])
    # argument errors of the device form
    L = _lib.lib()
    v, am = (C.c_double * 14)(*PANDA_VMAX), (C.c_double * 14)(*PANDA_AMAX)
    d_rows, d_first, d_time = _dev(one["rows"]), _dev(one["path_first"]), _dev(one["time"])
    out = [torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda"),
           torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")]
    args = [cons.ctx.handle, d_rows.data_ptr(), d_first.data_ptr(), d_time.data_ptr(), 1, 3, v, am, None] + [t.data_ptr() for t in out]
    assert L.ccmp_path_fit_timestamps(*args, None) == 0
    for k in (1, 2, 3, 6, 7, 9, 10, 11, 12, 13):  # NULL rows, path_first, time, vmax, amax, time_out, status, passes, peak, duration
        bad = list(args)
        bad[k] = None
        assert L.ccmp_path_fit_timestamps(*bad, None) == EINVAL, k
    bad = list(args)
    bad[9] = d_time.data_ptr()  # in place
    assert L.ccmp_path_fit_timestamps(*bad, None) == EINVAL
    for o in (_lib.CcmpFitOpts(0.001, 65536, 0.0, 8), _lib.CcmpFitOpts(0.001, 65536, 1.25, 8), _lib.CcmpFitOpts(0.001, 65536, float("nan"), 8),
              _lib.CcmpFitOpts(0.001, 65536, 0.95, -1), _lib.CcmpFitOpts(0.001, 1, 0.95, 8), _lib.CcmpFitOpts(-1.0, 65536, 0.95, 8)):
        bad = list(args)
        bad[8] = C.byref(o)
        assert L.ccmp_path_fit_timestamps(*bad, None) == EINVAL
    torch.cuda.synchronize()


def test_executable_solution_with_fit(cons):
    """... -> time stamps -> fit -> setpoints and audit: the fit's dict is appended, the setpoints are those of the fitted stamps, and without
    fit the tuple is what it was"""
    from closed_chain_motion_planner_amd import Roadmap
    from dense_path_cases import recorded_roadmap

    c = cons
    nodes, uv = recorded_roadmap()
    rm = Roadmap(c, capacity_hint=4)
    try:
        rm.append(_dev(nodes))
        assert rm.add_edges(_dev(uv)) == 0
        plain = rm.executable_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True)
        fitted = rm.executable_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True, fit=True)
    finally:
        rm.close()
    assert len(plain) == 8 and len(fitted) == 9
    sp, duration, _, sampled, stamps, _, _, _, fit = fitted
    rows, first, time = (x.cpu().numpy() for x in (sampled["joints"], sampled["path_first"], stamps["time"]))
    assert sc.same_f64(time, plain[4]["time"].cpu().numpy()) and duration == plain[1]
    want = fc.fit_py(rows, first, time, PANDA_VMAX, PANDA_AMAX)
    same_fit(fit, want, "executable solution")
    audit = sc.setpoints_py(rows, first, want["time"], PANDA_VMAX, PANDA_AMAX)
    sc.same_setpoints(sp, audit, "setpoints of the fitted stamps", keys=("q", "qd", "tau", "tick_first", "status"))
    got_peak = sp["peak"].cpu().numpy()
    assert sc.same_f64(got_peak[:, :2], want["peak"])
    print("executable solution with fit: %s after %d dilations, %.3f -> %.3f s, peaks %s (before: %s)" % (
        fc.FITTED == want["status"][0], want["passes"][0], duration, want["duration"][0], want["peak"][0].tolist(), plain[0]["peak"].cpu().numpy()[0, :2].tolist()))
    assert want["status"].tolist() == [FITTED] and (want["peak"] <= 1.0).all() and want["duration"][0] > duration
