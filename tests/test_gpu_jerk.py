"""Jerk-bounded setpoints on the device (ccmp_path_jerk_setpoints / _host: the jerk_* kernels around the setpoints unit's status and tangent
launchers and the function, is-satisfied and clearance launchers) through the C ABI and both mirror forms.  Expected values are never the
code under test: the plain-Python restatement of tests/jerk_cases.py for q, qd, tau, the window search and the audit, the det oracle's
`function`, `is_satisfied` and `clearance` applied to the expected FILTERED ticks for f, satisfied and the clearance — computed once
(jerk_cases.reference) and shared; where a larger input makes the restatement slow, the _ref form (itself compared with the restatement in
tests/test_jerk_ref.py).  Comparisons are bit for bit.  Calls through the C ABI give every destination a guard element that must survive.

What the batch is for is asserted on the CPU in tests/test_jerk_cases.py; the mutations tried against the rule are listed in
tests/test_jerk_ref.py — the kernels compile the same header."""
import ctypes as C

import numpy as np
import pytest

import arm_model_cases as A
import jerk_cases as jc
import setpoint_cases as sc
from dense_path_cases import RECORDED
from jerk_cases import CASE_TILE, EMPTY, FIXED_WINDOWS, FULL, NAMES, OK, PANDA_AMAX, PANDA_JMAX, PANDA_VMAX, WINDOW, same_jerk
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
EINVAL = -1
GUARD_F64, GUARD_I32, GUARD_U8 = -7.0, -77, 177
SHAPES = {"q": 14, "qd": 14, "tau": 1, "f": 2, "satisfied": 1, "clearance": 1}  # per tick
PER_PATH = {"status": 1, "window": 1, "passes": 1, "peak": 6, "peak_tick": 6, "counts": 2}
ORDER = ("q", "qd", "tau", "tick_first", "f", "satisfied", "clearance", "status", "window", "passes", "peak", "peak_tick", "counts")
DTYPE = {"tick_first": "int32", "satisfied": "uint8", "status": "int32", "window": "int32", "passes": "int32", "peak_tick": "int32", "counts": "int32"}


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def cons(gpu_ctx, oracle_det):
    """the constraint whose problem is the one of jerk_cases.reference()"""
    c = _constraint(OBJ, gpu_ctx, 1)
    c.problem.delta = RECORDED[OBJ]["delta"]
    assert bytes(_oracle_problem(oracle_det, c)) == bytes(jc.reference()["P"])
    return c


def _opts(case, **over):
    from closed_chain_motion_planner_amd import _lib

    kw = dict(jc.options(case), window=0, tile_ticks=0)
    kw.update(over)
    return _lib.CcmpJerkOpts(kw["period"], kw["max_ticks"], kw["window"], kw["max_window"], kw["aim"], kw["tile_ticks"])


def _guarded(c, case, scene=None, margin=0.0, opts=True, host=False, vmax=PANDA_VMAX, amax=PANDA_AMAX, jmax=None, **over):
    """ccmp_path_jerk_setpoints (or _host) and ccmp_jerk_setpoints_copy through the C ABI: every destination one element longer than the
    result, pre-filled with a guard value.  Returns (rc, outputs without the guard or None, every guard survived / no handle on an error)."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    L, h = _lib.lib(), C.c_void_p(1)
    rows, first, time = case["rows"], case["path_first"], case["time"]
    F, R = len(first) - 1, len(rows)
    o = _opts(case, **over)
    v, a, j = ((C.c_double * 14)(*x) for x in (vmax, amax, case["jmax"] if jmax is None else jmax))
    sh = scene._h if scene is not None else None
    if host:
        r, pf, t = (np.ascontiguousarray(x) for x in (rows, first, time))
        p = lambda x, ty: x.ctypes.data_as(C.POINTER(ty)) if x.size else None
        code = L.ccmp_path_jerk_setpoints_host(c.ctx.handle, C.byref(c.problem), sh, float(margin), p(r, C.c_double), p(pf, C.c_int32), p(t, C.c_double), F, R, v, a, j,
                                               C.byref(o) if opts else None, C.byref(h))
    else:
        d_rows, d_first, d_time = _dev(rows), _dev(first), _dev(time)
        code = L.ccmp_path_jerk_setpoints(c.ctx.handle, C.byref(c.problem), sh, float(margin), d_rows.data_ptr() if R else None, d_first.data_ptr(),
                                          d_time.data_ptr() if R else None, F, R, v, a, j, C.byref(o) if opts else None, C.byref(h), None)
    if code != 0:
        return code, None, not h.value  # no handle on any error
    try:
        nF, M = C.c_size_t(0), C.c_size_t(0)
        assert L.ccmp_jerk_setpoints_info(h, C.byref(nF), C.byref(M)) == 0 and int(nF.value) == F
        M = int(M.value)
        n = {**{k: M * w for k, w in SHAPES.items()}, **{k: F * w for k, w in PER_PATH.items()}, "tick_first": F + 1}
        guard = lambda k: GUARD_F64 if k not in DTYPE else GUARD_U8 if DTYPE[k] == "uint8" else GUARD_I32
        if host:
            buf = {k: np.full(n[k] + 1, guard(k), dtype=DTYPE.get(k, "float64")) for k in ORDER}
            ty = {"float64": C.c_double, "int32": C.c_int32, "uint8": C.c_uint8}
            assert L.ccmp_jerk_setpoints_copy_host(h, *[buf[k].ctypes.data_as(C.POINTER(ty[DTYPE.get(k, "float64")])) for k in ORDER]) == 0
            hostbuf = buf
        else:
            buf = {k: torch.full((n[k] + 1,), guard(k), dtype=getattr(torch, DTYPE.get(k, "float64")), device="cuda") for k in ORDER}
            assert L.ccmp_jerk_setpoints_copy(h, *[buf[k].data_ptr() for k in ORDER], None) == 0
            torch.cuda.synchronize()
            hostbuf = {k: t.cpu().numpy() for k, t in buf.items()}
    finally:
        L.ccmp_jerk_setpoints_destroy(h)
    intact = all(hostbuf[k][-1] == guard(k) for k in ORDER)
    width = {**SHAPES, **PER_PATH}
    out = {k: (hostbuf[k][:-1].reshape(-1, width[k]) if width.get(k, 1) > 1 else hostbuf[k][:-1]) for k in ORDER}
    out["ticks"] = M
    return code, out, intact


def _mirror(c, case, dev=True, scene=None, margin=0.0, **over):
    kw = dict(jc.options(case), scene=scene, margin=margin)
    kw.update(over)
    put = _dev if dev else (lambda x: x)
    return c.jerk_setpoint_paths(put(case["rows"]), put(case["path_first"]), put(case["time"]), PANDA_VMAX, PANDA_AMAX, case["jmax"], **kw)


def test_ragged_batch_everywhere(cons):
    """the chosen window: device and host forms of the C ABI and of the mirror against the restatement, and against each other"""
    ref = jc.reference()
    case, want = ref["case"], ref[0]
    code, got, intact = _guarded(cons, case)
    assert code == 0 and intact and got["ticks"] == want["ticks"]
    same_jerk(got, want, "C ABI")
    code, got_host, intact = _guarded(cons, case, host=True)
    assert code == 0 and intact
    same_jerk(got_host, want, "C ABI, host form")
    same_jerk(got_host, got, "host form against device form")
    dev = _mirror(cons, case)
    assert dev["q"].is_cuda and dev["ticks"] == want["ticks"]
    same_jerk(dev, want, "device mirror")
    host = _mirror(cons, case, dev=False)
    assert isinstance(host["q"], np.ndarray)
    same_jerk(host, want, "host mirror")
    print("ragged batch: status %s window %s passes %s ticks %s" % (got["status"].tolist(), got["window"].tolist(), got["passes"].tolist(),
                                                                    np.diff(got["tick_first"]).tolist()))
    # the device jerk peak is the P the last measure pass saw: the search stopped on it (OK: <= 1, WINDOW: > 1), and the delivered qd put
    # through the Python audit gives the same bits
    for f, name in enumerate(NAMES):
        a, b = int(got["tick_first"][f]), int(got["tick_first"][f + 1])
        if got["status"][f] in (OK, WINDOW):
            assert sc.bits(np.array([want["traces"][f][-1][1]]))[0] == sc.bits(got["peak"][f, jc.JERK:jc.JERK + 1])[0], name
            pv, pj = sc.peak_py(jc.jerk_values_py(got["qd"][a:b], case["period"], case["jmax"]))
            assert sc.bits(np.array([pv]))[0] == sc.bits(got["peak"][f, jc.JERK:jc.JERK + 1])[0] and pj == got["peak_tick"][f, jc.JERK], name
            assert (got["peak"][f, jc.JERK] <= 1.0) == (got["status"][f] == OK), name
            assert np.array_equal(sc.bits(got["tau"][a:b]), sc.bits(np.array([float(j) * case["period"] for j in range(b - a)]))), name


@pytest.mark.parametrize("window", FIXED_WINDOWS)
def test_fixed_windows(cons, window):
    """1, 2, 3 (no power of two) and max_window for every path of the batch: one measurement, passes = 0"""
    ref = jc.reference()
    case, want = ref["case"], ref[window]
    code, got, intact = _guarded(cons, case, window=window)
    assert code == 0 and intact
    same_jerk(got, want, ("C ABI", window))
    same_jerk(_mirror(cons, case, dev=False, window=window), want, ("host mirror", window))
    if window == 1:  # the setpoints unit's ticks on the grid
        sp = cons.setpoint_paths(_dev(case["rows"]), _dev(case["path_first"]), _dev(case["time"]), PANDA_VMAX, PANDA_AMAX, period=case["period"],
                                 max_ticks=case["max_ticks"])
        assert np.array_equal(sp["tick_first"].cpu().numpy(), got["tick_first"]) and sc.same_f64(sp["q"].cpu().numpy(), got["q"])
        assert sc.same_f64(sp["qd"].cpu().numpy(), got["qd"]) and sc.same_f64(sp["f"].cpu().numpy(), got["f"])


@pytest.mark.parametrize("tile_ticks", [1, 3, CASE_TILE, 0])
def test_tile_edges_do_not_show(cons, tile_ticks):
    """tile_ticks at its smallest value, at a value below the windows (a window across every tile edge), at the length the batch's tick
    counts are cut for (M = T - 1, T, T + 1, 2 T + 1) and at the default: the same bits, for the chosen window and for a fixed one"""
    ref = jc.reference()
    case = ref["case"]
    assert max(ref[0]["window"]) > 3
    same_jerk(_mirror(cons, case, tile_ticks=tile_ticks), ref[0], ("chosen", tile_ticks))
    same_jerk(_mirror(cons, case, tile_ticks=tile_ticks, window=3), ref[3], ("fixed 3", tile_ticks))
    code, got, intact = _guarded(cons, case, host=True, tile_ticks=tile_ticks, window=case["max_window"])
    assert code == 0 and intact
    same_jerk(got, ref[case["max_window"]], ("fixed max_window", tile_ticks))


def test_wide_windows_and_long_paths_against_the_host_form(cons):
    """max_window = 256 fixed (the staging kernels' LDS at its bound) and the default search on a recorded path's 3 700 ticks (many tiles
    per path), against ccmp_jerk_setpoints_ref — cheaper here than the restatement, and compared with it on the CPU"""
    from closed_chain_motion_planner_amd import jerk_setpoints_ref, timestamps_ref
    from conftest import load_path_rows

    g = load_path_rows(OBJ)
    first = np.array([0, len(g)], dtype=np.int32)
    t = timestamps_ref(g, first, PANDA_VMAX, PANDA_AMAX, 0.5)["time"]
    case = dict(rows=g, path_first=first, time=t, jmax=PANDA_JMAX, period=0.001, max_ticks=65536, max_window=64, aim=0.95)
    want = jerk_setpoints_ref(g, first, t, PANDA_VMAX, PANDA_AMAX, PANDA_JMAX)
    got = _mirror(cons, case)
    same_jerk(got, want, "recorded path", keys=("q", "qd", "tau", "tick_first", "status", "window", "passes"))
    assert sc.same_f64(got["peak"].cpu().numpy()[:, :3], want["peak"]) and np.array_equal(got["peak_tick"].cpu().numpy()[:, :3], want["peak_tick"])
    assert want["status"].tolist() == [OK] and want["window"][0] > 1
    ref = jc.reference()["case"]
    wide = dict(ref, max_window=256, max_ticks=600)
    for tile_ticks in (0, 5):
        want = jerk_setpoints_ref(wide["rows"], wide["path_first"], wide["time"], PANDA_VMAX, PANDA_AMAX, wide["jmax"], window=256, **jc.options(wide))
        got = _mirror(cons, wide, window=256, tile_ticks=tile_ticks)
        same_jerk(got, want, ("window 256", tile_ticks), keys=("q", "qd", "tau", "tick_first", "status", "window", "passes"))
        assert sc.same_f64(got["peak"].cpu().numpy()[:, :3], want["peak"]) and np.array_equal(got["peak_tick"].cpu().numpy()[:, :3], want["peak_tick"])
        assert (want["window"][np.isin(want["status"], (OK, WINDOW))] == 256).all() and OK in want["status"].tolist()


def test_scene(cons):
    """with a proxy scene at the setpoints tests' 4 ms case: f, satisfied, clearance, n_off, n_below and their peaks are the det oracle's on
    the expected filtered ticks"""
    from closed_chain_motion_planner_amd import ProxyScene

    case = jc.reference()["scene"]
    want = case["want"]
    scene = ProxyScene(cons, *case["scene"])
    code, got, intact = _guarded(cons, case, scene, case["margin"])
    assert code == 0 and intact
    same_jerk(got, want, "scene, C ABI")
    same_jerk(_mirror(cons, case, scene=scene, margin=case["margin"]), want, "scene, device mirror")
    same_jerk(_mirror(cons, case, dev=False, scene=scene, margin=case["margin"]), want, "scene, host mirror")
    print("scene: window %d after %d passes, peaks %s at %s, counts %s" % (got["window"][0], got["passes"][0], got["peak"][0].tolist(), got["peak_tick"][0].tolist(),
                                                                         got["counts"][0].tolist()))


@pytest.mark.parametrize("model", ["tilted", "calibrated"])
def test_arm_models(gpu_ctx, oracle_det, model):
    """the per-tick launchers are the only model-dependent part: the 17-row path of the batch (M = T ticks) under a calibrated arm and under a
    tilted base, f, satisfied and their peaks the det oracle's under that model"""
    case = jc.one_path(jc.reference()["case"], "m_tile")
    c = _constraint(A.OBJ, gpu_ctx, mode=1)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        want = jc.jerk_py(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, case["jmax"], O=oracle_det, P=P, **jc.options(case))
        stock = jc.reference()[0]
        f = NAMES.index("m_tile")
        assert want["ticks"] == CASE_TILE and not sc.same_f64(want["f"], stock["f"][stock["tick_first"][f]:stock["tick_first"][f + 1]])  # the model changes the gap
        same_jerk(_mirror(c, case), want, (model, "device"))
        same_jerk(_mirror(c, case, dev=False), want, (model, "host"))


def test_defaults_an_empty_call_and_errors_leave_no_handle(cons):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, _lib

    ref = jc.reference()
    case = jc.one_path(ref["case"], "three")
    want = jc.jerk_py(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, PANDA_JMAX)  # 1 ms, 65 536 ticks, max_window 64, aim 0.95
    for host in (False, True):
        code, got, intact = _guarded(cons, case, host=host, opts=False)
        assert code == 0 and intact
        same_jerk(got, want, ("defaults", host), keys=("q", "qd", "tau", "tick_first", "status", "window", "passes"))
        assert sc.same_f64(got["peak"][:, :3], want["peak"])
    empty = dict(case, rows=np.zeros((0, 14)), path_first=np.array([0], dtype=np.int32), time=np.zeros(0))
    for host in (False, True):
        code, got, intact = _guarded(cons, empty, host=host)  # F == 0: an empty result
        assert code == 0 and intact and got["ticks"] == 0 and got["tick_first"].tolist() == [0] and len(got["status"]) == 0
    nan, inf = float("nan"), float("inf")
    for host in (False, True):
        for bad in (0.0, -2.0, nan, inf):
            lim = list(PANDA_JMAX)
            lim[5] = bad
            for kw in (dict(vmax=lim), dict(amax=lim), dict(jmax=lim), dict(period=bad)):
                code, _, no_handle = _guarded(cons, case, host=host, **kw)
                assert code == EINVAL and no_handle, (host, kw)
        for kw in (dict(max_ticks=1), dict(window=-1), dict(window=9), dict(max_window=0), dict(max_window=257), dict(aim=0.0), dict(aim=1.5), dict(aim=nan),
                   dict(tile_ticks=-1)):
            code, _, no_handle = _guarded(cons, case, host=host, **kw)
            assert code == EINVAL and no_handle, (host, kw)
    # path_first: the host form checks it; the device form never reads such a path and answers EMPTY
    for bad in ([-1, 3], [0, 4], [2, 1]):
        wrong = dict(case, path_first=np.array(bad, dtype=np.int32))
        code, _, no_handle = _guarded(cons, wrong, host=True)
        assert code == EINVAL and no_handle, bad
        with pytest.raises(CcmpError) as e:
            _mirror(cons, wrong, dev=False)
        assert e.value.code == EINVAL, bad
        code, got, intact = _guarded(cons, wrong)
        assert code == 0 and intact and got["status"].tolist() == [EMPTY] and got["ticks"] == 0 and got["peak_tick"].tolist() == [[-1] * 6] and got["window"].tolist() == [0], bad
    # NULL pointers
    L = _lib.lib()
    v, a, j = ((C.c_double * 14)(*x) for x in (PANDA_VMAX, PANDA_AMAX, PANDA_JMAX))
    d_rows, d_first, d_time = _dev(case["rows"]), _dev(case["path_first"]), _dev(case["time"])
    args = [cons.ctx.handle, C.byref(cons.problem), None, 0.0, d_rows.data_ptr(), d_first.data_ptr(), d_time.data_ptr(), 1, 3, v, a, j, None]
    for k in (1, 4, 5, 6, 9, 10, 11):  # a NULL problem, rows, path_first, time, vmax, amax, jmax
        bad, h = list(args), C.c_void_p(1)
        bad[k] = None
        assert L.ccmp_path_jerk_setpoints(*bad, C.byref(h), None) == EINVAL and not h.value, k
    assert L.ccmp_path_jerk_setpoints(*args, None, None) == EINVAL  # no out
    torch.cuda.synchronize()


def test_executable_solution_with_jmax(cons):
    """... -> time stamps -> jerk-bounded setpoints and audit: with jmax the setpoints are this unit's, equal to the unit called by hand on the
    same rows and stamps; without jmax the return value is what it was"""
    from closed_chain_motion_planner_amd import PANDA_JERK_LIMITS, Roadmap, jerk_setpoints_ref
    from dense_path_cases import recorded_roadmap

    c = cons
    jmax = PANDA_JERK_LIMITS * 2
    assert tuple(jmax) == tuple(PANDA_JMAX)
    nodes, uv = recorded_roadmap()
    rm = Roadmap(c, capacity_hint=4)
    try:
        rm.append(_dev(nodes))
        assert rm.add_edges(_dev(uv)) == 0
        plain = rm.executable_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True)
        jerked = rm.executable_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True, jmax=jmax)
        narrow = rm.executable_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True, jmax=jmax, jerk_window=2, jerk_max_window=4)
    finally:
        rm.close()
    assert len(plain) == 8 and len(jerked) == 8 and "stretch" in plain[0] and "window" not in plain[0] and plain[0]["peak"].shape[1] == 5
    sp, duration, _, sampled, stamps = jerked[:5]
    assert duration == plain[1] and sc.same_f64(stamps["time"].cpu().numpy(), plain[4]["time"].cpu().numpy())
    by_hand = c.jerk_setpoint_paths(sampled["joints"], sampled["path_first"], stamps["time"], PANDA_VMAX, PANDA_AMAX, jmax)
    same_jerk(sp, {k: v.cpu().numpy() for k, v in by_hand.items() if hasattr(v, "cpu")}, "executable solution against the unit by hand")
    rows, first, time = (x.cpu().numpy() for x in (sampled["joints"], sampled["path_first"], stamps["time"]))
    want = jerk_setpoints_ref(rows, first, time, PANDA_VMAX, PANDA_AMAX, jmax)
    same_jerk(sp, want, "executable solution against the host form", keys=("q", "qd", "tau", "tick_first", "status", "window", "passes"))
    got = {k: v.cpu().numpy() for k, v in sp.items() if hasattr(v, "cpu")}
    assert sc.same_f64(got["peak"][:, :3], want["peak"]) and got["status"].tolist() == [OK] and got["window"][0] > 1
    assert sp["ticks"] == plain[0]["ticks"] + got["window"][0] - 1
    fixed = {k: v.cpu().numpy() for k, v in narrow[0].items() if hasattr(v, "cpu")}
    assert fixed["window"].tolist() == [2] and fixed["passes"].tolist() == [0] and narrow[0]["ticks"] == plain[0]["ticks"] + 1
    print("executable solution with jmax: window %d after %d passes, %d -> %d ticks, peaks %s (before: %s)" % (
        got["window"][0], got["passes"][0], plain[0]["ticks"], sp["ticks"], got["peak"][0].tolist(), plain[0]["peak"].cpu().numpy()[0].tolist()))
