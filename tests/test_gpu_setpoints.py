"""Controller-rate setpoints and the execution audit on the device (ccmp_path_setpoints / _host: the setpoints_* kernels around the function,
is-satisfied and clearance launchers) through the C ABI and both mirror forms.  Expected values are never the code under test: the
plain-Python restatement of tests/setpoint_cases.py for q, qd, tau and the audit, the det oracle's `function`, `is_satisfied` and
`clearance` applied to the expected setpoints for f, satisfied and the clearance — computed once (setpoint_cases.reference) and shared.
Comparisons are bit for bit.  Calls through the C ABI give every destination a guard element that must survive.

What each batch is for is asserted on the CPU in tests/test_setpoint_cases.py; the mutations tried against the rule are listed in
tests/test_setpoints_ref.py — the kernels compile the same header."""
import ctypes as C

import numpy as np
import pytest

import setpoint_cases as sc
from dense_path_cases import RECORDED
from setpoint_cases import PANDA_AMAX, PANDA_VMAX, same_setpoints
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
EINVAL = -1
GUARD_F64, GUARD_I32, GUARD_U8 = -7.0, -77, 177
SHAPES = {"q": 14, "qd": 14, "tau": 1, "f": 2, "satisfied": 1, "clearance": 1}  # per tick
PER_PATH = {"status": 1, "peak": 5, "peak_tick": 5, "counts": 2, "stretch": 1}
ORDER = ("q", "qd", "tau", "tick_first", "f", "satisfied", "clearance", "status", "peak", "peak_tick", "counts", "stretch")
DTYPE = {"tick_first": "int32", "satisfied": "uint8", "status": "int32", "peak_tick": "int32", "counts": "int32"}


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def cons(gpu_ctx, oracle_det):
    """the constraint whose problem is the one of setpoint_cases.reference()"""
    c = _constraint(OBJ, gpu_ctx, 1)
    c.problem.delta = RECORDED[OBJ]["delta"]
    assert bytes(_oracle_problem(oracle_det, c)) == bytes(sc.reference()["P"])
    return c


def _guarded(c, case, scene=None, margin=0.0, period=None, max_ticks=None, opts=True, vmax=PANDA_VMAX, amax=PANDA_AMAX, host=False):
    """ccmp_path_setpoints (or _host) and ccmp_setpoints_copy through the C ABI: every destination one element longer than the result,
    pre-filled with a guard value.  Returns (rc, outputs without the guard or None, every guard survived / no handle on an error)."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    L, h = _lib.lib(), C.c_void_p(1)
    rows, first, time = case["rows"], case["path_first"], case["time"]
    F, R = len(first) - 1, len(rows)
    o = _lib.CcmpSetpointOpts(case["period"] if period is None else period, case.get("max_ticks", 65536) if max_ticks is None else max_ticks)
    v, a = (C.c_double * 14)(*vmax), (C.c_double * 14)(*amax)
    sh = scene._h if scene is not None else None
    if host:
        r, pf, t = (np.ascontiguousarray(x) for x in (rows, first, time))
        p = lambda x, ty: x.ctypes.data_as(C.POINTER(ty)) if x.size else None
        code = L.ccmp_path_setpoints_host(c.ctx.handle, C.byref(c.problem), sh, float(margin), p(r, C.c_double), p(pf, C.c_int32), p(t, C.c_double), F, R, v, a,
                                          C.byref(o) if opts else None, C.byref(h))
    else:
        d_rows, d_first, d_time = _dev(rows), _dev(first), _dev(time)
        code = L.ccmp_path_setpoints(c.ctx.handle, C.byref(c.problem), sh, float(margin), d_rows.data_ptr() if R else None, d_first.data_ptr(),
                                     d_time.data_ptr() if R else None, F, R, v, a, C.byref(o) if opts else None, C.byref(h), None)
    if code != 0:
        return code, None, not h.value  # no handle on any error
    try:
        nF, M = C.c_size_t(0), C.c_size_t(0)
        assert L.ccmp_setpoints_info(h, C.byref(nF), C.byref(M)) == 0 and int(nF.value) == F
        M = int(M.value)
        n = {**{k: M * w for k, w in SHAPES.items()}, **{k: F * w for k, w in PER_PATH.items()}, "tick_first": F + 1}
        guard = lambda k: GUARD_F64 if k not in DTYPE else GUARD_U8 if DTYPE[k] == "uint8" else GUARD_I32
        buf = {k: torch.full((n[k] + 1,), guard(k), dtype=getattr(torch, DTYPE.get(k, "float64")), device="cuda") for k in ORDER}
        assert L.ccmp_setpoints_copy(h, *[buf[k].data_ptr() for k in ORDER], None) == 0
        torch.cuda.synchronize()
    finally:
        L.ccmp_setpoints_destroy(h)
    hostbuf = {k: t.cpu().numpy() for k, t in buf.items()}
    intact = all(hostbuf[k][-1] == guard(k) for k in ORDER)
    width = {**SHAPES, **PER_PATH}
    out = {k: (hostbuf[k][:-1].reshape(-1, width[k]) if width.get(k, 1) > 1 else hostbuf[k][:-1]) for k in ORDER}
    out["ticks"] = M
    return code, out, intact


def _everywhere(c, case, want, what, scene=None, margin=0.0):
    """the C ABI with guards (device and host forms) and both mirror forms against the expected result; the host forms against the device's"""
    kw = dict(period=case["period"], max_ticks=case.get("max_ticks", 65536), scene=scene, margin=margin)
    code, got, intact = _guarded(c, case, scene, margin)
    assert code == 0 and intact and got["ticks"] == want["ticks"], what
    same_setpoints(got, want, (what, "C ABI"))
    code, got_host, intact = _guarded(c, case, scene, margin, host=True)
    assert code == 0 and intact, what
    same_setpoints(got_host, want, (what, "C ABI, host form"))
    same_setpoints(got_host, got, (what, "host form against device form"))
    dev = c.setpoint_paths(_dev(case["rows"]), _dev(case["path_first"]), _dev(case["time"]), PANDA_VMAX, PANDA_AMAX, **kw)
    assert dev["q"].is_cuda and dev["ticks"] == want["ticks"]
    same_setpoints(dev, want, (what, "device mirror"))
    host = c.setpoint_paths(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, **kw)
    assert isinstance(host["q"], np.ndarray)
    same_setpoints(host, want, (what, "host mirror"))


@pytest.mark.parametrize("name", ["ragged", "on_the_stamp", "still", "full"])
def test_batches(cons, name):
    ref = sc.reference()[name]
    _everywhere(cons, ref["case"], ref["want"], name)
    if name == "still":
        assert ref["want"]["peak_tick"][0].tolist() == [0, 0, 0, 0, -1]
    if name == "full":
        assert ref["want"]["status"].tolist() == [sc.OK, sc.FULL, sc.OK]


def test_scene(cons):
    from closed_chain_motion_planner_amd import ProxyScene

    ref = sc.reference()["scene"]
    case = ref["case"]
    scene = ProxyScene(cons, *case["scene"])
    _everywhere(cons, case, ref["want"], "scene", scene=scene, margin=case["margin"])
    assert 0 < int(ref["want"]["peak_tick"][0, sc.CLEARANCE]) < ref["want"]["ticks"] - 1


def test_default_options_and_an_empty_call(cons):
    case = dict(sc.reference()["ragged"]["case"], period=0.001)
    code, got, intact = _guarded(cons, case, opts=False)  # opts NULL: 1 kHz, 65 536 ticks at most — the ragged batch's own period
    assert code == 0 and intact
    same_setpoints(got, sc.reference()["ragged"]["want"], "default options")
    empty = dict(rows=np.zeros((0, 14)), path_first=np.array([0], dtype=np.int32), time=np.zeros(0), period=0.001)
    for host in (False, True):
        code, got, intact = _guarded(cons, empty, host=host)  # F == 0: an empty result
        assert code == 0 and intact and got["ticks"] == 0 and got["tick_first"].tolist() == [0] and len(got["status"]) == 0


def test_errors_leave_no_handle(cons):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, ProxyScene, _lib

    c = cons
    case = sc.reference()["ragged"]["case"]
    nan, inf = float("nan"), float("inf")
    for host in (False, True):
        for bad in (0.0, -2.0, nan, inf):
            lim = list(PANDA_VMAX)
            lim[5] = bad
            for kw in (dict(vmax=lim), dict(amax=lim), dict(period=bad)):
                code, _, no_handle = _guarded(c, case, host=host, **kw)
                assert code == EINVAL and no_handle, (host, kw)
        for max_ticks in (1, 0, -3):
            code, _, no_handle = _guarded(c, case, host=host, max_ticks=max_ticks)
            assert code == EINVAL and no_handle, (host, max_ticks)
    # path_first: the host form checks it; the device form never reads such a path and answers EMPTY
    for bad in ([-1, 3], [0, 3, 2], [0, len(case["rows"]) + 1]):
        wrong = dict(case, path_first=np.array(bad, dtype=np.int32))
        code, _, no_handle = _guarded(c, wrong, host=True)
        assert code == EINVAL and no_handle, bad
        with pytest.raises(CcmpError) as e:
            c.setpoint_paths(case["rows"], wrong["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX)
        assert e.value.code == EINVAL, bad
        code, got, intact = _guarded(c, wrong)
        assert code == 0 and intact and sc.EMPTY in got["status"].tolist(), bad
    code, got, intact = _guarded(c, dict(case, path_first=np.array([0, len(case["rows"]) + 1], dtype=np.int32)))
    assert code == 0 and intact and got["status"].tolist() == [sc.EMPTY] and got["ticks"] == 0 and got["peak_tick"].tolist() == [[-1] * 5]
    # NULL pointers, a NaN margin with a scene
    L = _lib.lib()
    v, a = (C.c_double * 14)(*PANDA_VMAX), (C.c_double * 14)(*PANDA_AMAX)
    d_rows, d_first, d_time = _dev(case["rows"]), _dev(case["path_first"]), _dev(case["time"])
    F, R = len(case["path_first"]) - 1, len(case["rows"])
    args = [c.ctx.handle, C.byref(c.problem), None, 0.0, d_rows.data_ptr(), d_first.data_ptr(), d_time.data_ptr(), F, R, v, a, None]
    for k in (1, 4, 5, 6, 9, 10):  # a NULL problem, rows, path_first, time, vmax, amax
        bad, h = list(args), C.c_void_p(1)
        bad[k] = None
        assert L.ccmp_path_setpoints(*bad, C.byref(h), None) == EINVAL and not h.value, k
    assert L.ccmp_path_setpoints(*args, None, None) == EINVAL  # no out
    scene = ProxyScene(c, *sc.reference()["scene"]["case"]["scene"])
    h = C.c_void_p(1)
    bad = list(args)
    bad[2], bad[3] = scene._h, nan
    assert L.ccmp_path_setpoints(*bad, C.byref(h), None) == EINVAL and not h.value
    torch.cuda.synchronize()


def test_executable_solution(cons):
    """solution -> shortcut -> smooth -> densify -> resample -> time stamps -> setpoints and audit, and the audit of the result"""
    from closed_chain_motion_planner_amd import Roadmap
    from dense_path_cases import recorded_roadmap

    c = cons
    nodes, uv = recorded_roadmap()
    rm = Roadmap(c, capacity_hint=4)
    try:
        rm.append(_dev(nodes))
        assert rm.add_edges(_dev(uv)) == 0
        sp, duration, idx, sampled, stamps, dense, sm, sc_ = rm.executable_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True)
    finally:
        rm.close()
    rows, first, time = (x.cpu().numpy() for x in (sampled["joints"], sampled["path_first"], stamps["time"]))
    want = sc.setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX)
    same_setpoints(sp, want, "executable solution", keys=("q", "qd", "tau", "tick_first", "status"))
    got = {k: v.cpu().numpy() for k, v in sp.items() if hasattr(v, "cpu")}
    assert got["status"].tolist() == [sc.OK] and sp["ticks"] == sc.count_py(duration, 0.001) and got["tau"][-1] == duration
    assert sc.same_f64(got["peak"][:, :2], want["peak"]) and np.array_equal(got["peak_tick"][:, :2], want["peak_tick"]) and sc.same_f64(got["stretch"], want["stretch"])
    print("executable solution: %d ticks, peaks %s at %s, stretch %.3f, off %d" % (sp["ticks"], got["peak"][0].tolist(), got["peak_tick"][0].tolist(),
                                                                                   got["stretch"][0], got["counts"][0, 0]))
