"""Resample and time stamps on the device (ccmp_path_resample: the resample_* kernels around ONE projector call and the dense unit's arc
kernel; ccmp_path_timestamps / _host: the retime_* kernels) through the C ABI and both mirror forms, in both Jacobian modes.  Expected
values are never the code under test: the plain-Python restatement of tests/retime_cases.py on the det oracle's discrete_geodesic,
interpolate and project, with distances in the library's rounding, computed once per mode (retime_cases.reference) and shared.
Comparisons are bit for bit: rows, kinds, counts, status, path_first, arcs, lengths; ceilings x, envelopes y, times t and durations.
Calls through the C ABI give every output a guard element that must survive.

What each batch is for is asserted on the CPU in tests/test_retime_cases.py.  A DEGENERATE row (a target arc that is not > 0) needs a path
whose whole length is a subnormal number; no batch has one, the status is covered by ccmp_resample_targets_ref on the CPU alone.

Mutation check: the kernels compile the rule text of csrc/ccmp_retime.h that tests/test_retime_ref.py mutates on the CPU (see there); of
this file's own cases, a bracket with `>` for `>=` differs on no batch here (no target is a dense arc), which is why the CPU test adds
such targets."""
import ctypes as C

import numpy as np
import pytest

import retime_cases as rc
from dense_path_cases import RECORDED
from retime_cases import PANDA_AMAX, PANDA_VMAX, same_f64, same_sampled, same_stamps
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
EINVAL = -1
GUARD_F64, GUARD_I32, GUARD_U8 = -7.0, -77, 177
MODES = [0, 1]


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def cons(gpu_ctx, oracle_det):
    """one constraint per Jacobian mode at the delta the fixture's path was recorded with: the problem of retime_cases.reference(mode)"""
    made = {}

    def get(mode):
        if mode not in made:
            c = _constraint(OBJ, gpu_ctx, mode)
            c.problem.delta = RECORDED[OBJ]["delta"]
            assert bytes(_oracle_problem(oracle_det, c)) == bytes(rc.reference(mode)["P"])
            made[mode] = c
        return made[mode]

    return get


def _dense(c, case, device=True, distinct=False):
    pj, pl = case["pj"], case["pl"]
    return c.densify_paths(_dev(pj) if device else pj, _dev(pl) if device else pl, distinct=distinct, keep_handle=True)


def _same_dense(got, want):
    g = got["joints"].cpu().numpy() if hasattr(got["joints"], "cpu") else got["joints"]
    assert same_f64(g, want["rows"]) and np.array_equal(np.asarray(got["path_first"].cpu() if hasattr(got["path_first"], "cpu") else got["path_first"]), want["path_first"])


def _resample_guarded(c, dense, opts):
    """ccmp_path_resample and ccmp_sampled_paths_copy through the C ABI: every destination one element longer than the result, pre-filled
    with a guard value.  Returns (rc, outputs without the guard or None, every guard survived)."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    L, h = _lib.lib(), C.c_void_p(1)
    o = _lib.CcmpResampleOpts(*opts)
    code = L.ccmp_path_resample(c.ctx.handle, C.byref(c.problem), dense["handle"]._h, C.byref(o), C.byref(h), None)
    if code != 0:
        return code, None, not h.value  # no handle on any error
    try:
        F, R = C.c_size_t(0), C.c_size_t(0)
        assert L.ccmp_sampled_paths_info(h, C.byref(F), C.byref(R)) == 0
        F, R = int(F.value), int(R.value)
        full = lambda n, dt, v: torch.full((n + 1,), v, dtype=dt, device="cuda")
        buf = {"joints": full(R * 14, torch.float64, GUARD_F64), "path_first": full(F + 1, torch.int32, GUARD_I32), "arc": full(R, torch.float64, GUARD_F64),
               "length": full(F, torch.float64, GUARD_F64), "kind": full(R, torch.uint8, GUARD_U8), "status": full(F, torch.int32, GUARD_I32),
               "counts": full(F * 4, torch.int32, GUARD_I32)}
        assert L.ccmp_sampled_paths_copy(h, *[b.data_ptr() for b in buf.values()], None) == 0
        torch.cuda.synchronize()
    finally:
        L.ccmp_sampled_paths_destroy(h)
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    intact = all(host[k][-1] == {np.float64: GUARD_F64, np.int32: GUARD_I32, np.uint8: GUARD_U8}[host[k].dtype.type] for k in host)
    shapes = {"joints": (R, 14), "counts": (F, 4)}
    return code, {k: host[k][:-1].reshape(shapes.get(k, (-1,))) for k in host}, intact


def _stamps_guarded(c, rows, first, vmax=PANDA_VMAX, amax=PANDA_AMAX, beta=0.5, profile=True, total_rows=None):
    """ccmp_path_timestamps through the C ABI with guard elements.  Returns (rc, outputs without the guard, guards survived, raw buffers)."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    R, F = (len(rows) if total_rows is None else total_rows), len(first) - 1
    full = lambda n, dt, v: torch.full((n + 1,), v, dtype=dt, device="cuda")
    buf = {"time": full(R, torch.float64, GUARD_F64), "duration": full(F, torch.float64, GUARD_F64), "ceiling": full(R, torch.float64, GUARD_F64),
           "envelope": full(R, torch.float64, GUARD_F64), "status": full(F, torch.int32, GUARD_I32)}
    v, a = (C.c_double * 14)(*vmax), (C.c_double * 14)(*amax)
    d_rows, d_first = _dev(rows), _dev(first)
    ptr = lambda k: buf[k].data_ptr() if profile or k not in ("ceiling", "envelope") else None
    code = _lib.lib().ccmp_path_timestamps(c.ctx.handle, d_rows.data_ptr(), d_first.data_ptr(), F, R, v, a, float(beta), *[ptr(k) for k in buf], None)
    torch.cuda.synchronize()
    host = {k: t.cpu().numpy() for k, t in buf.items()}
    intact = all(host[k][-1] == (GUARD_F64 if host[k].dtype == np.float64 else GUARD_I32) for k in host)
    return code, {k: host[k][:-1] for k in host}, intact, host


def _untouched(raw):
    return all((v == (GUARD_F64 if v.dtype == np.float64 else GUARD_I32)).all() for v in raw.values())


def _stamps_everywhere(c, rows, first, what, beta=0.5):
    """the C ABI with guards (with and without the profile outputs), the device mirror and the host mirror against the restatement"""
    want = rc.timestamps_py(rows, first, PANDA_VMAX, PANDA_AMAX, beta, fill=GUARD_F64)
    code, got, intact, _ = _stamps_guarded(c, rows, first, beta=beta)
    assert code == 0 and intact, what
    same_stamps(got, want, (what, "C ABI"))
    code, got, intact, raw = _stamps_guarded(c, rows, first, beta=beta, profile=False)  # ceiling and envelope in the context's workspace
    assert code == 0 and intact and (raw["ceiling"] == GUARD_F64).all() and (raw["envelope"] == GUARD_F64).all(), what
    same_stamps(got, want, (what, "C ABI, no profile"), keys=("time", "duration"))
    want0 = rc.timestamps_py(rows, first, PANDA_VMAX, PANDA_AMAX, beta, fill=0.0)  # the mirror's outputs start as zeros
    same_stamps(c.timestamp_paths(_dev(rows), _dev(first), PANDA_VMAX, PANDA_AMAX, beta=beta, profile=True), want0, (what, "device"))
    same_stamps(c.timestamp_paths(rows, first, PANDA_VMAX, PANDA_AMAX, beta=beta, profile=True), want0, (what, "host"))
    return want


# ---- 1. the ragged batch: every output size, count mode, both layouts, spacing mode at the same N -----------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_ragged_batch(cons, mode):
    c, ref = cons(mode), rc.reference(mode)["ragged"]
    case = ref["case"]
    dense, distinct, host_dense = _dense(c, case), _dense(c, case, distinct=True), _dense(c, case, device=False)
    try:
        _same_dense(dense, ref["dense"])
        _same_dense(distinct, ref["distinct"])
        for count in case["counts"]:
            want = ref["want"][count]
            code, got, intact = _resample_guarded(c, dense, (count, 0.0, 65536))
            assert code == 0 and intact, count
            same_sampled(got, want, (mode, count, "C ABI"))
            same_sampled(c.resample_paths(dense, count=count), want, (mode, count, "device"))
            same_sampled(c.resample_paths(distinct, count=count), want, (mode, count, "distinct layout"))  # duplicates add +0.0: the same bits
        same_sampled(c.resample_paths(host_dense, count=17), ref["want"][17], (mode, "host"))
        assert isinstance(c.resample_paths(host_dense, count=17)["joints"], np.ndarray)
        # spacing mode chosen to give the same N: one path alone, spacing = T / (count - 1.5), so ceil(T / spacing) = count - 1
        for f, count in ((4, 17), (6, 65)):
            one = dict(pj=case["pj"][f:f + 1], pl=case["pl"][f:f + 1])
            d1 = _dense(c, one)
            T = float(ref["dense"]["length"][f])
            by_count, by_spacing = c.resample_paths(d1, count=count), c.resample_paths(d1, spacing=T / (count - 1.5))
            d1["handle"].close()
            a, b = ref["want"][count]["path_first"][f], ref["want"][count]["path_first"][f + 1]
            assert by_spacing["rows"] == count and same_f64(by_count["joints"].cpu().numpy(), ref["want"][count]["joints"][a:b])
            for k in ("joints", "arc", "length", "kind", "counts", "status"):
                assert np.array_equal(by_count[k].cpu().numpy().view(np.uint8), by_spacing[k].cpu().numpy().view(np.uint8)), (f, k)
    finally:
        for d in (dense, distinct, host_dense):
            d["handle"].close()
    rows, first = ref["rows"]
    want = _stamps_everywhere(c, rows, first, ("ragged", mode))
    assert want["status"].tolist() == [rc.EMPTY] + [rc.OK] * 6


# ---- 2. the wide batch: spacing mode, every status --------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_wide_batch(cons, mode):
    c, ref = cons(mode), rc.reference(mode)["wide"]
    case, want = ref["case"], ref["want"]
    dense = _dense(c, case)
    try:
        _same_dense(dense, ref["dense"])
        code, got, intact = _resample_guarded(c, dense, (0, case["spacing"], case["max_rows"]))
        assert code == 0 and intact
        same_sampled(got, want, (mode, "C ABI"))
        same_sampled(c.resample_paths(dense, spacing=case["spacing"], max_rows=case["max_rows"]), want, (mode, "device"))
    finally:
        dense["handle"].close()
    _stamps_everywhere(c, want["joints"], want["path_first"], ("wide", mode), beta=0.2)


# ---- 3. the long path: three chunks of the stamps; a captured call ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_long_path(cons, mode):
    import torch

    c, ref = cons(mode), rc.reference(mode)["long"]
    dense = _dense(c, ref["case"])
    try:
        got = c.resample_paths(dense, count=ref["case"]["count"])
    finally:
        dense["handle"].close()
    same_sampled(got, ref["want"], (mode, "device"))
    rows, first = ref["want"]["joints"], ref["want"]["path_first"]
    want = _stamps_everywhere(c, rows, first, ("long", mode))
    assert want["duration"][0] > 0.0
    if mode == 0:  # captured into a HIP graph (after the eager calls above, which grew the context's workspace) and replayed once
        d_rows, d_first = got["joints"], got["path_first"]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = c.timestamp_paths(d_rows, d_first, PANDA_VMAX, PANDA_AMAX, profile=True)
        for t in out.values():
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        same_stamps(out, rc.timestamps_py(rows, first, PANDA_VMAX, PANDA_AMAX, fill=0.0), "graph replay")


# ---- 4. every projection fails: the fallback rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_fallback_case(cons, gpu_ctx, oracle_det, mode):
    c, case = cons(mode), rc.reference(mode)["fallback"]["case"]
    strict = _constraint(OBJ, gpu_ctx, mode)
    strict.problem.delta = RECORDED[OBJ]["delta"]
    strict.setTolerance(case["tolerance"], case["tolerance"])
    assert bytes(_oracle_problem(oracle_det, strict)) == bytes(rc.strict_problem(rc.reference(mode)["P"]))
    dense = _dense(c, case)  # the dense path is made with the stock tolerances
    try:
        same_sampled(strict.resample_paths(dense, count=case["count"]), case["want"], (mode, "fallback"))
    finally:
        dense["handle"].close()
    _stamps_everywhere(c, case["want"]["joints"], case["want"]["path_first"], ("fallback", mode))


# ---- 5. repeated states; non-finite and empty paths -------------------------------------------------------------------------------------
def test_still_rows_and_statuses(cons):
    c = cons(0)
    rows, first = rc.still_rows()
    want = _stamps_everywhere(c, rows, first, "still")
    assert np.isinf(want["ceiling"]).any() and (want["duration"][[1, 2, 5]] == 0.0).all()
    r, f = rc.reference(0)["ragged"]["rows"]
    rows = np.vstack([r[f[4]:f[5]], r[f[3]:f[4]], r[f[4]:f[5]], r[f[2]:f[3]]])
    rows[17 + 1, 3], rows[17 + 3 + 5, 0] = np.nan, np.inf
    first = np.array([0, 0, 17, 20, 20, 37, 39, 39], dtype=np.int32)
    want = _stamps_everywhere(c, rows, first, "statuses")
    assert want["status"].tolist() == [rc.EMPTY, rc.OK, rc.NONFINITE, rc.EMPTY, rc.NONFINITE, rc.OK, rc.EMPTY]


# ---- 6. error paths leave the outputs untouched --------------------------------------------------------------------------------------------
def test_errors_leave_outputs_untouched(cons):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, _lib

    c, ref = cons(0), rc.reference(0)["ragged"]
    rows, first = ref["rows"]
    nan, inf = float("nan"), float("inf")
    bad_limits = [list(PANDA_VMAX) for _ in range(4)]
    for lim, v in zip(bad_limits, (0.0, -2.0, nan, inf)):
        lim[5] = v
    for lim in bad_limits:
        for kw in (dict(vmax=lim), dict(amax=lim)):
            code, _, _, raw = _stamps_guarded(c, rows, first, **kw)
            assert code == EINVAL and _untouched(raw), kw
    for beta in (0.0, 1.0, -0.1, nan):
        code, _, _, raw = _stamps_guarded(c, rows, first, beta=beta)
        assert code == EINVAL and _untouched(raw), beta
    for bad in ([-1, 3], [0, 3, 2], [0, len(rows) + 1]):  # the host form checks path_first; the device form never reads such a path
        with pytest.raises(CcmpError) as e:
            c.timestamp_paths(rows, np.array(bad, dtype=np.int32), PANDA_VMAX, PANDA_AMAX)
        assert e.value.code == EINVAL, bad
        code, got, intact, _ = _stamps_guarded(c, rows, np.array(bad, dtype=np.int32))
        assert code == 0 and intact and (got["time"][3:] == GUARD_F64).all(), bad
    code, got, intact, _ = _stamps_guarded(c, rows, np.array([0, len(rows) + 1], dtype=np.int32))
    assert code == 0 and got["status"].tolist() == [rc.EMPTY] and (got["time"] == GUARD_F64).all()
    L = _lib.lib()
    v, a = (C.c_double * 14)(*PANDA_VMAX), (C.c_double * 14)(*PANDA_AMAX)
    assert L.ccmp_path_timestamps(c.ctx.handle, None, None, 0, 0, v, a, 0.5, None, None, None, None, None, None) == 0  # F == 0 touches nothing
    t = torch.zeros(4, dtype=torch.float64, device="cuda")
    s = torch.zeros(4, dtype=torch.int32, device="cuda")
    args = [c.ctx.handle, t.data_ptr(), s.data_ptr(), 1, 0, v, a, 0.5, t.data_ptr(), t.data_ptr(), None, None, s.data_ptr(), None]
    for k in (2, 9, 12):  # a NULL path_first, duration, status
        bad = list(args)
        bad[k] = None
        assert L.ccmp_path_timestamps(*bad) == EINVAL, k
    assert L.ccmp_path_timestamps(*(args[:4] + [1, v, a, 0.5, None] + args[9:])) == EINVAL  # rows exist but no time
    # resample: bad options give no handle
    dense = _dense(c, dict(pj=ref["case"]["pj"][2:3], pl=ref["case"]["pl"][2:3]))
    try:
        for opts in ((1, 0.25, 65536), (-3, 0.25, 65536), (0, 0.0, 65536), (0, -1.0, 65536), (0, nan, 65536), (5, 0.25, 1), (0, 0.25, 0)):
            code, _, no_handle = _resample_guarded(c, dense, opts)
            assert code == EINVAL and no_handle, opts
        h = C.c_void_p(1)
        assert L.ccmp_path_resample(c.ctx.handle, C.byref(c.problem), None, None, C.byref(h), None) == EINVAL and not h.value
        assert L.ccmp_path_resample(c.ctx.handle, C.byref(c.problem), dense["handle"]._h, None, None, None) == EINVAL
        assert L.ccmp_path_resample(c.ctx.handle, None, dense["handle"]._h, None, C.byref(h), None) == EINVAL and not h.value
        with pytest.raises(CcmpError) as e:
            c.resample_paths(dense, count=1)
        assert e.value.code == EINVAL
        default = c.resample_paths(dense)  # opts of the mirror's defaults: spacing = the problem's delta
        T = float(ref["dense"]["length"][2])
        assert default["rows"] == rc.count_py(T, 0, c.problem.delta)
    finally:
        dense["handle"].close()
    with pytest.raises(ValueError):
        c.resample_paths(dense)  # a closed handle
    empty = c.densify_paths(_dev(ref["case"]["pj"][:0]), _dev(ref["case"]["pl"][:0]), keep_handle=True)  # F == 0: an empty result
    try:
        got = c.resample_paths(empty)
        assert got["rows"] == 0 and got["path_first"].cpu().tolist() == [0] and got["status"].numel() == 0
    finally:
        empty["handle"].close()


# ---- 7. solution -> shortcut -> smooth -> densify -> resample -> time stamps -------------------------------------------------------------
def test_timed_solution(cons):
    from closed_chain_motion_planner_amd import PANDA_ACCELERATION_LIMITS, PANDA_VELOCITY_LIMITS, Roadmap
    from dense_path_cases import recorded_roadmap

    c = cons(0)
    assert tuple(PANDA_VELOCITY_LIMITS) * 2 == PANDA_VMAX and tuple(PANDA_ACCELERATION_LIMITS) * 2 == PANDA_AMAX
    nodes, uv = recorded_roadmap()
    rm = Roadmap(c, capacity_hint=4)
    try:
        rm.append(_dev(nodes))
        assert rm.add_edges(_dev(uv)) == 0
        duration, idx, sampled, stamps, dense, sm, sc = rm.timed_solution(c, [0, 1], [9, 6], PANDA_VMAX, PANDA_AMAX, max_steps=2, distinct=True)
        _, idx2, dense2, _, _ = rm.dense_smooth_solution(c, [0, 1], [9, 6], max_steps=2, distinct=True, keep_handle=True)
        try:
            ref = c.resample_paths(dense2)
        finally:
            dense2["handle"].close()
        assert np.array_equal(idx, idx2) and "handle" not in dense and int(sampled["status"][0]) == rc.OK and sampled["rows"] >= 2
        for k in ("joints", "arc", "kind"):
            assert np.array_equal(sampled[k].cpu().numpy().view(np.uint8), ref[k].cpu().numpy().view(np.uint8)), k
        rows = sampled["joints"].cpu().numpy()
        want = rc.timestamps_py(rows, sampled["path_first"].cpu().numpy(), PANDA_VMAX, PANDA_AMAX, fill=0.0)
        same_stamps(stamps, want, "timed solution", keys=("time", "duration"))
        assert duration == float(want["duration"][0]) > 0.0
        # even arc: the spread of the resampled steps is far below that of the dense rows it came from
        step, dense_step = np.diff(sampled["arc"].cpu().numpy()), np.diff(dense["arc"].cpu().numpy())
        assert step.max() / step.min() < dense_step.max() / dense_step[dense_step > 0].min()
    finally:
        rm.close()
