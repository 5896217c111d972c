"""The host-only forms of the setpoint rule (ccmp_setpoints_ref, ccmp_setpoint_tangents_ref: the text of csrc/ccmp_setpoints.h compiled for
the host, no device) bit for bit against the plain-Python restatement of tests/setpoint_cases.py, on every batch of that module and on the
reference's two recorded path files under the time stamps of retime_cases.timestamps_py; then the three properties the rule guarantees by
construction, every status, every argument error and the two-call sizing.

Mutations tried against the rule.  They are made in the RESTATEMENT (setpoint_cases.setpoints_py(..., mutate=...)), not in the library's
sources: test_mutations_are_caught asserts, for each, on which batch the wrong rule stops agreeing with the library — the same comparison
that test_setpoints_match makes with the right rule, so a library carrying the mutation would turn that case red:
  * "bracket": `>` for `>=` in the bracket (csrc/ccmp_dense.h: arc_bracket)
        -> on_the_stamp, its second path: the ticks that ARE a stamp take the next interval.  The interpolant is C1, so in exact arithmetic
           both intervals answer the same q and qd there; the mutation shows only where fl(a + fl(b - a)) != b, which is why that path's
           rows are random joint vectors whose differences round (on the first path's geodesic rows the two agree bit for bit, and the
           test says so).  No other batch has a tick on a stamp: the ragged and still batches agree under the mutation
  * "tangent": a tangent without the sign test `m_{i-1} m_i > 0` (csrc/ccmp_setpoints.h: setpoint_tangent)
        -> ragged (joint slopes change sign inside the 70-row path: test_tangents_match and test_setpoints_match), and the first property
           of test_properties — the cubic overshoots its rows
  * "tau": tau_j without the `min` against D (setpoint_tau)
        -> NO case differs, and none can: an interior product fl(j period) never exceeds D (test_interior_products_never_pass_the_duration
           gives the argument and checks it on 10^4 durations around products that round either way).  The `min` stays in the rule as
           stated: it makes "tau is non-decreasing and ends at D" hold by the text alone, whatever the count rule
  * "tie": a peak that keeps the last tick of a tie (setpoint_higher / setpoint_lower)
        -> still (every tick of a path of identical rows ties on speed and acceleration: the answer must be tick 0)
"""
import ctypes as C

import numpy as np
import pytest

import retime_cases as rc
import setpoint_cases as sc
from conftest import load_path_rows
from setpoint_cases import EMPTY, FULL, NONFINITE, OK, PANDA_AMAX, PANDA_VMAX, POINT, UNORDERED

EINVAL, ENODEV = -1, -5
ULP = 2.0 ** -52
NAMES = ["ragged", "on_the_stamp", "still", "full", "scene", "golden-Wine_Bottle", "golden-dumbbell"]


@pytest.fixture(scope="module")
def ref(ccmp_built):
    return sc.reference()


def _batches(ref):
    for name in ("ragged", "on_the_stamp", "still", "full", "scene"):
        c = ref[name]["case"]
        yield name, c["rows"], c["path_first"], c["time"], c["period"], c.get("max_ticks", 65536)
    for obj in ("Wine_Bottle", "dumbbell"):
        g = load_path_rows(obj)
        first = np.array([0, len(g)], dtype=np.int32)
        yield "golden-" + obj, g, first, rc.timestamps_py(g, first, PANDA_VMAX, PANDA_AMAX)["time"], 0.001, 65536


def _case(ref, name):
    return next(b[1:] for b in _batches(ref) if b[0] == name)


@pytest.mark.parametrize("name", NAMES)
def test_setpoints_match(ref, name):
    from closed_chain_motion_planner_amd import setpoints_ref

    rows, first, time, period, max_ticks = _case(ref, name)
    want = sc.setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, period, max_ticks)
    got = setpoints_ref(rows, first, time, PANDA_VMAX, PANDA_AMAX, period=period, max_ticks=max_ticks)
    sc.same_setpoints(got, want, name)
    assert got["ticks"] == want["ticks"]
    if name in ref:  # the part of the full expected result (oracle's f and clearance included) that the host form answers
        sc.same_setpoints(got, sc.host_part(ref[name]["want"]), (name, "shared reference"))
    if name.startswith("golden"):
        print("%s at 1 ms: %d ticks, speed %.3f x vmax at tick %d, mean tick-interval acceleration %.3f x amax at tick %d, stretch %.3f" % (
            name, got["ticks"], got["peak"][0, 0], got["peak_tick"][0, 0], got["peak"][0, 1], got["peak_tick"][0, 1], got["stretch"][0]))


def _agrees(got, want):
    try:
        sc.same_setpoints(got, want)
        return True
    except AssertionError:
        return False


def test_mutations_are_caught(ref):
    """each wrong variant of the rule, made in the restatement: the batches on which it stops agreeing with the library (module docstring)"""
    from closed_chain_motion_planner_amd import setpoints_ref

    agree = {}
    for name in ("ragged", "on_the_stamp", "still", "full", "scene"):
        rows, first, time, period, max_ticks = _case(ref, name)
        got = setpoints_ref(rows, first, time, PANDA_VMAX, PANDA_AMAX, period=period, max_ticks=max_ticks)
        for m in ("bracket", "tangent", "tau", "tie"):
            agree[(m, name)] = _agrees(got, sc.setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, period, max_ticks, mutate=(m,)))
    assert not agree[("bracket", "on_the_stamp")] and agree[("bracket", "ragged")] and agree[("bracket", "still")]
    assert not agree[("tangent", "ragged")]
    assert not agree[("tie", "still")] and not agree[("tie", "ragged")]  # (ragged: the two-tick path is at rest at both of its ticks)
    assert all(agree[("tau", name)] for name in ("ragged", "on_the_stamp", "still", "full", "scene"))
    # the tangent mutation breaks the first guarantee on the ragged batch: some interior setpoint leaves the interval of its bracket rows
    rows, first, time, period, _ = _case(ref, "ragged")
    a, b = int(first[5]), int(first[6])
    q, _, _, ks = sc.path_py(rows[a:b], time[a:b], period, 17, mutate=("tangent",))
    r = rows[a:b]
    out = [j for j, k in enumerate(ks, start=1) if ((q[j] < np.minimum(r[k - 1], r[k]) - 1e-9) | (q[j] > np.maximum(r[k - 1], r[k]) + 1e-9)).any()]
    assert out, "the mutated cubic stays within its rows"


def test_interior_products_never_pass_the_duration():
    """why no case can tell tau_j = min(fl(j period), D) from fl(j period): rounding is monotone, so fl(j period) > D needs j period > D in the
    reals, then D / period < j, fl(D / period) <= j and N - 1 = ceil(fl(D / period)) <= j: such a tick is the last one or beyond, never
    interior.  Asserted on durations at, just below and just above products that round up, down and not at all"""
    rng = np.random.default_rng(0x7800)
    checked = 0
    for period in [0.001, 0.1, 2.0 ** -9, 1.0 / 3.0, 0.004] + rng.uniform(1e-4, 0.5, 40).tolist():
        for m in list(range(1, 60)) + rng.integers(60, 60000, 60).tolist():
            at = float(m) * period
            for D in (at, float(np.nextafter(at, 0.0)), float(np.nextafter(at, 1e9)), at * (1.0 + 1e-9)):
                N = sc.count_py(D, period)
                assert N >= 2 and all(float(j) * period <= D for j in range(max(N - 3, 1), N - 1)), (period, D, N)
                checked += 1
    assert checked > 10000


@pytest.mark.parametrize("name", ["ragged", "on_the_stamp", "still", "golden-Wine_Bottle"])
def test_tangents_match(ref, name):
    from closed_chain_motion_planner_amd import setpoint_tangents_ref

    rows, first, time, _, _ = _case(ref, name)
    seen = 0
    for f in range(len(first) - 1):
        a, b = int(first[f]), int(first[f + 1])
        r, t = rows[a:b], time[a:b]
        if sc.status_py(r, t, 0.001, 2 ** 30)[0] not in (OK, POINT, FULL):
            continue
        w = setpoint_tangents_ref(r, t)
        assert sc.same_f64(w, sc.tangents_py(r, t)), (name, f)
        assert (w[[0, -1]] == 0.0).all() if b > a else True
        seen += int((w != 0.0).sum())
    if name == "ragged":
        assert seen > 500
    assert setpoint_tangents_ref(rows[:0], time[:0]).shape == (0, 14)


def test_properties(ref):
    """what the rule guarantees by construction.
    1. An interior q lies between its bracket rows a = r_{k-1} and b = r_k up to the rounding of the header's expression q = fl(fl(a + p) + e),
       p = fl(s d), e = fl(fl(h fl(u v)) fl(fl(v wa) - fl(u wb))), with 0 <= s <= 1 and |e| <= h max(|wa|, |wb|) / 4.  With r = 2^-53: d = fl(b - a)
       carries r |d|; s three roundings and p one more: 5 r |d| with d's own; e's seven operations at most 7 r h max|w|; the two sums r each of
       a magnitude at most |a| + |d| + |e|.  The exact cubic is monotone (the tangents obey |w| <= 3 |m| on both sides, up to their own three
       roundings, which scale |d|), so the bound is r (2 |a| + 7 |d| + 9 h max|w|) <= 4.5 * 2^-52 (|a| + |d| + h max|w|); asserted with
       8 * 2^-52, not quite twice the derived figure.
    2. The trajectory starts and ends at rest on r_0 and r_{R-1}, bit for bit.
    3. tau is non-decreasing, starts at +0.0 and ends exactly at D; consecutive ticks are at most one period apart up to one rounding."""
    from closed_chain_motion_planner_amd import setpoints_ref

    interior = 0
    for name, rows, first, time, period, max_ticks in _batches(ref):
        got = setpoints_ref(rows, first, time, PANDA_VMAX, PANDA_AMAX, period=period, max_ticks=max_ticks)
        want = sc.setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, period, max_ticks)
        for f in range(len(first) - 1):
            if got["status"][f] != OK:
                continue
            a, b = int(first[f]), int(first[f + 1])
            r, t = rows[a:b], time[a:b]
            g0, g1 = int(got["tick_first"][f]), int(got["tick_first"][f + 1])
            q, qd, tau = got["q"][g0:g1], got["qd"][g0:g1], got["tau"][g0:g1]
            w = sc.tangents_py(r, t)
            for j, k in enumerate(want["brackets"][f], start=1):
                lo, hi = np.minimum(r[k - 1], r[k]), np.maximum(r[k - 1], r[k])
                h = float(t[k]) - float(t[k - 1])
                margin = 8 * ULP * (np.abs(r[k - 1]) + np.abs(r[k] - r[k - 1]) + h * np.maximum(np.abs(w[k - 1]), np.abs(w[k])))
                assert (q[j] >= lo - margin).all() and (q[j] <= hi + margin).all(), (name, f, j, k)
                interior += 1
            assert sc.same_f64(q[0], r[0]) and sc.same_f64(q[-1], r[-1]) and (qd[0] == 0.0).all() and (qd[-1] == 0.0).all(), (name, f)
            assert sc.bits(tau[:1])[0] == 0 and tau[-1] == t[-1] and (np.diff(tau) >= 0).all(), (name, f)
            assert (np.diff(tau) <= period * (1 + 2 * ULP) + 2 * ULP * tau[1:]).all(), (name, f)
    assert interior > 1000


def test_every_status_and_the_two_call_sizing(ref):
    from closed_chain_motion_planner_amd import SETPOINT_STATUS, _lib

    assert SETPOINT_STATUS == ("ok", "empty", "non_finite", "unordered", "point", "full")
    seen = set()
    for name in ("ragged", "full"):
        seen |= set(ref[name]["want"]["status"].tolist())
    assert seen == {OK, EMPTY, NONFINITE, UNORDERED, POINT, FULL}
    # a duration that is not > 0 is a POINT whatever the rows; a count beyond INT32_MAX is FULL
    case = ref["ragged"]["case"]
    r = case["run"][:2]
    L, v, a = _lib.lib(), (C.c_double * 14)(*PANDA_VMAX), (C.c_double * 14)(*PANDA_AMAX)

    def sizes(rows, first, time, period, max_ticks):
        rows, time, first = np.ascontiguousarray(rows), np.ascontiguousarray(time, dtype=np.float64), np.ascontiguousarray(first, dtype=np.int32)
        F = len(first) - 1
        tf, st = np.full(F + 2, -77, dtype=np.int32), np.full(F + 1, -77, dtype=np.int32)
        o = _lib.CcmpSetpointOpts(period, max_ticks)
        p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
        code = L.ccmp_setpoints_ref(p(rows, C.c_double), p(first, C.c_int32), p(time, C.c_double), F, len(rows), v, a, C.byref(o), p(tf, C.c_int32), p(st, C.c_int32),
                                    None, None, None, None, None, None)
        assert tf[-1] == -77 and st[-1] == -77  # the guard elements
        return code, tf[:-1].tolist(), st[:-1].tolist()

    assert sizes(np.vstack([r[0], r[0]]), [0, 2], [0.0, 0.0], 0.001, 65536) == (0, [0, 1], [POINT])
    assert sizes(r, [0, 2], [0.0, 1.0], 1e-10, 2 ** 31 - 1) == (0, [0, 0], [FULL])
    assert sizes(r, [0, 2], [0.0, 1.0], 5e-324, 65536) == (0, [0, 0], [FULL])  # the quotient overflows
    assert sizes(r, [0, 2], [0.0, 1e-300], 0.001, 2) == (0, [0, 2], [OK])  # a quotient that underflows towards zero: still two ticks
    assert sizes(r, [0, 2], [0.0, 0.002], 0.001, 2) == (0, [0, 0], [FULL]) and sizes(r, [0, 2], [0.0, 0.002], 0.001, 3) == (0, [0, 3], [OK])
    assert sizes(r, [0, 2], [-0.0, 0.002], 0.001, 3) == (0, [0, 3], [OK])  # t_0 = -0.0 is zero
    # the sizing call answers what the full call answers
    code, tf, st = sizes(case["rows"], case["path_first"], case["time"], case["period"], 65536)
    assert code == 0 and tf == ref["ragged"]["want"]["tick_first"].tolist() and st == ref["ragged"]["want"]["status"].tolist()


def test_argument_errors(ref):
    from closed_chain_motion_planner_amd import CcmpError, _lib, setpoint_tangents_ref, setpoints_ref

    case = ref["ragged"]["case"]
    rows, first, time = case["rows"], case["path_first"], case["time"]

    def refused(fn, *a, **k):
        with pytest.raises(CcmpError) as e:
            fn(*a, **k)
        assert e.value.code == EINVAL, (a, k)

    nan, inf = float("nan"), float("inf")
    for bad in (0.0, -1.0, nan, inf):  # a limit that is not finite and positive
        for which in (0, 13):
            v, a = list(PANDA_VMAX), list(PANDA_AMAX)
            v[which] = bad
            refused(setpoints_ref, rows, first, time, v, PANDA_AMAX)
            a[which] = bad
            refused(setpoints_ref, rows, first, time, PANDA_VMAX, a)
    for period in (0.0, -0.001, nan, inf):
        refused(setpoints_ref, rows, first, time, PANDA_VMAX, PANDA_AMAX, period=period)
    for max_ticks in (1, 0, -5):
        refused(setpoints_ref, rows, first, time, PANDA_VMAX, PANDA_AMAX, max_ticks=max_ticks)
    for pf in ([-1, 3], [0, 3, 2], [0, len(rows) + 1]):  # negative, decreasing, beyond the rows
        refused(setpoints_ref, rows, np.array(pf, dtype=np.int32), time, PANDA_VMAX, PANDA_AMAX)
    empty = setpoints_ref(rows[:0], np.array([0], dtype=np.int32), time[:0], PANDA_VMAX, PANDA_AMAX)  # F == 0
    assert empty["ticks"] == 0 and empty["tick_first"].tolist() == [0] and len(empty["status"]) == 0
    L = _lib.lib()
    v, a = (C.c_double * 14)(*PANDA_VMAX), (C.c_double * 14)(*PANDA_AMAX)
    r3, t3, pf3 = np.ascontiguousarray(rows[:3]), np.array([0.0, 0.1, 0.2]), np.array([0, 3], dtype=np.int32)
    tf, st = np.zeros(2, dtype=np.int32), np.zeros(1, dtype=np.int32)
    p = lambda x, t: x.ctypes.data_as(C.POINTER(t))
    good = [p(r3, C.c_double), p(pf3, C.c_int32), p(t3, C.c_double), 1, 3, v, a, None, p(tf, C.c_int32), p(st, C.c_int32), None, None, None, None, None, None]
    assert L.ccmp_setpoints_ref(*good) == 0 and tf.tolist() == [0, sc.count_py(0.2, 0.001)] and st.tolist() == [OK]  # opts NULL: period 0.001, 65 536 ticks at most
    for k in (0, 1, 2, 5, 6, 8, 9):  # a NULL rows, path_first, time, vmax, amax, tick_first, status
        bad = list(good)
        bad[k] = None
        assert L.ccmp_setpoints_ref(*bad) == EINVAL, k
    assert L.ccmp_setpoint_tangents_ref(None, p(t3, C.c_double), 3, p(r3, C.c_double)) == EINVAL
    assert L.ccmp_setpoint_tangents_ref(p(r3, C.c_double), None, 3, p(r3, C.c_double)) == EINVAL
    assert L.ccmp_setpoint_tangents_ref(p(r3, C.c_double), p(t3, C.c_double), 3, None) == EINVAL
    with pytest.raises(ValueError):
        setpoint_tangents_ref(rows[:3], time[:2])
    # without a context: no device here -> CCMP_ENODEV, a device -> CCMP_EINVAL; either way before anything else is looked at
    out = C.c_void_p(1)
    assert L.ccmp_path_setpoints(None, None, None, 0.0, None, None, None, 0, 0, None, None, None, C.byref(out), None) in (ENODEV, EINVAL) and not out.value
    out = C.c_void_p(1)
    assert L.ccmp_path_setpoints_host(None, None, None, 0.0, None, None, None, 0, 0, None, None, None, C.byref(out)) in (ENODEV, EINVAL) and not out.value
    assert L.ccmp_setpoints_copy(None, *[None] * 13) in (ENODEV, EINVAL) and L.ccmp_setpoints_copy_host(None, *[None] * 12) in (ENODEV, EINVAL)
    assert L.ccmp_setpoints_info(None, None, None) == EINVAL
    L.ccmp_setpoints_destroy(None)
    o = _lib.CcmpSetpointOpts()
    L.ccmp_setpoint_opts_default(C.byref(o))
    assert (o.period, o.max_ticks) == (0.001, 65536)
