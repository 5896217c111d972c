"""Jerk-bounded setpoints: a plain-Python restatement of the rule of csrc/ccmp_jerk.h and the expected values the tests compare with.

The expected values are never the code under test.  The rule is restated here in Python floats (IEEE doubles, one rounding per operation,
nothing fused) on top of setpoint_cases.path_py, which restates the interpolant:

    input        x_0 .. x_n = path_py's ticks of N = n + 1 (tick n is the last row at rest); x_i = x_0 for i < 0, x_n for i > n
    window       a NAIVE sum of the W terms of every tick, oldest to newest, then one division; ticks 0 and M - 1 are copies
    peaks        an explicit loop over the ticks in order with a strict comparison (setpoint_cases.peak_py: the first tick of a tie stays)
    search       a linear scan: W = 1, measure, grow by min(max_window, max(W + 1, ceil(W P / aim))) while P > 1

For the constraint gap, isSatisfied and the clearance the expected values are the det oracle's applied to the expected FILTERED ticks.
The case builders at the end need no device; tests/test_jerk_cases.py asserts what each contains.

Deliberately wrong variants (mutate=...): "running" a sum carried from tick to tick (plus the newest term, minus the oldest), "divide_first"
every term divided by W before the sum, "left" the jerk attributed to the left tick of its three, "ends" the end ticks computed as means
instead of copied, "no_plus_one" the W + 1 term dropped from the update.
"""
import functools
import math

import numpy as np

import setpoint_cases as sc
from retime_cases import PANDA_AMAX, PANDA_VMAX  # noqa: F401  (the limits: for the tests)
from setpoint_cases import INF, NAN, bits, geodesic_rows, pack, same_f64, scaled_stamps  # noqa: F401

OK, EMPTY, NONFINITE, UNORDERED, POINT, FULL, WINDOW = range(7)
SPEED, ACC, JERK, DP, ANGLE, CLEARANCE = range(6)
PANDA_JMAX = (7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0) * 2
DEFAULT_TILE, SAMPLE_TILE = 128, 32  # csrc/ccmp_launch.h: kJerkTile, kJerkSampleTile


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def inputs_py(r, t, period):
    """(n, xq (n+1,14), xd (n+1,14)) of a path the setpoints rule calls OK for some tick budget: its interior ticks, both end rows at rest"""
    N = sc.count_py(float(t[-1]), period)
    xq, xd, _, _ = sc.path_py(r, t, period, N)
    return N - 1, xq, xd


def ticks_py(n, W, max_ticks):
    """M, or 0 when it does not fit"""
    return 0 if n + W > max_ticks else n + W


def mean_py(terms, W, divide_first=False):
    if divide_first:
        s = terms[0] / float(W)
        for v in terms[1:]:
            s = s + v / float(W)
        return s
    s = terms[0]
    for v in terms[1:]:
        s = s + v
    return s / float(W)


def window_py(xq, xd, n, W, period, mutate=()):
    """(q (M,14), qd (M,14), tau (M,)) of the window W"""
    M = n + W
    q, qd, tau = np.zeros((M, 14)), np.zeros((M, 14)), np.zeros(M)
    at = lambda x, i, c: float(x[min(max(i, 0), n)][c])
    run = None
    for j in range(M):
        tau[j] = float(j) * period
        if (j == 0 or j == M - 1) and "ends" not in mutate:
            q[j] = xq[0] if j == 0 else xq[n]
            if "running" in mutate and j == 0:
                run = [[mean_py([at(x, i, c) for i in range(1 - W, 1)], 1) for c in range(14)] for x in (xq, xd)]
            continue
        if "running" in mutate:
            if run is None:
                run = [[mean_py([at(x, i, c) for i in range(j - W + 1, j + 1)], 1) for c in range(14)] for x in (xq, xd)]
            else:
                for p, x in enumerate((xq, xd)):
                    for c in range(14):
                        run[p][c] = (run[p][c] + at(x, j, c)) - at(x, j - W, c)
            for c in range(14):
                q[j, c], qd[j, c] = run[0][c] / float(W), run[1][c] / float(W)
            continue
        for c in range(14):
            q[j, c] = mean_py([at(xq, i, c) for i in range(j - W + 1, j + 1)], W, "divide_first" in mutate)
            qd[j, c] = mean_py([at(xd, i, c) for i in range(j - W + 1, j + 1)], W, "divide_first" in mutate)
    return q, qd, tau


def velocity_window_py(xd, n, W):
    """qd alone (what a measurement of the search needs)"""
    M = n + W
    qd = np.zeros((M, 14))
    for j in range(1, M - 1):
        for c in range(14):
            qd[j, c] = mean_py([float(xd[min(max(i, 0), n)][c]) for i in range(j - W + 1, j + 1)], W)
    return qd


def jerk_values_py(qd, period, jmax, left=False):
    """[(tick, jerk ratio)] of the middle ticks 1 .. M - 2 (left: the mutation that names the left tick); a NaN share makes the tick's a NaN"""
    M = len(qd)
    out = []
    for j in range(M - 2):
        t0, t1, t2 = float(j) * period, float(j + 1) * period, float(j + 2) * period
        shares = []
        for c in range(14):
            a0 = (float(qd[j + 1][c]) - float(qd[j][c])) / (t1 - t0)
            a1 = (float(qd[j + 2][c]) - float(qd[j + 1][c])) / (t2 - t1)
            shares.append((abs(a1 - a0) / (0.5 * (t2 - t0))) / jmax[c])
        out.append((j if left else j + 1, NAN if any(s != s for s in shares) else max(shares)))
    return out


def next_window_py(W, P, aim, max_window, plus_one=True):
    y = (float(W) * P) / aim
    nxt = max_window if (math.isinf(y) or math.ceil(y) >= max_window) else int(math.ceil(y))
    if plus_one:
        nxt = max(nxt, W + 1)
    return min(nxt, max_window)


def search_py(xd, n, jmax, period, max_ticks, window, max_window, aim, mutate=()):
    """(status, W, passes, trace [(W, P)]) of one path whose W = `window or 1` fits"""
    W, passes, trace = (window or 1), 0, []
    while True:
        P = sc.peak_py(jerk_values_py(velocity_window_py(xd, n, W), period, jmax))[0]
        trace.append((W, P))
        if P <= 1.0:
            return OK, W, passes, trace
        if window or W >= max_window:
            return WINDOW, W, passes, trace
        nxt = next_window_py(W, P, aim, max_window, "no_plus_one" not in mutate)
        if nxt <= W:  # (only the mutation can stall)
            return WINDOW, W, passes, trace
        W, passes = nxt, passes + 1
        if not ticks_py(n, W, max_ticks):
            return FULL, W, passes, trace


def audit_py(qd, tau, f, satisfied, clearance, vmax, amax, jmax, period, margin, mutate=()):
    """one path's (peak [6], peak_tick [6], counts [2]): speed, acceleration and the other three as the setpoints audit takes them"""
    pk, tk, counts, _ = sc.audit_py(qd, tau, f, satisfied, clearance, vmax, amax, margin)
    jv, jt = sc.peak_py(jerk_values_py(qd, period, jmax, left="left" in mutate))
    return [pk[0], pk[1], jv, pk[2], pk[3], pk[4]], [tk[0], tk[1], jt, tk[2], tk[3], tk[4]], counts


def jerk_py(rows, path_first, time, vmax, amax, jmax, period=0.001, max_ticks=65536, window=0, max_window=64, aim=0.95, O=None, P=None, scene=None,
            margin=0.0, mutate=()):
    """the whole result as the library's copy returns it.  With an oracle O and its problem P: f and satisfied from it (and the clearance from
    scene = (spheres, boxes, allowed)) and six peaks; without: three peaks (what ccmp_jerk_setpoints_ref answers)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 14)
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    F = len(path_first) - 1
    status, win, passes = np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32), np.zeros(F, dtype=np.int32)
    first, parts, traces = [0], [], []
    none = (np.zeros((0, 14)), np.zeros((0, 14)), np.zeros(0))
    for f in range(F):
        a, b = int(path_first[f]), int(path_first[f + 1])
        r, t = rows[a:b], time[a:b]
        st, N = sc.status_py(r, t, period, max_ticks)
        part, trace = none, []
        if st == sc.POINT:
            part = (r[:1].copy(), np.zeros((1, 14)), np.zeros(1))
        elif st == sc.FULL:
            win[f] = window or 1
        elif st == sc.OK:
            n, xq, xd = inputs_py(r, t, period)
            assert n == N - 1
            if not ticks_py(n, window or 1, max_ticks):
                st, win[f] = FULL, window or 1
            else:
                st, win[f], passes[f], trace = search_py(xd, n, jmax, period, max_ticks, window, max_window, aim, mutate)
                if st != FULL:
                    part = window_py(xq, xd, n, int(win[f]), period, mutate)
        status[f] = st
        parts.append(part)
        traces.append(trace)
        first.append(first[-1] + len(part[2]))
    out = dict(q=np.vstack([p[0] for p in parts]) if F else np.zeros((0, 14)), qd=np.vstack([p[1] for p in parts]) if F else np.zeros((0, 14)),
               tau=np.concatenate([p[2] for p in parts]) if F else np.zeros(0), tick_first=np.array(first, dtype=np.int32), status=status, window=win,
               passes=passes, traces=traces)
    M = first[-1]
    out["ticks"] = M
    if O is not None:
        out["f"] = np.array([O.function(P, x) for x in out["q"]]).reshape(M, 2)
        out["satisfied"] = np.array([O.is_satisfied(P, x) for x in out["q"]], dtype=np.uint8)
        out["clearance"] = np.array([O.clearance(P, scene[0], scene[1], scene[2], x)[0] for x in out["q"]]) if scene is not None else np.full(M, NAN)
        f_, sat, clr = out["f"], out["satisfied"], out["clearance"]
    else:
        f_, sat, clr = np.full((M, 2), NAN), np.ones(M, dtype=np.uint8), np.full(M, NAN)
    peak, tick, counts = np.zeros((F, 6)), np.zeros((F, 6), dtype=np.int32), np.zeros((F, 2), dtype=np.int32)
    for f in range(F):
        a, b = first[f], first[f + 1]
        peak[f], tick[f], counts[f] = audit_py(out["qd"][a:b], out["tau"][a:b], f_[a:b], sat[a:b], clr[a:b], vmax, amax, jmax, period, margin, mutate)
    if O is not None:
        out.update(peak=peak, peak_tick=tick, counts=counts)
    else:
        out.update(peak=peak[:, :3].copy(), peak_tick=tick[:, :3].copy())
    return out


FLOAT_KEYS = ("q", "qd", "tau", "f", "clearance", "peak")
INT_KEYS = ("tick_first", "status", "window", "passes", "satisfied", "peak_tick", "counts")


def same_jerk(got, want, what="", keys=FLOAT_KEYS + INT_KEYS):
    """bit for bit, every array both sides have"""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    for k in keys:
        if k not in want or k not in g:
            continue
        if k in INT_KEYS:
            assert np.array_equal(np.asarray(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1)), (what, k, g[k], want[k])
        else:
            assert np.asarray(g[k]).shape == np.asarray(want[k]).shape and same_f64(g[k], want[k]), (what, k, np.argwhere(bits(g[k]) != bits(want[k]))[:5])


def host_part(want):
    """what ccmp_jerk_setpoints_ref answers of a full expected result"""
    out = {k: want[k] for k in ("q", "qd", "tau", "tick_first", "status", "window", "passes")}
    out["peak"], out["peak_tick"] = want["peak"][:, :3], want["peak_tick"][:, :3]
    return out


# ---- case builders (no device: the oracle alone; tests/test_jerk_cases.py asserts what each must contain) --------------------------------
RAGGED_SEED = sc.RAGGED_SEED
BATCH_PERIOD, BATCH_MAX_TICKS, BATCH_MAX_WINDOW, BATCH_AIM = 0.001, 300, 8, 0.95
CASE_TILE = 96  # the tile length the batch's tick counts are cut for: M of CASE_TILE - 1, CASE_TILE, CASE_TILE + 1 and 2 CASE_TILE + 1
BATCH_JMAX = PANDA_JMAX
NAMES = ("empty", "point", "non_finite", "unordered", "one_interval", "short", "m_less", "m_tile", "m_more", "m_two", "full", "full_after", "stiff", "three",
         "five", "two")
TARGET_M = {"m_less": (3, CASE_TILE - 1), "m_tile": (17, CASE_TILE), "m_more": (70, CASE_TILE + 1), "m_two": (17, 2 * CASE_TILE + 1)}  # name -> (rows, M)


def options(case):
    return dict(period=case["period"], max_ticks=case["max_ticks"], max_window=case["max_window"], aim=case["aim"])


def stamps_for(r, n, period):
    """a time-stamp profile scaled to end between n - 1 and n periods: ceil(D / period) = n"""
    return scaled_stamps(r, period * (n - 0.5))


def natural_stamps(r, scale=1.0):
    """the time-stamp rule's stamps (retime_cases.stamp_path_py, beta 0.5, the Panda's limits), every one times `scale`"""
    return [v * scale for v in sc.stamp_path_py(r, PANDA_VMAX, PANDA_AMAX, 0.5)[0]]


def path_with_ticks(r, M, period, jmax, max_window, aim):
    """stamps for rows r such that the CHOSEN window gives exactly M ticks: n + W(n) = M, found by a scan over n"""
    for n in range(M - 1, 0, -1):
        t = stamps_for(r, n, period)
        _, _, xd = inputs_py(r, t, period)
        _, W, _, _ = search_py(xd, n, jmax, period, 10 ** 6, 0, max_window, aim)
        if n + W == M:
            return t
    raise AssertionError("no stamps give %d ticks" % M)


def ragged_batch(O, P):
    """one call at period 0.001, max_ticks 300, max_window 8, aim 0.95 under the Panda's limits; the rows are the first rows of ONE 70-row run
    of the oracle's geodesic states:
        empty, point, non_finite, unordered   the setpoints rule's reasons
        one_interval   two rows with D <= period: n = 1, every qd zero, M = 1 + W
        short          two rows 1e-3 rad apart over 2.5 periods: n = 3 < W at the end, and the jerk ratio stays above 1: WINDOW
        m_less .. m_two   3, 17, 70 and 17 rows whose stamps are scaled so that the chosen window gives M = T - 1, T, T + 1 and 2 T + 1 ticks
                       for T = CASE_TILE
        full           n + 1 = max_ticks + 1: FULL before any measurement
        full_after     n + 1 = max_ticks: fits with W = 1, and the first growth of the window does not
        stiff, three, five, two   3, 3, 5 and 2 rows under their natural stamps times 0.5, 1, 1 and 1: different windows and passes in one launch
    -> dict(rows, path_first, time, period, max_ticks, max_window, aim, jmax, names)"""
    run = geodesic_rows(O, P, 70, RAGGED_SEED)
    bad_row = run[:3].copy()
    bad_row[1, 9] = NAN
    t3 = scaled_stamps(run[:3], 0.05)
    near = np.array([run[0], run[0]])
    near[1] = near[1] + 1e-3
    pd = BATCH_PERIOD
    paths = {
        "empty": (run[:0], []),
        "point": (run[:1], [0.0]),
        "non_finite": (bad_row, t3),
        "unordered": (run[:3], [t3[0], t3[2], t3[1]]),
        "one_interval": (run[:2], [0.0, 0.75 * pd]),
        "short": (near, [0.0, 2.5 * pd]),
        "full": (run[:9], stamps_for(run[:9], BATCH_MAX_TICKS, pd)),
        "full_after": (run[:5], stamps_for(run[:5], BATCH_MAX_TICKS - 1, pd)),
        "stiff": (run[:3], natural_stamps(run[:3], 0.5)),
        "three": (run[:3], natural_stamps(run[:3])),
        "five": (run[:5], natural_stamps(run[:5])),
        "two": (run[:2], natural_stamps(run[:2])),
    }
    for name, (nrows, M) in TARGET_M.items():
        paths[name] = (run[:nrows], path_with_ticks(run[:nrows], M, pd, BATCH_JMAX, BATCH_MAX_WINDOW, BATCH_AIM))
    rows, first, time = pack([paths[n] for n in NAMES])
    return dict(rows=rows, path_first=first, time=time, period=pd, max_ticks=BATCH_MAX_TICKS, max_window=BATCH_MAX_WINDOW, aim=BATCH_AIM, jmax=BATCH_JMAX,
                names=NAMES)


def one_path(case, name):
    f = case["names"].index(name)
    a, b = case["path_first"][f], case["path_first"][f + 1]
    return dict(case, rows=case["rows"][a:b], path_first=np.array([0, b - a], dtype=np.int32), time=case["time"][a:b], names=(name,))


def scene_case(O, P):
    """the setpoints tests' scene case (three waypoints 0.6 apart at 4 ms, one moving and one static sphere) under jerk limits that make the
    search grow the window: the filtered ticks cut the corner at the middle waypoint, and f, satisfied, clearance and their peaks are
    the oracle's on those ticks"""
    base = sc.scene_case(O, P)
    case = dict(rows=base["rows"], path_first=base["path_first"], time=base["time"], period=base["period"], max_ticks=65536, max_window=8, aim=0.95,
                jmax=PANDA_JMAX, scene=base["scene"], margin=base["margin"])
    case["want"] = jerk_py(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, case["jmax"], O=O, P=P, scene=case["scene"],
                           margin=case["margin"], **options(case))
    return case


FIXED_WINDOWS = (1, 2, 3, BATCH_MAX_WINDOW)


@functools.lru_cache(maxsize=None)
def reference():
    """the ragged batch with its expected results under the stock problem — the chosen window and every fixed window of FIXED_WINDOWS — and the
    scene case, computed once per process and shared by the tests that need it (never changed by them)"""
    from graph_cases import _det
    from smooth_cases import stock_problem

    O = _det()[0]
    P = stock_problem(O, 1)
    case = ragged_batch(O, P)
    out = {"O": O, "P": P, "case": case}
    for w in (0,) + FIXED_WINDOWS:
        out[w] = jerk_py(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, case["jmax"], window=w, O=O, P=P, **options(case))
    out["scene"] = scene_case(O, P)
    return out
