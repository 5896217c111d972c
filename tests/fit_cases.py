"""Time stamps fitted to the limits at the controller's rate: a plain-Python restatement of the rule of csrc/ccmp_fit.h and the expected values
the tests compare with.

The expected values are never the code under test.  The rule is restated here in Python floats (IEEE doubles, one rounding per operation,
nothing fused) and `math.sqrt`, on the pieces of setpoint_cases.py — status_py, tangents_py, qd_py, tau_py and bracket_py, imported and
unchanged:

    status      setpoint_cases.status_py on the current stamps; anything but OK ends the path with the stamps it was found on
    ticks       every tick's tau, its bracket by the LINEAR scan of the definition (k_0 = k_1), every tick's qd held in a list — the library
                holds no tick array at all
    S, A        S_k = max{ s_j : k_j = k }, A_k = max{ a_j : k_j <= k <= k_{j+1} } by explicit loops over the ticks in order
    done        P_s <= 1 and P_a <= 1: FITTED; passes == max_passes: PASSES
    dilation    f_k = max(1, S_k / aim, sqrt(A_k / aim)), h'_k = (t_k - t_{k-1}) f_k, the stamps summed left to right from +0.0

`mutate` names deliberately wrong variants (tests/test_fit_ref.py lists them).  The case builders at the end need no device;
tests/test_fit_cases.py asserts what each contains.
"""
import functools
import math

import numpy as np

from setpoint_cases import (EMPTY, FULL, NAN, NONFINITE, OK, PANDA_AMAX, PANDA_VMAX, POINT, RAGGED_SEED, UNORDERED, bits, bracket_py,  # noqa: F401
                            geodesic_rows, pack, qd_py, same_f64, status_py, tangents_py, tau_py)
from retime_cases import stamp_path_py

FITTED, PASSES = 0, 6
SPEED, ACC = 0, 1


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def measure_py(r, t, N, vmax, amax, period, mutate=()):
    """(S [R], A [R], brackets k [N]) of an OK path with N ticks under the stamps t (a list of floats)"""
    R, D = len(r), t[-1]
    w = tangents_py(r, t)
    tau = [tau_py(j, N, period, D) for j in range(N)]
    k = [0] * N
    for j in range(1, N):
        k[j] = bracket_py(t, tau[j])
    k[0] = 1 if "k0" in mutate else k[1]
    qd = [[0.0] * 14 for _ in range(N)]
    for j in range(1, N - 1):
        a, b = k[j] - 1, k[j]
        h = t[b] - t[a]
        u = (tau[j] - t[a]) / h
        qd[j] = [qd_py(float(r[a][c]), float(r[b][c]), float(w[a, c]), float(w[b, c]), h, u) for c in range(14)]
    S, A = [0.0] * R, [0.0] * R
    for j in range(N):
        shares = [abs(qd[j][c]) / vmax[c] for c in range(14)]
        if any(v != v for v in shares):
            continue  # a NaN never contributes
        S[k[j]] = max(S[k[j]], max(shares))
    for j in range(N - 1):
        width = tau[j + 1] - tau[j]
        if not width > 0.0:
            continue
        shares = [(abs(qd[j + 1][c] - qd[j][c]) / width) / amax[c] for c in range(14)]
        if any(v != v for v in shares):
            continue
        a = max(shares)
        for kk in range(k[j], (k[j] if "own" in mutate else k[j + 1]) + 1):
            A[kk] = max(A[kk], a)
    return S, A, k


def factor_py(S, A, aim, mutate=()):
    return max(1.0, S / aim, (A / aim) if "nosqrt" in mutate else math.sqrt(A / aim))


def closed_duration_py(st, t):
    return 0.0 if st == EMPTY else NAN if st == NONFINITE else t[-1]


def fit_path_py(r, t, vmax, amax, period=0.001, max_ticks=65536, aim=0.95, max_passes=8, mutate=()):
    """one path -> dict(time [R], status, passes, peak (P_s, P_a), duration, trace: per measurement (S, A, k))"""
    t = [float(v) for v in t]
    passes, peak, trace = 0, (0.0, 0.0), []
    while True:
        st, N = status_py(r, np.array(t, dtype=np.float64), period, max_ticks)
        if st != OK:
            return dict(time=t, status=st, passes=passes, peak=peak, duration=closed_duration_py(st, t), trace=trace)
        S, A, k = measure_py(r, t, N, vmax, amax, period, mutate)
        trace.append((S, A, k))
        peak = (max(S[1:]), max(A[1:]))
        done = peak[0] <= 1.0 and peak[1] <= 1.0
        if done or passes == max_passes:
            return dict(time=t, status=FITTED if done else PASSES, passes=passes, peak=peak, duration=t[-1], trace=trace)
        new = [0.0] * len(t)
        for i in range(1, len(t)):
            new[i] = new[i - 1] + (t[i] - t[i - 1]) * factor_py(S[i], A[i], aim, mutate)
        t = new
        passes += 1


def fit_py(rows, path_first, time, vmax, amax, period=0.001, max_ticks=65536, aim=0.95, max_passes=8, mutate=()):
    """the whole result as the library returns it: dict(time, status, passes, peak, duration, factor) plus traces"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 14)
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    F = len(path_first) - 1
    out = dict(time=time.copy(), status=np.zeros(F, dtype=np.int32), passes=np.zeros(F, dtype=np.int32), peak=np.zeros((F, 2)), duration=np.zeros(F),
               factor=np.ones(len(time)), traces=[])
    for f in range(F):
        a, b = int(path_first[f]), int(path_first[f + 1])
        p = fit_path_py(rows[a:b], time[a:b], vmax, amax, period, max_ticks, aim, max_passes, mutate)
        out["time"][a:b] = p["time"]
        out["status"][f], out["passes"][f], out["peak"][f], out["duration"][f] = p["status"], p["passes"], p["peak"], p["duration"]
        out["traces"].append(p["trace"])
        for i in range(a + 1, b):
            hin = float(time[i]) - float(time[i - 1])
            if hin > 0.0:
                out["factor"][i] = (float(out["time"][i]) - float(out["time"][i - 1])) / hin
    return out


FLOAT_KEYS, INT_KEYS = ("time", "peak", "duration", "factor"), ("status", "passes")


def same_fit(got, want, what="", keys=FLOAT_KEYS + INT_KEYS):
    """bit for bit, every array both sides have"""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    for k in keys:
        if k not in want or k not in g:
            continue
        if k in INT_KEYS:
            assert np.array_equal(np.asarray(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1)), (what, k, g[k], want[k])
        else:
            assert np.asarray(g[k]).shape == np.asarray(want[k]).shape and same_f64(g[k], want[k]), (what, k, np.argwhere(bits(g[k]) != bits(want[k]))[:5])


# ---- case builders (no device: the oracle alone; tests/test_fit_cases.py asserts what each must contain) ---------------------------------
BATCH_PERIOD, BATCH_MAX_TICKS, BATCH_AIM, BATCH_MAX_PASSES = 0.004, 2048, 0.95, 6
NAMES = ("two", "three", "empty", "seventeen", "point", "seventy", "non_finite", "repeats", "unordered", "tight", "within", "full_after", "slow_start")


def natural_stamps(r, scale=1.0):
    """the time-stamp rule's stamps (retime_cases.stamp_path_py, beta 0.5, the Panda's limits), every one times `scale`"""
    return [v * scale for v in stamp_path_py(r, PANDA_VMAX, PANDA_AMAX, 0.5)[0]]


def ragged_batch(O, P):
    """one call at period 0.004 under max_ticks 2048; the rows are the first rows of ONE 70-row run of the oracle's geodesic states:
        two, three, seventeen, seventy   2, 3, 17 and 70 rows under their natural stamps scaled by 1, 0.8, 0.6 and 1: they need different
                                         numbers of dilations
        empty, point, non_finite, unordered   between the others
        repeats      a b b c d d with repeated stamps on the repeated rows: two intervals of no width, one of them the last
        tight        30 rows in 0.026 s: at 4 ms several row intervals hold no tick, one tick interval spans many row intervals
        within       9 rows under four times their natural stamps: inside the limits as it comes
        full_after   five rows 0.5 apart with stamps 0, 4, 4.001, 4.002, 8.1: 2026 ticks, and the first dilation takes it beyond 2048
        slow_start   17 rows under 1.3 times their natural stamps
    -> dict(rows, path_first, time, period, max_ticks, aim, max_passes, names)"""
    run = geodesic_rows(O, P, 70, RAGGED_SEED)
    bad_row = run[:3].copy()
    bad_row[1, 9] = NAN
    t3 = natural_stamps(run[:3])
    a, b, c, d = run[0], run[5], run[10], run[15]
    tr = natural_stamps(np.array([a, b, c, d]))
    far = run[[0, 10, 20, 30, 40]]
    paths = {
        "two": (run[:2], natural_stamps(run[:2])),
        "three": (run[:3], natural_stamps(run[:3], 0.8)),
        "empty": (run[:0], []),
        "seventeen": (run[:17], natural_stamps(run[:17], 0.6)),
        "point": (run[:1], [0.0]),
        "seventy": (run, natural_stamps(run)),
        "non_finite": (bad_row, t3),
        "repeats": (np.array([a, b, b, c, d, d]), [tr[0], tr[1], tr[1], tr[2], tr[3], tr[3]]),
        "unordered": (run[:3], [t3[0], t3[2], t3[1]]),
        "tight": (run[:30], natural_stamps(run[:30], 0.026 / natural_stamps(run[:30])[-1])),
        "within": (run[:9], natural_stamps(run[:9], 4.0)),
        "full_after": (far, [0.0, 4.0, 4.001, 4.002, 8.1]),
        "slow_start": (run[20:37], natural_stamps(run[20:37], 1.3)),
    }
    rows, first, time = pack([paths[n] for n in NAMES])
    return dict(rows=rows, path_first=first, time=time, period=BATCH_PERIOD, max_ticks=BATCH_MAX_TICKS, aim=BATCH_AIM, max_passes=BATCH_MAX_PASSES, names=NAMES)


def reordered(case):
    """the same paths in another order behind a copy of the three-row path: every tick interval lands in another group, wavefront and block —
    another launch shape for the same work.  -> (case, order) with order[i] = the path of `case` that path i + 1 of the result is"""
    pf = case["path_first"]
    F = len(pf) - 1
    order = list(range(F - 1, -1, -1))
    take = [NAMES.index("three")] + order
    paths = [(case["rows"][pf[f]:pf[f + 1]], case["time"][pf[f]:pf[f + 1]]) for f in take]
    rows, first, time = pack(paths)
    return dict(case, rows=rows, path_first=first, time=time), order


def options(case):
    return dict(period=case["period"], max_ticks=case["max_ticks"], aim=case["aim"], max_passes=case["max_passes"])


@functools.lru_cache(maxsize=None)
def reference():
    """the ragged batch with its expected result under the stock problem's geodesic rows, computed once per process and shared by the tests
    that need it (never changed by them)"""
    from graph_cases import _det
    from smooth_cases import stock_problem

    O = _det()[0]
    P = stock_problem(O, 1)
    case = ragged_batch(O, P)
    return dict(case=case, want=fit_py(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, **options(case)))
