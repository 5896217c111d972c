"""Controller-rate setpoints and the execution audit: a plain-Python restatement of the rule of csrc/ccmp_setpoints.h and the expected values
the tests compare with.

The expected values are never the code under test.  The rule is restated here operation for operation in Python floats (IEEE doubles, one
rounding per operation, nothing fused) and `math.sqrt`:

    status       in the order EMPTY, NONFINITE, UNORDERED, POINT, FULL, OK; N = 1 + ceil(D / period), at least 2
    ticks        tau_0 = 0, tau_{N-1} = D, else min(j * period, D)
    tangents     Fritsch-Butland: zero at the ends and where the two slopes do not share a sign, else (a + b) / (a / m0 + b / m1)
    bracket      a LINEAR scan for the smallest k >= 1 with t_k >= tau (the library bisects); u = (tau - t_{k-1}) / (t_k - t_{k-1})
    q, qd        the cubic in the header's operation order
    audit        the peaks by an explicit loop over the ticks in order with a strict comparison (the first tick of a tie stays)

For the constraint gap, isSatisfied and the clearance the expected values are the det oracle's `function`, `is_satisfied` and `clearance`
applied to the expected setpoints.  The case builders at the end need no device; tests/test_setpoint_cases.py asserts what each contains.
"""
import functools
import math

import numpy as np

from retime_cases import PANDA_AMAX, PANDA_VMAX, stamp_path_py, traversable_chains  # noqa: F401  (the limits: for the tests)
from smooth_cases import bits, same_f64  # noqa: F401

OK, EMPTY, NONFINITE, UNORDERED, POINT, FULL = range(6)
SPEED, ACC, DP, ANGLE, CLEARANCE = range(5)
INT32_MAX = 2 ** 31 - 1
INF, NAN = float("inf"), float("nan")


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def count_py(D, period):
    """N of a path with D > 0, or None beyond INT32_MAX"""
    q = D / period
    if math.isinf(q) or not math.ceil(q) < INT32_MAX:
        return None
    return max(1 + int(math.ceil(q)), 2)


def status_py(r, t, period, max_ticks):
    """(status, ticks) of one path: rows r (R,14), stamps t (R,)"""
    R = len(r)
    if R == 0:
        return EMPTY, 0
    if not (np.isfinite(r).all() and np.isfinite(t).all()):
        return NONFINITE, 0
    t = [float(v) for v in t]
    if t[0] != 0.0:
        return UNORDERED, 0
    for i in range(R - 1):
        if t[i + 1] < t[i] or (t[i + 1] == t[i] and any(float(r[i][c]) != float(r[i + 1][c]) for c in range(14))):
            return UNORDERED, 0
    if R == 1 or not t[-1] > 0.0:
        return POINT, 1
    N = count_py(t[-1], period)
    if N is None or N > max_ticks:
        return FULL, 0
    return OK, N


def tau_py(j, N, period, D, with_min=True):
    if j == 0:
        return 0.0
    if j == N - 1:
        return D
    return min(float(j) * period, D) if with_min else float(j) * period


def slope_py(ra, rb, h):
    d = rb - ra
    return d / h if h > 0.0 else 0.0


def tangent_py(hp, h, mp, m, sign_test=True):
    if sign_test and not mp * m > 0.0:
        return 0.0
    if not sign_test:  # the mutation: numpy's doubles, which divide by zero without raising
        hp, h, mp, m = (np.float64(v) for v in (hp, h, mp, m))
        with np.errstate(all="ignore"):
            return float((2.0 * h + hp + (h + 2.0 * hp)) / ((2.0 * h + hp) / mp + (h + 2.0 * hp) / m))
    a = 2.0 * h + hp
    b = h + 2.0 * hp
    return (a + b) / (a / mp + b / m)


def tangents_py(r, t, sign_test=True):
    """w (R,14) of one path"""
    R = len(r)
    w = np.zeros((R, 14))
    for i in range(1, R - 1):
        hp, h = float(t[i]) - float(t[i - 1]), float(t[i + 1]) - float(t[i])
        for c in range(14):
            w[i, c] = tangent_py(hp, h, slope_py(float(r[i - 1][c]), float(r[i][c]), hp), slope_py(float(r[i][c]), float(r[i + 1][c]), h), sign_test)
    return w


def bracket_py(t, tau, strict=False):
    """the smallest k >= 1 with t_k >= tau (strict: the mutation `>`), by the linear scan of the definition"""
    return next(k for k in range(1, len(t)) if (t[k] > tau if strict else t[k] >= tau))


def q_py(ra, rb, wa, wb, h, u):
    d = rb - ra
    v = 1.0 - u
    s = (u * u) * (3.0 - 2.0 * u)
    p = s * d
    huv = h * (u * v)
    e = v * wa - u * wb
    return (ra + p) + huv * e


def qd_py(ra, rb, wa, wb, h, u):
    d = rb - ra
    v = 1.0 - u
    g = (6.0 * u) * v
    t1 = (g * d) / h
    t2 = (v * (1.0 - 3.0 * u)) * wa
    t3 = (u * (3.0 * u - 2.0)) * wb
    return (t1 + t2) + t3


def path_py(r, t, period, N, mutate=()):
    """(q (N,14), qd (N,14), tau (N,), brackets [k per interior tick]) of an OK path.  mutate: names of deliberately wrong variants of the
    rule — "bracket" (`>` for `>=`), "tangent" (no sign test), "tau" (no min against D); "tie" is peak_py's"""
    R = len(r)
    t = [float(v) for v in t]
    D = t[-1]
    w = np.nan_to_num(tangents_py(r, t, sign_test="tangent" not in mutate))
    q, qd, tau, ks = np.zeros((N, 14)), np.zeros((N, 14)), np.zeros(N), []
    q[0], q[N - 1], tau[N - 1] = r[0], r[R - 1], D
    for j in range(1, N - 1):
        tau[j] = tau_py(j, N, period, D, with_min="tau" not in mutate)
        k = bracket_py(t, tau[j], strict="bracket" in mutate and tau[j] < D)
        ks.append(k)
        h = t[k] - t[k - 1]
        u = (float(tau[j]) - t[k - 1]) / h
        for c in range(14):
            q[j, c] = q_py(float(r[k - 1][c]), float(r[k][c]), float(w[k - 1, c]), float(w[k, c]), h, u)
            qd[j, c] = qd_py(float(r[k - 1][c]), float(r[k][c]), float(w[k - 1, c]), float(w[k, c]), h, u)
    return q, qd, tau, ks


def peak_py(values, lowest=False, last_tie=False):
    """(value, tick) over (tick, value) pairs in tick order: a NaN never contributes, the first tick of a tie stays (last_tie: the mutation
    that keeps the last); none: +0.0 (+inf), -1"""
    bv, bj = (INF if lowest else 0.0), -1
    for j, v in values:
        if v != v:
            continue
        if bj < 0 or (v < bv if lowest else v > bv) or (last_tie and v == bv):
            bv, bj = v, j
    return bv, bj


def audit_py(qd, tau, f, satisfied, clearance, vmax, amax, margin, last_tie=False):
    """one path's (peak [5], peak_tick [5], counts [2], stretch)"""
    N = len(tau)
    speed, acc = [], []
    for j in range(N):
        speed.append((j, max((abs(float(qd[j][c])) / vmax[c] for c in range(14)), default=0.0)))
        if j + 1 < N:
            width = float(tau[j + 1]) - float(tau[j])
            if width > 0.0:
                acc.append((j, max((abs(float(qd[j + 1][c]) - float(qd[j][c])) / width) / amax[c] for c in range(14))))
    lt = dict(last_tie=last_tie)
    peaks = [peak_py(speed, **lt), peak_py(acc, **lt), peak_py([(j, float(f[j][0])) for j in range(N)], **lt),
             peak_py([(j, float(f[j][1])) for j in range(N)], **lt), peak_py([(j, float(clearance[j])) for j in range(N)], lowest=True, **lt)]
    counts = [sum(1 for j in range(N) if not satisfied[j]), sum(1 for j in range(N) if float(clearance[j]) < margin)]
    stretch = max(1.0, peaks[SPEED][0], math.sqrt(peaks[ACC][0]))
    return [p[0] for p in peaks], [p[1] for p in peaks], counts, stretch


def setpoints_py(rows, path_first, time, vmax, amax, period=0.001, max_ticks=65536, O=None, P=None, scene=None, margin=0.0, mutate=()):
    """the whole result as the library's copy returns it.  With an oracle O and its problem P: f and satisfied from it (and the clearance from
    scene = (spheres, boxes, allowed)); without: f, satisfied, clearance and the peaks that need them are left out (what ccmp_setpoints_ref
    answers)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 14)
    time = np.asarray(time, dtype=np.float64).reshape(-1)
    F = len(path_first) - 1
    status, first, parts, brackets = np.zeros(F, dtype=np.int32), [0], [], []
    for f in range(F):
        a, b = int(path_first[f]), int(path_first[f + 1])
        r, t = rows[a:b], time[a:b]
        st, N = status_py(r, t, period, max_ticks)
        status[f] = st
        if st == POINT:
            parts.append((r[:1].copy(), np.zeros((1, 14)), np.zeros(1)))
            brackets.append([])
        elif st == OK:
            q, qd, tau, ks = path_py(r, t, period, N, mutate)
            parts.append((q, qd, tau))
            brackets.append(ks)
        else:
            parts.append((np.zeros((0, 14)), np.zeros((0, 14)), np.zeros(0)))
            brackets.append([])
        first.append(first[-1] + N)
    out = dict(q=np.vstack([p[0] for p in parts]) if F else np.zeros((0, 14)), qd=np.vstack([p[1] for p in parts]) if F else np.zeros((0, 14)),
               tau=np.concatenate([p[2] for p in parts]) if F else np.zeros(0), tick_first=np.array(first, dtype=np.int32), status=status, brackets=brackets)
    M = first[-1]
    out["ticks"] = M
    if O is not None:
        out["f"] = np.array([O.function(P, x) for x in out["q"]]).reshape(M, 2)
        out["satisfied"] = np.array([O.is_satisfied(P, x) for x in out["q"]], dtype=np.uint8)
        out["clearance"] = np.array([O.clearance(P, scene[0], scene[1], scene[2], x)[0] for x in out["q"]]) if scene is not None else np.full(M, NAN)
        f_, sat, clr = out["f"], out["satisfied"], out["clearance"]
    else:
        f_, sat, clr = np.full((M, 2), NAN), np.ones(M, dtype=np.uint8), np.full(M, NAN)
    peak, tick, counts, stretch = np.zeros((F, 5)), np.zeros((F, 5), dtype=np.int32), np.zeros((F, 2), dtype=np.int32), np.zeros(F)
    for f in range(F):
        a, b = first[f], first[f + 1]
        peak[f], tick[f], counts[f], stretch[f] = audit_py(out["qd"][a:b], out["tau"][a:b], f_[a:b], sat[a:b], clr[a:b], vmax, amax, margin, "tie" in mutate)
    if O is not None:
        out.update(peak=peak, peak_tick=tick, counts=counts, stretch=stretch)
    else:
        out.update(peak=peak[:, :2].copy(), peak_tick=tick[:, :2].copy(), stretch=stretch)
    return out


FLOAT_KEYS = ("q", "qd", "tau", "f", "clearance", "peak", "stretch")
INT_KEYS = ("tick_first", "status", "satisfied", "peak_tick", "counts")


def same_setpoints(got, want, what="", keys=FLOAT_KEYS + INT_KEYS):
    """bit for bit, every array both sides have"""
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    for k in keys:
        if k not in want or k not in g:
            continue
        if k in INT_KEYS:
            assert np.array_equal(np.asarray(g[k]).reshape(-1), np.asarray(want[k]).reshape(-1)), (what, k, g[k], want[k])
        else:
            assert np.asarray(g[k]).shape == np.asarray(want[k]).shape and same_f64(g[k], want[k]), (what, k, np.argwhere(bits(g[k]) != bits(want[k]))[:5])


# ---- case builders (no device: the oracle alone; tests/test_setpoint_cases.py asserts what each must contain) ----------------------------
RAGGED_SEED, SCENE_SEED, STAMP_SEED = 0x7600, 0x7700, 0x7900
GEODESIC_DELTA = 0.05  # the rows of the batches are the oracle's geodesic states at this step
RAGGED_ROWS = (0, 1, 2, 3, 17, 70, 5)  # rows of the OK / POINT / EMPTY paths; the bad paths follow
RAGGED_TICKS = {2: 2, 3: 15, 17: 257, 70: 17, 5: 16}  # rows -> the ticks its stamps are scaled to give
RAGGED_PERIOD = 0.001
STAMP_PERIOD, STAMP_STEP = 2.0 ** -9, 2.0 ** -7
SCENE_PERIOD = 0.004


def geodesic_rows(O, P, n, seed):
    """n rows on the manifold: the oracle's geodesic states (step GEODESIC_DELTA, analytic Jacobian) along a traversable chain of waypoints,
    segment after segment, cut at n"""
    Pg = type(P).from_buffer_copy(bytes(P))
    Pg.delta, Pg.jacobian_mode = GEODESIC_DELTA, 1
    chain = traversable_chains(O, P, (8,), seed, 16)[0]
    rows = []
    for i in range(len(chain) - 1):
        ok, st, _ = O.discrete_geodesic(Pg, chain[i], chain[i + 1], interpolate=True, max_states=1024)
        assert ok
        rows.extend(st)
        if len(rows) >= n:
            break
    assert len(rows) >= n, (len(rows), n)
    return np.array(rows[:n])


def scaled_stamps(r, D):
    """stamps of an OK time-stamp profile (retime_cases.stamp_path_py under the Panda's limits) scaled to end exactly at D"""
    t = stamp_path_py(r, PANDA_VMAX, PANDA_AMAX, 0.5)[0]
    s = [v * (D / t[-1]) for v in t]
    s[0], s[-1] = 0.0, D
    assert all(s[i + 1] > s[i] for i in range(len(s) - 1))
    return s


def pack(paths):
    """[(rows, stamps)] -> (rows (R,14), path_first (F+1,), time (R,))"""
    first = np.cumsum([0] + [len(r) for r, _ in paths]).astype(np.int32)
    rows = np.vstack([np.asarray(r, dtype=np.float64).reshape(-1, 14) for r, _ in paths]) if paths else np.zeros((0, 14))
    return rows, first, np.array([v for _, t in paths for v in t], dtype=np.float64)


def ragged_batch(O, P):
    """one call at period 0.001: paths of 0, 1, 2, 3, 17, 70 and 5 rows on the manifold (the first rows of ONE 70-row run of geodesic states),
    their stamps a time-stamp profile scaled so that the OK paths get 2, 15, 257, 17 and 16 ticks: 2 ticks = a period longer than the
    duration; the 70-row path's 17 ticks = a period of several row intervals, so brackets skip rows.  Then five bad paths on the 3-row
    path: a NaN coordinate, a NaN stamp, t_0 != 0, a decreasing stamp, a repeated stamp on rows that differ.
    -> dict(rows, path_first, time, period, statuses, ticks)"""
    run = geodesic_rows(O, P, 70, RAGGED_SEED)
    paths, statuses, ticks = [], [], []
    for n in RAGGED_ROWS:
        r = run[:n]
        if n < 2:
            paths.append((r, [0.0] * n))
            statuses.append(EMPTY if n == 0 else POINT)
            ticks.append(n)
            continue
        N = RAGGED_TICKS[n]
        D = RAGGED_PERIOD * (0.5 if N == 2 else N - 1.5)  # ceil(D / period) = N - 1
        paths.append((r, scaled_stamps(r, D)))
        statuses.append(OK)
        ticks.append(N)
    r3, t3 = run[:3], scaled_stamps(run[:3], 0.0135)
    bad_row = r3.copy()
    bad_row[1, 9] = NAN
    paths += [(bad_row, t3), (r3, [t3[0], NAN, t3[2]]), (r3, [1e-9, t3[1], t3[2]]), (r3, [t3[0], t3[2], t3[1]]), (r3, [t3[0], t3[1], t3[1]])]
    statuses += [NONFINITE, NONFINITE, UNORDERED, UNORDERED, UNORDERED]
    ticks += [0] * 5
    rows, first, time = pack(paths)
    return dict(rows=rows, path_first=first, time=time, period=RAGGED_PERIOD, statuses=statuses, ticks=ticks, run=run)


def on_the_stamp_batch(O, P):
    """stamps that are multiples of 2^-7 under a period of 2^-9: every product j * period is exact and every fourth tick of the first path
    (stamps i 2^-7) EQUALS a stamp, where the bracket's `>=` must take the interval that ends there.  The interpolant is C1, so at a stamp
    both intervals give the same q and qd IN EXACT ARITHMETIC; what tells them apart is rounding: the interval that ends there computes
    fl(a + fl(b - a)), which is b only while the difference is exact.  The first path's geodesic rows are 0.05 apart and their differences
    exact (the tick is the row, bit for bit, from either side); the second path has uneven multiples and rows that are random joint vectors
    (on no manifold: the rule asks for none) whose differences round, so there `>` and `>=` differ in bits."""
    run = geodesic_rows(O, P, 70, RAGGED_SEED)
    a, b = run[:9], np.random.default_rng(STAMP_SEED).uniform(-2.5, 2.5, (8, 14))
    return dict(zip(("rows", "path_first", "time"), pack([(a, [i * STAMP_STEP for i in range(9)]), (b, [m * STAMP_STEP for m in (0, 1, 2, 4, 5, 8, 9, 11)])])),
                period=STAMP_PERIOD)


def still_batch(O, P):
    """path 0: five identical rows with advancing stamps — every peak ties on every tick and must answer tick 0; path 1: repeated stamps on
    repeated rows (a a b b c at 0, 0, s, s, 2 s), which is ordered: a zero-width interval is never a bracket"""
    run = geodesic_rows(O, P, 70, RAGGED_SEED)
    a, b, c = run[0], run[6], run[12]
    return dict(zip(("rows", "path_first", "time"), pack([([a] * 5, [0.0, 0.004, 0.008, 0.012, 0.016]), ([a, a, b, b, c], [0.0, 0.0, 0.0085, 0.0085, 0.017])])),
                period=RAGGED_PERIOD)


def full_batch(O, P):
    """three OK paths of the ragged batch (3, 17 and 5 rows: 15, 257 and 16 ticks) under max_ticks = 256: the middle one is FULL, the others
    are untouched"""
    rb = ragged_batch(O, P)
    pf = rb["path_first"]
    pick = [3, 4, 6]
    paths = [(rb["rows"][pf[f]:pf[f + 1]], rb["time"][pf[f]:pf[f + 1]]) for f in pick]
    return dict(zip(("rows", "path_first", "time"), pack(paths)), period=RAGGED_PERIOD, max_ticks=256, ticks=[15, 0, 16])


def scene_case(O, P):
    """one path of three waypoints 0.6 apart (a chain's, not geodesic states: the blend between them leaves the rows far behind) and a scene
    of ONE moving sphere (arm 0, frame 4) and ONE static sphere placed where the moving one is at an interior tick between rows 0 and 1,
    5 cm above: the smallest clearance along the ticks falls strictly between two rows.  The margin is half-way between that minimum and
    the smallest clearance at a row.  -> dict(rows, path_first, time, period, scene=(spheres, boxes, allowed), margin, min_tick, want)"""
    from closed_chain_motion_planner_amd import scene as S

    r = traversable_chains(O, P, (3,), SCENE_SEED, 16)[0]
    rows, first, time = pack([(r, scaled_stamps(r, 0.25))])
    moving = (S.frame(0, 4), 4, (0.0, 0.0, 0.0), 0.05)
    base = setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, SCENE_PERIOD)
    k1 = next(j for j in range(base["ticks"]) if base["tau"][j] >= time[1])  # the first tick at or behind row 1
    at = O.proxy_centres(P, [moving], base["q"][k1 // 2])[0]
    spheres = [moving, (S.FRAME_WORLD, S.GROUP_ENVIRONMENT, (float(at[0]), float(at[1]), float(at[2]) + 0.05), 0.02)]
    scene = (spheres, [], None)
    clr = [O.clearance(P, spheres, [], None, x)[0] for x in base["q"]]
    at_rows = [O.clearance(P, spheres, [], None, x)[0] for x in r]
    margin = 0.5 * (min(clr) + min(at_rows))
    want = setpoints_py(rows, first, time, PANDA_VMAX, PANDA_AMAX, SCENE_PERIOD, O=O, P=P, scene=scene, margin=margin)
    return dict(rows=rows, path_first=first, time=time, period=SCENE_PERIOD, scene=scene, margin=margin, at_rows=at_rows, want=want)


@functools.lru_cache(maxsize=None)
def reference():
    """every batch above with its expected results under the stock problem, computed once per process and shared by the tests that need it
    (never changed by them): {name: dict(case, want)}.  f and isSatisfied do not depend on the Jacobian mode."""
    from graph_cases import _det
    from smooth_cases import stock_problem

    O = _det()[0]
    P = stock_problem(O, 1)
    out = {"O": O, "P": P}
    for name, make in (("ragged", ragged_batch), ("on_the_stamp", on_the_stamp_batch), ("still", still_batch), ("full", full_batch)):
        case = make(O, P)
        want = setpoints_py(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, case["period"], case.get("max_ticks", 65536), O=O, P=P)
        out[name] = dict(case=case, want=want)
    case = scene_case(O, P)
    out["scene"] = dict(case=case, want=case["want"])
    return out


def host_part(want):
    """what ccmp_setpoints_ref answers of a full expected result"""
    out = {k: want[k] for k in ("q", "qd", "tau", "tick_first", "status", "stretch")}  # (stretch takes the speed and acceleration peaks alone)
    out["peak"], out["peak_tick"] = want["peak"][:, :2], want["peak_tick"][:, :2]
    return out
