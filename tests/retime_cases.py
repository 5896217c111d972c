"""Resample and time stamps: a plain-Python restatement of the rule of csrc/ccmp_retime.h and the expected values the tests compare with.

The expected values are never the code under test.  A dense path is the det oracle's ONE uninterrupted `discrete_geodesic(a, b,
interpolate=True)` per segment, joined by dense_path_cases.join; its arcs are dense_path_cases.arc_py on graph_cases.edge_weight (the
library's rounding of the joint distance); the blend is the oracle's `interpolate`, the projection its `project`.  Everything else is
restated here, in Python floats (IEEE doubles, one rounding per operation, nothing fused):

    bracket      a LINEAR scan for the smallest k >= 1 with s_k >= h; t = (h - s_{k-1}) / (s_k - s_{k-1}); lower = (h - s_{k-1}) <= (s_k - h)
    resample     status in the order EMPTY, BROKEN, NONFINITE, POINT, FULL, OK; N = count or 1 + ceil(T / spacing); rows 0 and N-1 copied;
                 h_j = (j / (N-1)) * T; not h_j > 0: r_0; else the blend at the bracket, projected, or the nearer bracket row
    time stamps  V_i, the ceilings x_i, A and g = 2 A, the envelope y_i by an explicit DOUBLE LOOP over (i, k), dt_i, the left-to-right sum

The case builders at the end need no device: they make the batches of tests/test_gpu_retime.py from the oracle's samplers;
tests/test_retime_cases.py asserts what each must contain.
"""
import functools
import math

import numpy as np

from dense_path_cases import arc_py, join, oracle_segments
from graph_cases import edge_weight
from smooth_cases import bits, rough_chain, same_f64  # noqa: F401  (same_f64, bits: for the tests)

PROJECTED, FALLBACK, DEGENERATE, COPIED = range(4)
OK, EMPTY, BROKEN, NONFINITE, POINT, FULL = range(6)
INT32_MAX = 2 ** 31 - 1
INF = float("inf")

# the robot's data sheet, both arms (the package's PANDA_VELOCITY_LIMITS / PANDA_ACCELERATION_LIMITS twice); restated, not imported
PANDA_VMAX = ((2.175,) * 4 + (2.61,) * 3) * 2
PANDA_AMAX = (15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0) * 2


# ---- the rule ---------------------------------------------------------------------------------------------------------------------------
def bracket_py(arcs, h):
    """(k, t, lower) by the linear scan of the definition; needs 0 < h <= arcs[-1]"""
    s = [float(v) for v in arcs]
    assert 0.0 < h <= s[-1]
    k = next(k for k in range(1, len(s)) if s[k] >= h)
    below, above = h - s[k - 1], s[k] - h
    return k, below / (s[k] - s[k - 1]), below <= above


def count_py(T, count, spacing):
    """N of a path with T > 0, or None beyond INT32_MAX"""
    if count >= 2:
        return count
    q = T / spacing
    if math.isinf(q) or not math.ceil(q) < INT32_MAX:
        return None
    return max(1 + int(math.ceil(q)), 2)


def target_py(j, N, T):
    return (float(j) / float(N - 1)) * T


def targets_py(T, count, spacing, max_rows):
    """what ccmp_resample_targets_ref answers: (N, [h_0 .. h_{N-1}]); N = 1 when not T > 0, 0 for FULL"""
    if not T > 0.0:
        return 1, [0.0]
    N = count_py(T, count, spacing)
    if N is None or N > max_rows:
        return 0, []
    return N, [0.0] + [target_py(j, N, T) for j in range(1, N - 1)] + [T]


def _div(a, b):
    return INF if b == 0.0 else a / b  # positive / +0.0 = +inf in IEEE arithmetic; Python raises instead


def envelope_term(xk, g, dist):
    return xk + g * float(dist)


def envelope_py(x, g, with_own_term=True):
    """y_i = min over k of e(i, k), the explicit double loop"""
    y = []
    for i in range(len(x)):
        m = x[i] if with_own_term else INF
        for k in range(len(x)):
            if k != i:
                m = min(m, envelope_term(x[k], g, abs(i - k)))
        y.append(m)
    return y


def stamp_path_py(q, vmax, amax, beta):
    """one OK path of R >= 1 rows: (time, ceiling, envelope, g)"""
    R = len(q)
    if R == 1:
        return [0.0], [0.0], [0.0], INF
    d = [[float(q[i + 1][c]) - float(q[i][c]) for c in range(14)] for i in range(R - 1)]
    V = [min(_div(vmax[c], abs(d[i][c])) for c in range(14)) for i in range(R - 1)]
    A = min(_div((1.0 - beta) * amax[c], abs(d[i][c])) for i in range(R - 1) for c in range(14))
    g = 2.0 * A
    x = [0.0] * R
    for i in range(1, R - 1):
        curv = min(_div(beta * amax[c], abs(d[i][c] - d[i - 1][c])) for c in range(14))
        x[i] = min(V[i - 1] * V[i - 1], V[i] * V[i], curv)
    y = envelope_py(x, g)
    if R == 2:
        dt = [2.0 / math.sqrt(min(V[0] * V[0], 0.5 * g))]
    else:
        dt = [2.0 / (math.sqrt(y[i]) + math.sqrt(y[i + 1])) for i in range(R - 1)]
    t = [0.0]
    for v in dt:
        t.append(t[-1] + v)
    return t, x, y, g


def timestamps_py(rows, path_first, vmax, amax, beta=0.5, fill=float("nan")):
    """dict(time, ceiling, envelope (R,), duration, status (F,), g [F]); rows of a path that is not OK hold `fill`"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 14)
    F, R = len(path_first) - 1, len(rows)
    out = {k: np.full(R, fill) for k in ("time", "ceiling", "envelope")}
    out.update(duration=np.zeros(F), status=np.zeros(F, dtype=np.int32), g=[None] * F)
    for f in range(F):
        a, b = int(path_first[f]), int(path_first[f + 1])
        if b == a:
            out["status"][f], out["duration"][f] = EMPTY, 0.0
        elif not np.isfinite(rows[a:b]).all():
            out["status"][f], out["duration"][f] = NONFINITE, float("nan")
        else:
            t, x, y, g = stamp_path_py(rows[a:b], vmax, amax, beta)
            out["time"][a:b], out["ceiling"][a:b], out["envelope"][a:b], out["duration"][f], out["g"][f] = t, x, y, t[-1], g
    return out


class Restatement:
    """resample on the oracle's primitives.  P is the problem the dense paths are made with, project_problem (default P) the one the blends
    are projected with.  Projections are memoised per blend; `lowers` records the `lower` of every bracketed row, in order."""

    def __init__(self, O, P, project_problem=None, distance=edge_weight):
        self.O, self.P, self.PP, self.distance = O, P, project_problem if project_problem is not None else P, distance
        self.projected, self.lowers = {}, []

    def dense(self, pj, pl, distinct=False):
        """the dense form of F waypoint paths: dense_path_cases.join's dict plus arc and length"""
        d = join(pj, pl, pj.shape[1], oracle_segments(self.O, self.P, pj, pl), distinct)
        d["arc"], d["length"] = arc_py(d["rows"], d["path_first"], self.distance)
        return d

    def project(self, x):
        key = x.tobytes()
        if key not in self.projected:
            ok, y, _ = self.O.project(self.PP, x)
            self.projected[key] = (bool(ok), y)
        return self.projected[key]

    def row(self, r, s, h):
        """(row, kind) of the target arc h on the rows r with arcs s"""
        if not h > 0.0:
            return r[0], DEGENERATE
        k, t, lower = bracket_py(s, h)
        self.lowers.append(lower)
        ok, y = self.project(self.O.interpolate(r[k - 1], r[k], t))
        return (y, PROJECTED) if ok else (r[k - 1] if lower else r[k], FALLBACK)

    def resample(self, dense, count=0, spacing=None, max_rows=65536):
        spacing = self.P.delta if spacing is None else spacing
        pf = dense["path_first"]
        F = len(pf) - 1
        rows, kinds, first = [], [], [0]
        status, counts = np.zeros(F, dtype=np.int32), np.zeros((F, 4), dtype=np.int32)
        for f in range(F):
            r, s = dense["rows"][pf[f]:pf[f + 1]], dense["arc"][pf[f]:pf[f + 1]]
            new = []
            if len(r) == 0:
                status[f] = EMPTY
            elif any(sf >= 0 and ok == 0 for sf, ok in zip(dense["seg_first"][f], dense["seg_ok"][f])):
                status[f] = BROKEN
            elif not np.isfinite(r).all():
                status[f] = NONFINITE
            elif not float(s[-1]) > 0.0:
                status[f], new = POINT, [(r[0], COPIED)]
            else:
                T = float(s[-1])
                N = count_py(T, count, spacing)
                if N is None or N > max_rows:
                    status[f] = FULL
                else:
                    new = [(r[0], COPIED)] + [self.row(r, s, target_py(j, N, T)) for j in range(1, N - 1)] + [(r[-1], COPIED)]
            for y, kind in new:
                rows.append(np.array(y, dtype=np.float64))
                kinds.append(kind)
                counts[f, kind] += 1
            first.append(len(rows))
        out = dict(joints=np.array(rows, dtype=np.float64).reshape(-1, 14), path_first=np.array(first, dtype=np.int32), kind=np.array(kinds, dtype=np.uint8),
                   status=status, counts=counts)
        out["arc"], out["length"] = arc_py(out["joints"], out["path_first"], self.distance)
        return out


def same_sampled(got, want, what=""):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    for k in ("path_first", "status", "counts", "kind"):
        assert np.array_equal(g[k], want[k]), (what, k, g[k], want[k])
    for k in ("joints", "arc", "length"):
        assert g[k].shape == want[k].shape and same_f64(g[k], want[k]), (what, k, np.argwhere(bits(g[k]) != bits(want[k]))[:5])


def same_stamps(got, want, what="", keys=("time", "duration", "ceiling", "envelope")):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    assert np.array_equal(g["status"], want["status"]), (what, g["status"], want["status"])
    for k in keys:
        assert g[k].shape == want[k].shape and same_f64(g[k], want[k]), (what, k, np.argwhere(bits(g[k]) != bits(want[k]))[:5])


def interior_projected_share(res):
    """the share of PROJECTED among the rows that were bracketed or degenerate (everything but the copies)"""
    c = res["counts"].sum(axis=0)
    inner = int(c[PROJECTED] + c[FALLBACK] + c[DEGENERATE])
    return 1.0 if inner == 0 else float(c[PROJECTED]) / inner


# ---- case builders (no device: the oracle alone; tests/test_retime_cases.py asserts what each must contain) ----------------------------
RAGGED_SEED, WIDE_SEED, LONG_SEED, FALLBACK_SEED, STILL_SEED = 0x7100, 0x7200, 0x7300, 0x7400, 0x7500
RAGGED_LENS = (0, 1, 2, 3, 2, 3, 4)
RAGGED_SIZES = (0, 1, 2, 3, 17, 64, 65)  # rows out of path f: none, the POINT's one, then count = the size
WIDE_F, WIDE_MAX_LEN, WIDE_SPACING = 70, 5, 0.125
WIDE_BROKEN, WIDE_POINT, WIDE_NONFINITE, WIDE_FULL = 7, 13, 21, 33
LONG_LEN, LONG_COUNT = 5, 130
FALLBACK_LEN, FALLBACK_COUNT, FALLBACK_TOLERANCE = 3, 17, 1e-300


def _batch(chains, lens, max_len):
    pj = np.full((len(lens), max_len, 14), np.nan)  # rows behind a path's length are NaN: never read
    for f, L in enumerate(lens):
        pj[f, :L] = chains[f][:L]
    return pj, np.array(lens, dtype=np.int32)


def traversable_chains(O, P, lens, seed, stride):
    """one chain of projected states per length (smooth_cases.rough_chain, seeds seed, seed + stride, ..), every segment of which the
    oracle traverses to its end in both Jacobian modes; a seed whose chain gets stuck or has a segment that does not is passed over"""
    modes = []
    for mode in (0, 1):
        Pm = type(P).from_buffer_copy(bytes(P))
        Pm.jacobian_mode = mode
        modes.append(Pm)
    chains = []
    while len(chains) < len(lens):
        n = max(lens[len(chains)], 1)
        rows = rough_chain(O, P, n, seed)
        seed += stride
        if rows is not None and all(O.discrete_geodesic(Pm, rows[i], rows[i + 1], interpolate=True, max_states=1024)[0] for Pm in modes for i in range(n - 1)):
            chains.append(rows)
    return chains


def ragged_batch(O, P):
    """7 waypoint paths of 0, 1, 2, 3, 2, 3 and 4 waypoints.  Resampled in count mode with count = 2, 3, 17, 64 and 65 every path of two or
    more waypoints gets that many rows, the empty path none and the one-waypoint path (no length: POINT) one — the sizes 0, 1, 2, 3, 17,
    64, 65 where the index arithmetic and the 64-interval chunk of the stamps can go wrong (2 rows: the pair rule; 3: one interior row;
    64 and 65 rows: 63 and 64 intervals, one short of a chunk and exactly one).  `ragged_rows` packs one path of every size.
    -> dict(pj, pl, counts)"""
    pj, pl = _batch(traversable_chains(O, P, RAGGED_LENS, RAGGED_SEED, 16), RAGGED_LENS, max(RAGGED_LENS))
    return dict(pj=pj, pl=pl, counts=tuple(s for s in RAGGED_SIZES if s >= 2))


def ragged_rows(resampled_by_count):
    """packed rows of 0, 1, 2, 3, 17, 64 and 65 rows: path f of the ragged batch as resampled with count = RAGGED_SIZES[f] (paths 0 and 1: by
    any count).  resampled_by_count: {count: the resample result}.  -> (rows, path_first)"""
    rows, first = [], [0]
    for f, size in enumerate(RAGGED_SIZES):
        res = resampled_by_count[size if size >= 2 else 2]
        a, b = res["path_first"][f], res["path_first"][f + 1]
        assert b - a == size, (f, size, b - a)
        rows.extend(res["joints"][a:b])
        first.append(len(rows))
    return np.array(rows, dtype=np.float64).reshape(-1, 14), np.array(first, dtype=np.int32)


def wide_batch(O, P):
    """70 short paths (2 or 3 waypoints; more paths than a block holds rows) for spacing mode at 0.125.  Path 7 is BROKEN: its second
    waypoint is the first state of another chain, which the traversal does not reach (seg_ok 0, as the recorded Wine_Bottle waypoints
    have).  Path 13 is a POINT: two equal waypoints.  Path 21 is NONFINITE: one waypoint with a NaN (no segment, so not BROKEN).  Path 33
    has 5 waypoints and is FULL under max_rows = the most rows any other path gets.
    -> dict(pj, pl, spacing, max_rows) — max_rows from the restatement's own lengths"""
    lens = [2 + (f % 3 == 1) for f in range(WIDE_F)]
    lens[WIDE_NONFINITE], lens[WIDE_FULL], lens[WIDE_POINT] = 1, WIDE_MAX_LEN, 2
    chains = traversable_chains(O, P, lens, WIDE_SEED, 16)
    pj, pl = _batch(chains, lens, WIDE_MAX_LEN)
    pj[WIDE_BROKEN, 1] = chains[WIDE_BROKEN + 1][0]
    pj[WIDE_POINT, 1] = pj[WIDE_POINT, 0]
    pj[WIDE_NONFINITE, 0, 9] = np.nan
    d = Restatement(O, P).dense(pj, pl)
    ordinary = [f for f in range(WIDE_F) if f not in (WIDE_BROKEN, WIDE_POINT, WIDE_NONFINITE, WIDE_FULL)]
    max_rows = max(count_py(float(d["length"][f]), 0, WIDE_SPACING) for f in ordinary)
    return dict(pj=pj, pl=pl, spacing=WIDE_SPACING, max_rows=max_rows)


def long_path(O, P):
    """one path of 5 waypoints resampled to 130 rows: 129 intervals, two full chunks of the stamps and one interval more"""
    pj, pl = _batch(traversable_chains(O, P, (LONG_LEN,), LONG_SEED, 16), (LONG_LEN,), LONG_LEN)
    return dict(pj=pj, pl=pl, count=LONG_COUNT)


def strict_problem(P):
    """P with tolerances no iterate meets: every projection fails"""
    P2 = type(P).from_buffer_copy(bytes(P))
    P2.tol_pos = P2.tol_rot = FALLBACK_TOLERANCE
    return P2


def fallback_case(O, P):
    """one path of 3 waypoints, densified with P and resampled to 17 rows with a second problem whose tolerances (1e-300) make the
    projection of every blend fail: every interior row is a FALLBACK, and rows nearer to the lower and to the upper bracket row both occur
    -> dict(pj, pl, count, tolerance, want: the restatement's result)"""
    pj, pl = _batch(traversable_chains(O, P, (FALLBACK_LEN,), FALLBACK_SEED, 16), (FALLBACK_LEN,), FALLBACK_LEN)
    R = Restatement(O, P, project_problem=strict_problem(P))
    want = R.resample(R.dense(pj, pl), count=FALLBACK_COUNT)
    assert (want["kind"][1:-1] == FALLBACK).all() and want["counts"][0].tolist() == [0, FALLBACK_COUNT - 2, 0, 2], want["counts"]
    assert True in R.lowers and False in R.lowers, R.lowers
    return dict(pj=pj, pl=pl, count=FALLBACK_COUNT, tolerance=FALLBACK_TOLERANCE, want=want)


def still_rows():
    """packed rows with repeated states (random joint vectors, on no manifold: time stamps ask for none): zero differences make ceilings
    +inf, and where every row of a path is equal A and g are +inf.  Paths: a a b b c | a a a | a a | a b b | a b a | a
    -> (rows, path_first)"""
    rng = np.random.default_rng(STILL_SEED)
    a, b, c = rng.uniform(-2.5, 2.5, (3, 14))
    paths = [[a, a, b, b, c], [a, a, a], [a, a], [a, b, b], [a, b, a], [a]]
    first = np.cumsum([0] + [len(p) for p in paths]).astype(np.int32)
    return np.array([r for p in paths for r in p]), first


def targets():
    """(T, count, spacing, max_rows) of the count / spacing arithmetic: count mode; spacing dividing T exactly, just not, and by far not; a
    quotient whose ceiling is 1; N at and one over max_rows; no length; a NaN length; a spacing so small that N passes INT32_MAX; a
    subnormal spacing (the quotient overflows)"""
    return [(1.0, 2, 0.0, 65536), (3.7, 17, 0.0, 65536), (3.7, 65, -1.0, 65), (3.7, 66, 0.25, 65), (2.0, 0, 0.25, 65536), (2.0, 0, 0.3, 65536),
            (0.7853981633974483, 0, 0.1, 65536), (0.1, 0, 0.25, 65536), (1e-300, 0, 0.25, 65536), (2.0, 0, 0.25, 9), (2.0, 0, 0.25, 8), (0.0, 0, 0.25, 65536),
            (0.0, 5, 0.0, 65536), (float("nan"), 0, 0.25, 65536), (1.0, 0, 1e-10, 2 ** 31 - 1), (1.0, 0, 5e-324, 65536), (3.0, 0, 1.0, 4)]


@functools.lru_cache(maxsize=None)
def reference(mode):
    """every batch above with its expected results under the stock problem in Jacobian mode `mode`, computed once per process and shared by
    the tests that need it (never changed by them): {name: dict(case, dense, want ...)}"""
    from graph_cases import _det
    from smooth_cases import stock_problem

    O = _det()[0]
    P = stock_problem(O, mode)
    R = Restatement(O, P)
    out = {"O": O, "P": P}
    case = ragged_batch(O, P)
    dense = R.dense(case["pj"], case["pl"])
    want = {c: R.resample(dense, count=c) for c in case["counts"]}
    out["ragged"] = dict(case=case, dense=dense, distinct=R.dense(case["pj"], case["pl"], distinct=True), want=want, rows=ragged_rows(want))
    case = wide_batch(O, P)
    dense = R.dense(case["pj"], case["pl"])
    out["wide"] = dict(case=case, dense=dense, want=R.resample(dense, spacing=case["spacing"], max_rows=case["max_rows"]))
    case = long_path(O, P)
    dense = R.dense(case["pj"], case["pl"])
    out["long"] = dict(case=case, dense=dense, want=R.resample(dense, count=case["count"]))
    out["fallback"] = dict(case=fallback_case(O, P))
    return out
