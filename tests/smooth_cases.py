"""Smooth solution paths: a plain-Python restatement of the rule of csrc/ccmp_smooth.h and the expected values the tests compare with.

The expected values are never the code under test.  A pair's closed list is the det oracle's ONE uninterrupted
`discrete_geodesic(a, b, interpolate=True, max_states=4096)` followed by b; the blend is the oracle's `interpolate`, the projection its
`project`, a checkMotion its `is_satisfied(target)` followed by one uninterrupted traversal.  Everything else is restated here:

    arcs       s_0 = +0.0, s_k = s_{k-1} + d(row_{k-1}, row_k), d the joint distance in the library's rounding (graph_cases.edge_weight:
               an exactly rounded FMA chain and sqrt), summed as dense_path_cases.arc_py sums
    midpoint   T = s_{n-1}, h = 0.5 T; not T > 0: a (degenerate); k = the smallest k >= 1 with s_k >= h, t = (h - s_{k-1}) / (s_k - s_{k-1});
               x = interpolate(row_{k-1}, row_k, t); (y, ok) = project(x); ok: y; else row_{k-1} when h - s_{k-1} <= s_k - h, else row_k
    pass       m_i = mid(w_i, w_{i+1}); c_i = mid(mid(m_{i-1}, w_i), mid(w_i, m_i)); accepted iff both checkMotions pass (with a scene:
               and the two clearances >= margin), else refused; then iff d(w_i, c_i) > min_change, else below
    loop       non-finite: stop 4; L < 3: 0; before a pass: max_steps run: 2, 2L - 1 > out_max_len: 3; after a pass with u == 0: 1
"""
import math

import numpy as np

from dense_path_cases import arc_py
from graph_cases import edge_weight

PROJECTED, FALLBACK, DEGENERATE, REFUSED, BELOW = range(5)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_f64(a, b):
    """bit for bit, except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def arcs_of(rows, distance=edge_weight):
    return arc_py(rows, [0, len(rows)], distance)[0]


def bracket_py(rows, arcs):
    """(k, t, blend operands' fallback row) of a closed list, or None for a degenerate one; the linear scan of the definition"""
    T = float(arcs[-1])
    if not T > 0.0:
        return None
    h = 0.5 * T
    k = next(k for k in range(1, len(arcs)) if arcs[k] >= h)
    below, above = h - float(arcs[k - 1]), float(arcs[k]) - h
    return k, below / (float(arcs[k]) - float(arcs[k - 1])), (k - 1 if below <= above else k)


class Restatement:
    """the rule on the oracle's primitives; memoised per (a, b) bit pattern, list lengths recorded (how many lists an extend call of a
    given chunk cannot finish)"""

    def __init__(self, O, P, valid=None, clearance=None, margin=None, distance=edge_weight):
        self.O, self.P, self.distance = O, P, distance
        self.edge, self.clearance, self.margin = valid, clearance, margin  # edge(a, b) -> ok of one scene traversal
        self.mids, self.motions, self.list_lengths = {}, {}, []

    def closed_list(self, a, b):
        _, st, _ = self.O.discrete_geodesic(self.P, a, b, interpolate=True, max_states=4096)
        self.list_lengths.append(len(st))
        return np.vstack([st, np.asarray(b, dtype=np.float64)[None]])

    def mid(self, a, b):
        """(midpoint, kind)"""
        key = (np.asarray(a).tobytes(), np.asarray(b).tobytes())
        if key not in self.mids:
            rows = self.closed_list(a, b)
            br = bracket_py(rows, arcs_of(rows, self.distance))
            if br is None:
                self.mids[key] = (np.array(a, dtype=np.float64), DEGENERATE)
            else:
                k, t, fb = br
                ok, y, _ = self.O.project(self.P, self.O.interpolate(rows[k - 1], rows[k], t))
                self.mids[key] = (y, PROJECTED) if ok else (rows[fb].copy(), FALLBACK)
        return self.mids[key]

    def check_motion(self, a, b):
        key = (np.asarray(a).tobytes(), np.asarray(b).tobytes())
        if key not in self.motions:
            if not self.O.is_satisfied(self.P, b):
                self.motions[key] = False
            elif self.edge is not None:
                self.motions[key] = bool(self.edge(a, b))
            else:
                self.motions[key] = bool(self.O.discrete_geodesic(self.P, a, b, max_states=4096)[0])
        return self.motions[key]

    def one_pass(self, w, min_change, stats):
        """(new path (2L-1,14), u)"""
        L = len(w)

        def mid(a, b):
            y, kind = self.mid(a, b)
            stats[kind] += 1
            return y

        m = [mid(w[i], w[i + 1]) for i in range(L - 1)]
        out, u = [w[0]], 0
        for i in range(1, L):
            out.append(m[i - 1])
            if i == L - 1:
                out.append(w[i])
                break
            c = mid(mid(m[i - 1], w[i]), mid(w[i], m[i]))
            ok = self.check_motion(m[i - 1], c) and self.check_motion(c, m[i])  # both traversals run on the device; the verdict is the same
            if ok and self.clearance is not None:
                ok = bool(self.clearance(m[i - 1]) >= self.margin and self.clearance(c) >= self.margin)
            if not ok:
                stats[REFUSED] += 1
            elif not self.distance(w[i], c) > min_change:
                stats[BELOW] += 1
            else:
                u += 1
                out.append(c)
                continue
            out.append(w[i])
        return np.array(out), u

    def length(self, rows):
        a = 0.0
        for r in range(1, len(rows)):
            a = a + float(self.distance(rows[r - 1], rows[r]))
        return a

    def smooth(self, rows, max_steps, min_change, out_max_len):
        """one path: dict(rows, passes, moved, stop, stats, length_in, length_out)"""
        w = np.array(rows, dtype=np.float64).reshape(-1, 14)
        stats, passes, moved = [0] * 5, 0, 0
        lin = self.length(w)
        if not np.isfinite(w).all():
            stop = 4
        elif len(w) < 3:
            stop = 0
        else:
            while True:
                if passes >= max_steps:
                    stop = 2
                    break
                if 2 * len(w) - 1 > out_max_len:
                    stop = 3
                    break
                w, u = self.one_pass(w, min_change, stats)
                passes += 1
                moved += u
                if u == 0:
                    stop = 1
                    break
        return dict(rows=w, passes=passes, moved=moved, stop=stop, stats=stats, length_in=lin, length_out=self.length(w))


def expect(R, path_joints, path_len, max_steps, min_change, out_max_len, fill):
    """the whole result for F paths as the library lays it out; rows behind out_len hold `fill(f)` (F,out_max_len,14 array or scalar)"""
    pj = np.asarray(path_joints, dtype=np.float64)
    F = pj.shape[0]
    out = {"joints": np.array(np.broadcast_to(fill, (F, out_max_len, 14)), dtype=np.float64), "out_len": np.zeros(F, dtype=np.int32),
           "passes": np.zeros(F, dtype=np.int32), "moved": np.zeros(F, dtype=np.int32), "stop": np.zeros(F, dtype=np.int32),
           "length_in": np.zeros(F), "length_out": np.zeros(F), "stats": np.zeros((F, 5), dtype=np.int32)}
    for f in range(F):
        r = R.smooth(pj[f, : int(path_len[f])], max_steps, min_change, out_max_len)
        n = len(r["rows"])
        out["joints"][f, :n] = r["rows"]
        out["out_len"][f], out["passes"][f], out["moved"][f], out["stop"][f] = n, r["passes"], r["moved"], r["stop"]
        out["length_in"][f], out["length_out"][f], out["stats"][f] = r["length_in"], r["length_out"], r["stats"]
    return out


def same_result(got, want, what=""):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    for k in ("out_len", "passes", "moved", "stop", "stats"):
        if k in g:
            assert np.array_equal(g[k], want[k]), (what, k, g[k], want[k])
    for k in ("length_in", "length_out"):
        assert same_f64(g[k], want[k]), (what, k, g[k], want[k])
    assert g["joints"].shape == want["joints"].shape, (what, g["joints"].shape, want["joints"].shape)
    assert same_f64(g["joints"], want["joints"]), (what, np.argwhere(bits(g["joints"]) != bits(want["joints"]))[:5])


def mirror_fill(path_joints, out_max_len):
    """what the mirror's outputs start as: the input's rows, zeros behind"""
    pj = np.asarray(path_joints, dtype=np.float64)
    fill = np.zeros((pj.shape[0], out_max_len, 14))
    fill[:, : pj.shape[1]] = pj
    return fill
