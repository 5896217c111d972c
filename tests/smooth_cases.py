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

The case builders at the end (rough_chain, wide_batch, long_batch, identity_batch, straddle_scene_case) need no device either: they make
the batches of tests/test_gpu_smooth_shapes.py from the oracle's samplers; tests/test_smooth_cases.py asserts what each must contain.
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
        self.mids, self.motions, self.list_lengths, self.changes = {}, {}, [], []  # changes: every d(w_i, c_i) that met min_change

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

    @staticmethod
    def from_midpoint(m, i):
        """the new neighbour a candidate's first test starts at, whose clearance the verdict reads: m_{i-1}"""
        return m[i - 1]

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
                ok = bool(self.clearance(self.from_midpoint(m, i)) >= self.margin and self.clearance(c) >= self.margin)
            if not ok:
                stats[REFUSED] += 1
                out.append(w[i])
                continue
            self.changes.append(float(self.distance(w[i], c)))
            if not self.changes[-1] > min_change:
                stats[BELOW] += 1
                out.append(w[i])
            else:
                u += 1
                out.append(c)
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


# ---- case builders (no device: the oracle alone; tests/test_smooth_cases.py asserts what each must contain) --------------------------------
OBJ = "Wine_Bottle"
WIDE_CYCLE = (3, 5, 0, 4, 1, 3, 2, 6, 3, 4)
WIDE_F, WIDE_LEN, WIDE_CAP, WIDE_STEPS = 70, 6, 9, 3
WIDE_NAN_PATH = 11  # 5 waypoints, a NaN in interior row 2
WIDE_SEED, LONG_SEED, IDENTITY_SEED = 0x5D00, 0x5E00, 0x5F00
LONG_LENS, LONG_CAP, LONG_STEPS = (70, 33, 2), 139, 2
IDENTITY_LENS = (0, 1, 2, 3, 64, 65, 66, 129, 130)
STRADDLE_SEED, STRADDLE_LEN, STRADDLE_VERTEX, STRADDLE_STEPS, STRADDLE_MARGIN = 0x6020, 5, 2, 2, 0.020522689572385112


def stock_problem(O, mode=0, obj=OBJ):
    """the oracle's own set-up of the fixture at the delta its path file was recorded with (test_gpu_smooth's `cons`)"""
    from conftest import load_cfg
    from dense_path_cases import RECORDED

    P = O.problem(load_cfg(obj))
    P.delta = RECORDED[obj]["delta"]
    P.jacobian_mode = mode
    return P


def rough_chain(O, P, n, seed):
    """n valid projected states: the first the first valid one of the oracle's sample_project stream `seed`, each further one the oracle's
    projected near-sample (distance 0.6, stream seed + j) of its predecessor, as arm_model_cases.waypoint_paths takes them; a sample whose
    projection fails or does not pass is_satisfied is replaced by the next sample index of its stream — never by a device result.  None
    when 64 samples in a row fail (a start state in a corner of the joint limits).  The chain is projected with the analytic Jacobian
    whatever P's mode (failed projections are what costs: the chains of the wide batch take the FD oracle 10 s, the analytic one 0.3 s):
    both modes run the same inputs, and is_satisfied does not depend on the mode"""
    P = type(P).from_buffer_copy(bytes(P))
    P.jacobian_mode = 1
    q, ok, _ = O.sample_project_batch(P, seed, 0, 64, 1)
    rows = [next(q[i] for i in range(64) if ok[i] == 1 and O.is_satisfied(P, q[i]))]
    for j in range(1, n):
        for index in range(64):
            good, y, _ = O.project(P, O.ambient_ref_batch(P, "near", seed + j, index, rows[-1], 0.6, 1)[0])
            y = O.enforce_bounds(y)
            if good and O.is_satisfied(P, y):
                break
        else:
            return None  # a start state none of whose near-samples projects: the caller takes another seed
        rows.append(y)
    return np.array(rows)


def rough_chains(O, P, lens, seed, stride):
    """one chain per length, from the seeds seed, seed + stride, ..; a seed whose chain gets stuck (rough_chain: None) is passed over"""
    chains = []
    while len(chains) < len(lens):
        rows = rough_chain(O, P, max(lens[len(chains)], 1), seed)
        seed += stride
        if rows is not None:
            chains.append(rows)
    return chains


def _batch(chains, lens, max_len):
    pj = np.full((len(lens), max_len, 14), np.nan)  # rows behind a path's length are NaN: never read
    for f, L in enumerate(lens):
        pj[f, :L] = chains[f][:L]
    return pj, np.array(lens, dtype=np.int32)


def wide_batch(O, P):
    """70 paths of up to 6 waypoints, lengths the cycle (3, 5, 0, 4, 1, 3, 2, 6, 3, 4), for a result of at most 9 vertices per path: a path of
    3 waypoints runs two passes, one of 4 or 5 one, one of 6 none.  Path 11 (5 waypoints) holds a NaN in interior row 2 (stop 4); every path
    shorter than 6 holds NaN only behind its length, which is not bad.  min_change is one of the distances d(w_i, c_i) the restatement meets in
    the first pass (the one an eighth up their order), so that vertex is BELOW and those above it are accepted.
    -> dict(pj, pl, max_steps, out_max_len, min_change, R: the restatement that met the distances, its midpoints memoised)"""
    lens = [WIDE_CYCLE[f % len(WIDE_CYCLE)] for f in range(WIDE_F)]
    pj, pl = _batch(rough_chains(O, P, lens, WIDE_SEED, 16), lens, WIDE_LEN)
    pj[WIDE_NAN_PATH, 2, 7] = np.nan
    R = Restatement(O, P)
    for f, L in enumerate(lens):
        if 3 <= L and 2 * L - 1 <= WIDE_CAP and f != WIDE_NAN_PATH:
            R.one_pass(pj[f, :L], 0.0, [0] * 5)
    first = sorted(R.changes)
    return dict(pj=pj, pl=pl, max_steps=WIDE_STEPS, out_max_len=WIDE_CAP, min_change=first[len(first) // 8], R=R)


def long_batch(O, P):
    """3 paths of 70, 33 and 2 waypoints for a result of at most 139 vertices and two passes: 70 -> 139 (stop 3 after one pass), 33 -> 65 ->
    129 (stop 2), 2 (stop 0).  The lengths summed cover 69, 138, 32 and 128 distances: a full 64-distance chunk and a partial one, two and
    a partial one, and exact multiples of 64"""
    pj, pl = _batch(rough_chains(O, P, LONG_LENS, LONG_SEED, 128), LONG_LENS, max(LONG_LENS))
    return dict(pj=pj, pl=pl, max_steps=LONG_STEPS, out_max_len=LONG_CAP, min_change=0.005)


def identity_batch():
    """9 paths of random finite joint vectors (on no manifold) of 0, 1, 2, 3, 64, 65, 66, 129 and 130 rows, run with max_steps 0: nothing is
    traversed, the rows come back, and the lengths sum 0, 0, 1, 2, 63, 64, 65, 128 and 129 distances"""
    rng = np.random.default_rng(IDENTITY_SEED)
    pj = rng.uniform(-2.5, 2.5, (len(IDENTITY_LENS), max(IDENTITY_LENS), 14))
    return dict(pj=pj, pl=np.array(IDENTITY_LENS, dtype=np.int32), max_steps=0, out_max_len=max(IDENTITY_LENS), min_change=0.005)


def identity_expect(case, fill):
    """the identity batch's result from its definition, no restatement: rows unchanged, out_len = L, stop 0 for L < 3 and 2 otherwise,
    both lengths the left-to-right edge_weight sum (+0.0 for L < 2)"""
    pj, pl = case["pj"], case["pl"]
    F, cap = len(pl), case["out_max_len"]
    out = {"joints": np.array(np.broadcast_to(fill, (F, cap, 14)), dtype=np.float64), "out_len": pl.copy(), "passes": np.zeros(F, dtype=np.int32),
           "moved": np.zeros(F, dtype=np.int32), "stop": np.where(pl < 3, 0, 2).astype(np.int32), "stats": np.zeros((F, 5), dtype=np.int32)}
    lengths = []
    for f, L in enumerate(pl):
        out["joints"][f, :L] = pj[f, :L]
        a = 0.0
        for r in range(1, int(L)):
            a = a + edge_weight(pj[f, r - 1], pj[f, r])
        lengths.append(a)
    out["length_in"], out["length_out"] = np.array(lengths), np.array(lengths)
    return out


def scene_restatement(O, P, scene, margin, cls=Restatement):
    """the restatement with a proxy scene: checkMotion behind the oracle's validity callback, the oracle's clearance of a state"""
    from test_gpu_geodesic_scene import OracleScene

    orc = OracleScene(O, P, scene, margin)

    def edge(a, b):
        r, _, n, _, _, _, _ = orc.edge(a, b, 4096)
        assert n <= 4096
        return r

    return cls(O, P, valid=edge, clearance=lambda x: O.clearance(P, scene.spheres, scene.boxes, scene.allowed, x)[0], margin=margin)


class WrongMidpoint(Restatement):
    """the rule with one index wrong: the clearance of the "from" midpoint taken at m_i instead of m_{i-1}"""

    @staticmethod
    def from_midpoint(m, i):
        return m[i]


def straddle_facts(O, P, scene, rows, margin):
    """first pass of one path with the scene: per interior vertex i (both checkMotion tests pass, clearance(m_{i-1}), clearance(m_i),
    clearance(c_i))"""
    R = scene_restatement(O, P, scene, margin)
    m = [R.mid(rows[i], rows[i + 1])[0] for i in range(len(rows) - 1)]
    facts = []
    for i in range(1, len(rows) - 1):
        c = R.mid(R.mid(m[i - 1], rows[i])[0], R.mid(rows[i], m[i])[0])[0]
        facts.append((R.check_motion(m[i - 1], c) and R.check_motion(c, m[i]), R.clearance(m[i - 1]), R.clearance(m[i]), R.clearance(c)))
    return facts


def straddle_scene_case(O, P, scene):
    """One stock path of 5 waypoints (rough_chain, seed 0x6020) with the default proxy scene and the margin 0.020522689572385112, found by a
    search over the seeds 0x6000, 0x6010, .. on the oracle alone.  In the first pass interior vertex 2 passes both checkMotion tests with the
    scene and clearance(c_2) = 0.022077 >= margin, while clearance(m_1) = 0.018500 < margin <= clearance(m_2) = 0.022545 (the margin is
    half their sum): the rule reads m_1 and refuses the vertex; a verdict that read m_2 would accept it.  Vertex 1 straddles the other
    way (clearance(m_0) = 0.023020): the rule accepts it, the wrong index refuses it.  Two passes accept 7 vertices.
    -> dict(pj, pl, max_steps, out_max_len, min_change, scene, margin)"""
    rows = rough_chain(O, P, STRADDLE_LEN, STRADDLE_SEED)
    cap = 2 ** STRADDLE_STEPS * (STRADDLE_LEN - 1) + 1
    return dict(pj=rows[None].copy(), pl=np.array([STRADDLE_LEN], dtype=np.int32), max_steps=STRADDLE_STEPS, out_max_len=cap, min_change=0.005, scene=scene,
                margin=STRADDLE_MARGIN)
