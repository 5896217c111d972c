"""Shared cases of the RRT-Connect tests (tests/test_rrtc_*.py, tests/test_gpu_rrtc.py).

Three things: a plain-Python restatement of the rule that csrc/ccmp_rrtc.h states (the arc's fold, the pick of step 2 and of step 3, the
commit's total order, the best gap, FULL, the solution test) on the state dict that `RRTConnect.state()` returns; builders of synthetic
traversal lists with a prescribed arc; and `HandRRTConnect`, a driver that runs the whole loop BY HAND over the public mirror calls
(sample, nearest_in_tree, traversal, rrtc_pick_ref, append, add_edges, labels) with the commit and the state update taken on the host by
the restatement.  The sequence is the one include/ccmp.h states for ccmp_rrtc_*; `RRTConnect` must leave the same bits."""
import copy

import numpy as np

OPEN, SOLVED, BUDGET, FULL = range(4)
NONE, TRAPPED, ADVANCED, REACHED, UNSETTLED = -1, 0, 1, 2, 3
C_NOTHING, C_ADDED, C_JOINED = range(3)
COUNTERS = ("samples", "projected", "trapped", "advanced", "reached", "unsettled", "connect_reached", "connect_added", "connect_nothing", "vertices", "edges")


def new_state(starts, goals, first_index=0):
    return {"starts": [int(v) for v in starts], "goals": [int(v) for v in goals], "status": OPEN, "cycle": 0, "next_index": int(first_index), "solved_start": -1,
            "solved_goal": -1, "best_a": -1, "best_b": -1, "best_gap": float("inf"), "counters": {n: 0 for n in COUNTERS}}


def full(size, width, max_vertices):
    return size + 2 * width > max_vertices


def dist(a, b):
    from closed_chain_motion_planner_amd import joint_distance

    return joint_distance(np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64))


def arc(rows, rng):
    """the fold over the listed rows: (j, s_j, nan) with j the largest index whose partial sum is <= rng (0: the first row)"""
    s, j, s_j, nan = 0.0, 0, 0.0, False
    for i in range(1, len(rows)):
        s = s + dist(rows[i - 1], rows[i])
        if s != s:
            nan = True
        elif s <= rng:
            j, s_j = i, s
    return j, s_j, nan


def extend(rows, n_states, max_states, ok, d, rng, use=1):
    """step 2's pick of one sample: (outcome, row index or -1); rows: the stored states (max_states, 14)"""
    if use == 0:
        return NONE, -1
    m = 0 if use != 1 else max(0, min(int(n_states), max_states))
    j, _, nan = arc(rows[:m], rng)
    if nan or d != d or not rng > 0.0 or m < 1:
        return TRAPPED, -1
    cut = n_states > max_states or ok == 2
    if d <= rng:
        return (REACHED if ok == 1 else UNSETTLED if cut else TRAPPED), -1
    if m < 2:
        return TRAPPED, -1
    jj = max(j, 1)
    if cut and jj == m - 1 and j >= 1:
        return UNSETTLED, -1
    return ADVANCED, jj


def connect(rows, n_states, max_states, ok, v, use=1):
    """step 3's pick of one produced vertex v: (outcome, row index or -1, gap)"""
    if use == 0:
        return NONE, -1, float("nan")
    m = 0 if use != 1 else max(0, min(int(n_states), max_states))
    gap = dist(rows[m - 1], v) if m > 0 else float("nan")
    if m < 1 or gap != gap:
        return C_NOTHING, -1, gap
    if ok == 1:
        return C_JOINED, -1, gap
    if m < 2:
        return C_NOTHING, -1, gap
    return C_ADDED, m - 1, gap


def pick(mode, states, n_states, ok, to, d=None, use=None, rng=0.1):
    """the restatement over E lists, in the shape of `rrtc_pick_ref`'s dict"""
    E, ms = states.shape[0], states.shape[1]
    out = {"outcome": np.empty(E, dtype=np.int32), "row_index": np.empty(E, dtype=np.int32), "row": np.zeros((E, 14)), "gap": np.full(E, np.nan)}
    for e in range(E):
        u = 1 if use is None else int(use[e])
        if mode == 0:
            o, r = extend(states[e], n_states[e], ms, ok[e], d[e], rng, u)
            if o == REACHED:
                out["row"][e] = to[e]
        else:
            o, r, out["gap"][e] = connect(states[e], n_states[e], ms, ok[e], to[e], u)
        if r >= 0:
            out["row"][e] = states[e, r]
        out["outcome"][e], out["row_index"][e] = o, r
    return out


def commit(state, N, a_is_start, use_a, pa, idx_a, pb, idx_b):
    """step 4 on the host: (new state, rows (V,14), uv (2 W,2) int32 with (-1,-1) where a sample gives no edge).  pa / pb: the dicts of
    the picks of step 2 / step 3; idx_a / idx_b: their nearest vertices.  New indices: step 2's vertices in ascending sample order, then
    step 3's in ascending sample order."""
    s = copy.deepcopy(state)
    W = len(use_a)
    oa, ob = pa["outcome"], pb["outcome"]
    keep_a = [oa[e] in (ADVANCED, REACHED) for e in range(W)]
    keep_b = [keep_a[e] and ob[e] == C_ADDED for e in range(W)]
    joined = [keep_a[e] and ob[e] == C_JOINED for e in range(W)]
    n_a, n_b = sum(keep_a), sum(keep_b)
    uv = np.full((2 * W, 2), -1, dtype=np.int32)
    rows = np.zeros((n_a + n_b, 14))
    v_a, v_b, ia, ib = [-1] * W, [-1] * W, 0, 0
    for e in range(W):
        if keep_a[e]:
            v_a[e] = N + ia
            rows[ia] = pa["row"][e]
            uv[e] = (idx_a[e], v_a[e])
            ia += 1
    for e in range(W):
        if keep_b[e]:
            v_b[e] = N + n_a + ib
            rows[n_a + ib] = pb["row"][e]
            uv[W + e] = (idx_b[e], v_b[e])
            ib += 1
        elif joined[e]:
            uv[W + e] = (idx_b[e], v_a[e])
    c = s["counters"]
    c["samples"] += W
    c["projected"] += int(sum(1 for e in range(W) if use_a[e]))
    for name, code in (("trapped", TRAPPED), ("advanced", ADVANCED), ("reached", REACHED), ("unsettled", UNSETTLED)):
        c[name] += int(sum(1 for e in range(W) if oa[e] == code))
    n_a, n_b, n_j = int(n_a), int(n_b), int(sum(joined))
    c["connect_reached"] += n_j
    c["connect_added"] += n_b
    c["connect_nothing"] += int(sum(1 for e in range(W) if keep_a[e] and ob[e] == C_NOTHING))
    c["vertices"] += n_a + n_b
    c["edges"] += n_a + n_b + n_j
    for e in range(W):  # the smallest gap so far, strict, samples in ascending order
        g = float(pb["gap"][e])
        if keep_a[e] and g == g and g < s["best_gap"]:
            b_end = v_b[e] if keep_b[e] else int(idx_b[e])
            s["best_gap"] = g
            s["best_a"], s["best_b"] = (v_a[e], b_end) if a_is_start else (b_end, v_a[e])
    s["next_index"] += W
    return s, rows, uv


def connected(labels, state):
    s = copy.deepcopy(state)
    if s["status"] == SOLVED:
        return s
    N = len(labels)
    for a in s["starts"]:
        for b in s["goals"]:
            if 0 <= a < N and 0 <= b < N and labels[a] == labels[b]:
                s["status"], s["solved_start"], s["solved_goal"] = SOLVED, int(a), int(b)
                return s
    return s


def state_bits(s):
    """a state dict as a tuple that compares bit for bit (floats by their bytes)"""
    return (tuple(s["starts"]), tuple(s["goals"]), s["status"], s["cycle"], s["next_index"], s["solved_start"], s["solved_goal"], s["best_a"], s["best_b"],
            np.float64(s["best_gap"]).tobytes(), tuple(s["counters"][n] for n in COUNTERS))


# ---- synthetic lists --------------------------------------------------------------------------------------------------------------------
def line_list(steps, max_states, origin=0.25):
    """a list whose consecutive rows differ in joint 0 alone by exactly `steps` (values with few mantissa bits, so the partial sums are
    exact): rows (max_states, 14), the unused rows NaN-free junk that must not be read into a decision"""
    rows = np.full((max_states, 14), 7.0)
    x = origin
    n = min(len(steps) + 1, max_states)
    for i in range(n):
        rows[i] = np.linspace(0.0, 0.4, 14)
        rows[i, 0] = x
        if i < len(steps):
            x = x + steps[i]
    return rows


def synthetic_cases(max_states=4):
    """(name, rows, n_states, ok, d, range) of step 2 — every n_states in {0, 1, 2, 3, max_states, max_states + 1}, ok in {0, 1, 2}, d below,
    at and above the range, the shapes a blocked list has (ok 0, not full), a range that equals a partial sum, a first step beyond the
    range, a NaN row"""
    ms, rng = max_states, 0.5
    cases = []
    steps = [0.25, 0.25, 0.125, 0.125, 0.25, 0.25]
    for ns in (0, 1, 2, 3, ms, ms + 1):
        for ok in (0, 1, 2):
            for d in (0.25, 0.5, 0.75):
                cases.append(("ns%d ok%d d%g" % (ns, ok, d), line_list(steps, ms), ns, ok, d, rng))
    cases.append(("range equals s_2: <= keeps row 2", line_list([0.25, 0.25, 0.25], ms), 4, 0, 2.0, 0.5))
    cases.append(("range equals the last stored row's sum, full list: unsettled", line_list([0.125, 0.125, 0.25, 0.25], ms), ms + 1, 0, 2.0, 0.5))
    cases.append(("range equals the last stored row's sum, whole list: advanced", line_list([0.125, 0.125, 0.25], ms), ms, 0, 2.0, 0.5))
    cases.append(("range just below s_2: row 1", line_list([0.25, 0.25, 0.25], ms), 4, 0, 2.0, 0.4999999999999999))
    cases.append(("first step beyond the range: row 1, advanced", line_list([0.75, 0.25], ms), 3, 0, 2.0, 0.5))
    cases.append(("first step beyond the range, full list", line_list([0.75, 0.25, 0.25, 0.25], ms), ms + 1, 0, 2.0, 0.5))
    cases.append(("blocked after one step (ok 0, short list)", line_list([0.125], ms), 2, 0, 2.0, 0.5))
    cases.append(("blocked, within delta of the target (ok 1)", line_list([0.125], ms), 2, 1, 2.0, 0.5))
    cases.append(("suspended inside the range", line_list([0.125, 0.125], ms), 3, 2, 2.0, 0.5))
    cases.append(("suspended beyond the range", line_list([0.25, 0.5], ms), 3, 2, 2.0, 0.5))
    bad = line_list([0.125, 0.125, 0.125], ms)
    bad[2, 5] = np.nan
    cases.append(("a NaN row", bad, 4, 0, 2.0, 0.5))
    cases.append(("a NaN distance", line_list(steps, ms), 3, 1, float("nan"), 0.5))
    return cases


def stack_cases(cases):
    """the arrays `rrtc_pick_ref` takes from a list of cases of one max_states; the sample rows are distinct from every listed row"""
    states = np.stack([c[1] for c in cases])
    ns = np.array([c[2] for c in cases], dtype=np.int32)
    ok = np.array([c[3] for c in cases], dtype=np.uint8)
    d = np.array([c[4] for c in cases])
    to = np.tile(np.linspace(1.0, 2.0, 14), (len(cases), 1)) + np.arange(len(cases))[:, None] * 0.5
    return states, ns, ok, to, d


# ---- nearest vertex of a tree ---------------------------------------------------------------------------------------------------------
def brute_nearest(joints, labels, roots, queries):
    """numpy over ccmp_joint_distance: ranking by (distance, index), NaN never a candidate, (-1, inf) for an empty tree"""
    N = len(joints)
    want = {int(labels[r]) for r in roots if 0 <= r < N}
    idx, out = np.full(len(queries), -1, dtype=np.int32), np.full(len(queries), np.inf)
    for q, x in enumerate(queries):
        for j in range(N):
            if int(labels[j]) not in want:
                continue
            dj = dist(joints[j], x)
            if dj == dj and dj < out[q]:  # strict, j ascending: a tie stays with the lower index
                idx[q], out[q] = j, dj
    return idx, out


def tree_store(N, seed=5):
    """N joint rows with duplicates and NaN (pose-only) rows mixed in: row 0 is finite; every 7th row from 3 on is NaN; rows 5 k + 2 repeat
    row 5 k"""
    r = np.random.default_rng(seed + N)
    j = r.uniform(-2.0, 2.0, size=(N, 14))
    for i in range(2, N, 5):
        j[i] = j[i - 2]
    for i in range(3, N, 7):
        j[i] = np.nan
    return j


def tree_edges(N, stride):
    """edges (i, i + stride): `stride` components, vertex v in component v % stride"""
    return np.array([(i, i + stride) for i in range(N - stride)], dtype=np.int32).reshape(-1, 2)


def tree_queries(joints, Q, seed=9):
    """Q query rows: every third one a copy of a store row (a zero distance, and a tie where the row is duplicated)"""
    r = np.random.default_rng(seed + Q)
    q = r.uniform(-2.0, 2.0, size=(Q, 14))
    fin = np.flatnonzero(np.isfinite(joints).all(axis=1))
    for i in range(0, Q, 3):
        q[i] = joints[fin[(i * 7) % len(fin)]]
    return q


# ---- the loop by hand -------------------------------------------------------------------------------------------------------------------
class HandRRTConnect:
    """the cycle over the mirror's calls, the commit and the state on the host (needs a device)"""

    def __init__(self, rm, c, starts, goals, scene=None, margin=0.0, width=32, range=0.1, rng_seed=0, first_index=0, max_states=64, round_budget=0,
                 max_vertices=2**31 - 1):
        import torch

        self.torch = torch
        self.rm, self.c, self.scene, self.margin = rm, c, scene, float(margin) if scene is not None else 0.0
        self.W, self.range, self.seed, self.ms, self.budget, self.max_vertices = int(width), float(range), rng_seed, int(max_states), int(round_budget), max_vertices
        self.seen = set()  # (step, outcome) pairs that occurred, for the coverage assertion
        self.state = connected(rm.labels(host=True), new_state(starts, goals, first_index))

    def _dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def _traverse(self, frm, to):
        c = self.c
        if self.scene is not None:
            out = c.discrete_geodesic_scene_batch(self._dev(frm), self._dev(to), self.scene, self.margin, max_states=self.ms, want_carry=True,
                                                  round_budget=self.budget)
        else:
            out = c.discrete_geodesic_batch(self._dev(frm), self._dev(to), max_states=self.ms, want_carry=True, round_budget=self.budget)
        return out[0].cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()

    def _edges(self, idx, rows, flags, joints):
        use = np.where(flags, np.where(idx >= 0, 1, 2), 0).astype(np.uint8)
        frm, to = np.zeros((self.W, 14)), np.zeros((self.W, 14))
        on = use == 1
        frm[on], to[on] = joints[idx[on]], rows[on]
        return use, frm, to

    def cycle(self):
        """one cycle; returns False when the loop has ended (SOLVED, FULL)"""
        from closed_chain_motion_planner_amd import rrtc_pick_ref

        rm, c, s, W = self.rm, self.c, self.state, self.W
        if s["status"] == SOLVED:
            return False
        N = len(rm)
        if full(N, W, self.max_vertices):
            s["status"] = FULL
            return False
        a_is_start = s["cycle"] % 2 == 0
        roots_a, roots_b = (s["starts"], s["goals"]) if a_is_start else (s["goals"], s["starts"])
        q, ok = c.sample_project_batch(self.seed, s["next_index"], W, want_iters=False)[:2]
        flags = ok.bool() & c.joint_valid_batch(q).bool()
        if self.scene is not None:
            flags = flags & self.scene.clearance_batch(q, self.margin, want_pair=False)[2].bool()
        flags, samples = flags.cpu().numpy(), q.cpu().numpy()
        joints = rm.read(host=True)[0]
        idx_a, d_a = [x.cpu().numpy() for x in rm.nearest_in_tree(roots_a, q)]
        use_a, frm, to = self._edges(idx_a, samples, flags, joints)
        st, ns, oks = self._traverse(frm, to)
        pa = rrtc_pick_ref(st, ns, oks, samples, d=d_a, use=use_a, range=self.range, mode=0)
        made = np.isin(pa["outcome"], (ADVANCED, REACHED))
        idx_b, _ = [x.cpu().numpy() for x in rm.nearest_in_tree(roots_b, self._dev(pa["row"]))]
        use_b, frm, to = self._edges(idx_b, pa["row"], made, joints)
        st, ns, oks = self._traverse(frm, to)
        pb = rrtc_pick_ref(st, ns, oks, pa["row"], use=use_b, range=self.range, mode=1)
        self.seen |= {("extend", int(o)) for o in pa["outcome"]} | {("connect", int(o)) for o in pb["outcome"][made]}
        s, rows, uv = commit(s, N, a_is_start, use_a, pa, idx_a, pb, idx_b)
        if len(rows):
            rm.append(joints=self._dev(rows))
        if (uv[:, 0] >= 0).any():
            rm.add_edges(self._dev(uv))
        s["cycle"] += 1
        self.state = connected(rm.labels(host=True), s)
        return self.state["status"] != SOLVED

    def run(self, max_cycles):
        ran = 0
        while ran < max_cycles:
            if self.state["status"] == SOLVED:
                return ran
            before = self.state["cycle"]
            more = self.cycle()
            ran += self.state["cycle"] - before
            if not more:
                return ran
        if self.state["status"] not in (SOLVED, FULL):
            self.state["status"] = BUDGET
        return ran
