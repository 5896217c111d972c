"""Helpers shared by the tests of the roadmap graph (tests/test_graph_ref.py, tests/test_gpu_graph.py).  Host only.

  * `union_find_labels`: a numpy union-find to min-index labels;
  * `Graph` / `grow_tree_tail`: a Python restatement of what growTree does after its traversals (stefanBiPRM.cpp:303-372) plus
    milestonesToAdd (:420-445), on a union-find that is updated edge by edge, so sameComponent_start(n) sees the earlier edges of the
    same vertex exactly as the reference's disjoint sets do.  Edge weights are formed here in exact rational arithmetic, one rounding
    per FMA, then math.sqrt (correctly rounded); poses of states are the det oracle's compute_t_wo through ccmp_pose_from_t_wo;
    distances are one ccmp_pose_distance call per pair.  ONE line differs from the reference: on the GREACHED exit the reference forgets
    its added_lists (:372 returns without milestonesToAdd); the rule of include/ccmp.h adds the mid-stones whatever the state;
  * the case builders.  Joint rows come from pose_ik_cases.sampled_case; state lists are assembled by hand, [joints[n], ..., joints[c]]
    with c closer to or farther from the goal pose than n, c = n for the exact tie (no mid-stone), and a NaN last state."""
import functools
import math
from fractions import Fraction

import numpy as np

from conftest import load_cfg
from pose_ik_cases import TARGETS, sampled_case

OBJ = "Wine_Bottle"
TRAPPED, SREACHED, GREACHED, UNSETTLED = range(4)
MS = 6  # max_states of the hand-made lists
KINDS = ("reached", "failed_closer", "empty", "failed_farther", "reached", "failed_tie", "failed_one", "failed_closer", "reached", "failed_nan",
         "unsettled_ok2", "failed_zero", "reached", "failed_closer", "failed_farther", "reached", "unsettled_long", "failed_closer", "empty", "reached",
         "failed_closer", "reached", "failed_farther")
SLOT_KINDS = ("empty", "unsettled", "reached", "failed")


def union_find_labels(uv, n):
    """labels (n,) int32: the smallest index of every vertex's component under the edges uv (E,2)"""
    parent = np.arange(n, dtype=np.int64)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in np.asarray(uv, dtype=np.int64).reshape(-1, 2):
        a, b = find(u), find(v)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.int32)


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))  # the exact value, rounded once


def edge_weight(a, b):
    """RealVectorStateSpace::distance over the 14 joints in the k-NN's rounding; NaN in, NaN out"""
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return float("nan")
    acc = 0.0
    for i in range(14):
        d = float(a[i]) - float(b[i])
        acc = _fma(d, d, acc)
    return math.sqrt(acc)


@functools.lru_cache(maxsize=None)
def _det():
    from oracle_binding import Oracle

    orc = Oracle("det")
    return orc, orc.problem(load_cfg(OBJ))


def pose_of_state(q):
    """the object pose of a joint state as an append derives it"""
    from closed_chain_motion_planner_amd import pose_from_t_wo

    q = np.asarray(q, dtype=np.float64)
    if not np.isfinite(q[:7]).all():
        return np.array([np.nan] * 7 + [0.0])
    orc, OP = _det()
    R, p = orc.compute_t_wo(OP, q[:7])
    return pose_from_t_wo(np.concatenate([R.reshape(9), p]))


class Graph:
    """the planner's graph as the reference keeps it: vertex properties, an edge list, boost's disjoint sets"""

    def __init__(self, joints, poses, edges=()):
        self.joints = [np.array(j) for j in joints]
        self.poses = [np.array(p) for p in poses]
        self.parent = list(range(len(self.joints)))
        self.edges = []  # (u, v, weight)
        for u, v in edges:
            self.add_edge(int(u), int(v))

    def clone(self):
        g = Graph.__new__(Graph)
        g.joints, g.poses, g.parent, g.edges = list(self.joints), list(self.poses), list(self.parent), list(self.edges)
        return g

    def add_vertex(self, joints, pose):
        self.joints.append(np.array(joints))
        self.poses.append(np.array(pose))
        self.parent.append(len(self.parent))  # disjointSets_.make_set
        return len(self.parent) - 1

    def remove_last_vertex(self):
        self.joints.pop()
        self.poses.pop()
        self.parent.pop()

    def find(self, x):
        while self.parent[x] != x:
            x = self.parent[x]
        return x

    def same_component(self, a, b):
        return self.find(a) == self.find(b)

    def add_edge(self, n, t, weight=None):
        self.edges.append((n, t, edge_weight(self.joints[n], self.joints[t]) if weight is None else weight))  # opt_->motionCost
        a, b = self.find(n), self.find(t)  # uniteComponents
        if a != b:
            self.parent[max(a, b)] = min(a, b)

    def labels(self):
        return union_find_labels([(u, v) for u, v, _ in self.edges], len(self.parent))

    def arrays(self):
        return np.array(self.joints).reshape(-1, 14), np.array(self.poses).reshape(-1, 8)


def slot_kind(nbr, ok, n_states, max_states):
    if nbr < 0:
        return "empty"
    if ok == 2 or n_states > max_states:
        return "unsettled"
    return "reached" if ok == 1 else "failed"


def grow_tree_tail(g, nbr, ok, n_states, states, q_new, pose_new, goal, roots, vertex_ok=1, keep_isolated=False, max_states=MS):
    """growTree(obj_state_) from `if (ik_success)` on, for one new vertex on the Graph g (modified in place).  nbr (k,), ok (k,),
    n_states (k,), states (k, max_states, 14) or None.  Returns (state, t or -1, mids (k,) with -1 for none)."""
    from closed_chain_motion_planner_amd import pose_distance

    k = len(nbr)
    mids = [-1] * k
    if not vertex_ok:  # ik_success false: the vertex goes (:375-378)
        return TRAPPED, -1, mids
    if any(slot_kind(nbr[r], ok[r], n_states[r], max_states) == "unsettled" for r in range(k)):
        return UNSETTLED, -1, mids  # a traversal has not ended: nothing to decide yet
    same_component_start = lambda n: any(g.same_component(s, n) for s in roots)
    pose = np.zeros(8)
    pose[:7] = pose_new[:7]
    t = g.add_vertex(q_new, pose)
    add_edge, added_lists = False, []
    for r in range(k):
        n = int(nbr[r])
        if slot_kind(n, ok[r], n_states[r], max_states) == "empty":
            continue
        if ok[r] == 1:  # discreteGeodesic returned true
            g.add_edge(n, t)
            add_edge = True
        elif states is not None and goal is not None and n_states[r] > 1 and same_component_start(n):
            back = states[r][n_states[r] - 1]
            obj_state = pose_of_state(back)
            current = pose_distance(g.poses[n], goal)
            new_dist = pose_distance(obj_state, goal)
            if new_dist < current:
                added_lists.append((r, n, back, obj_state))

    def milestones_to_add():
        for r, n, back, obj_state in added_lists:
            mid = g.add_vertex(back, obj_state)
            g.add_edge(n, mid)
            mids[r] = mid

    if not add_edge:
        if not keep_isolated:
            g.remove_last_vertex()
            t = -1
        milestones_to_add()
        return TRAPPED, t, mids
    milestones_to_add()  # (the reference: only in front of `return SREACHED`)
    if any(g.same_component(s, t) for s in roots):
        return SREACHED, t, mids
    return GREACHED, t, mids


def python_commit(g, case):
    """The rule on a batch: every query runs grow_tree_tail on the graph AS IT WAS AT ENTRY (the queries of one call do not see each
    other) with the indices the earlier queries took already taken; g is then extended by everything.  Returns new_index, mid_index,
    grow_state and the rows and edges that were added, in order."""
    Q, k = case["nbr_idx"].shape
    entry, n0, e0 = g.clone(), len(g.parent), len(g.edges)
    new_index, mid_index, grow_state = np.full(Q, -1, np.int32), np.full((Q, k), -1, np.int32), np.zeros(Q, np.int32)
    for q in range(Q):
        h = entry.clone()
        for i in range(n0, len(g.parent)):  # the earlier queries' vertices: present, isolated
            h.add_vertex(g.joints[i], g.poses[i])
        base_v, base_e = len(h.parent), len(h.edges)
        st = None if case["states"] is None else case["states"].reshape(Q, k, -1, 14)[q]
        state, t, mids = grow_tree_tail(h, case["nbr_idx"][q], case["edge_ok"].reshape(Q, k)[q], case["n_states"].reshape(Q, k)[q], st, case["new_joints"][q],
                                        case["new_poses"][q], case["goal_pose"], case["roots"], 1 if case["vertex_ok"] is None else case["vertex_ok"][q],
                                        bool(case["flags"] & 1), case["max_states"])
        grow_state[q], new_index[q], mid_index[q] = state, t, mids
        for i in range(base_v, len(h.parent)):
            g.add_vertex(h.joints[i], h.poses[i])
        for u, v, w in h.edges[base_e:]:
            g.add_edge(u, v, w)
    sj, sp = g.arrays()
    return {"new_index": new_index, "mid_index": mid_index, "grow_state": grow_state, "rows_joints": sj[n0:], "rows_poses": sp[n0:],
            "edges_uv": np.array([(u, v) for u, v, _ in g.edges[e0:]], dtype=np.int32).reshape(-1, 2),
            "edges_w": np.array([w for _, _, w in g.edges[e0:]], dtype=np.float64)}


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_store():
    """(joints (n,14), poses (n,8) as an append derives them, the states the new vertices take (40,14), their poses (40,8), goal pose (8,))"""
    _, _, valid, _, _, _ = sampled_case(OBJ)
    joints = np.array(valid[TARGETS:])
    poses = np.array([pose_of_state(x) for x in joints])
    fresh = np.array(valid[:TARGETS])
    fresh_poses = np.array([pose_of_state(x) for x in fresh])
    goal = pose_of_state(valid[3]).copy()
    goal[0] += 0.05  # no vertex sits on it
    for a in (joints, poses, fresh, fresh_poses, goal):
        a.setflags(write=False)
    return joints, poses, fresh, fresh_poses, goal


def initial_edges(n, seed=7):
    """in shuffled order: a chain through the multiples of 3 (vertex 0's component), one through the i % 3 == 2 below 100 (vertex 5's),
    random pairs among the rest (components of every size, singletons)"""
    rng = np.random.default_rng(seed)
    a, b = np.arange(0, n, 3), np.arange(2, min(n, 100), 3)
    rest = np.arange(1, n, 3)
    pairs = rng.choice(rest, size=(len(rest) // 3, 2))
    uv = np.concatenate([np.stack([a[:-1], a[1:]], axis=1), np.stack([b[1:], b[:-1]], axis=1), pairs[pairs[:, 0] != pairs[:, 1]]])
    return np.ascontiguousarray(rng.permutation(uv).astype(np.int32))


ROOTS = (0, 5)


def make_case(store_joints, store_poses, Q, k, seed, goal, fresh, fresh_poses, kinds=None, flags=0, with_vertex_ok=True, roots=ROOTS):
    """One commit call's inputs on the store's arrays as they stand: slot kinds cycle through KINDS from a seeded offset (or are
    `kinds`, a (Q,k) list of names), neighbours are distinct random vertices."""
    from closed_chain_motion_planner_amd import pose_distance

    rng = np.random.default_rng(seed)
    N = len(store_joints)
    to_goal = np.array([pose_distance(p, goal) for p in store_poses])
    finite = np.where(np.isfinite(to_goal), to_goal, np.inf)
    nearest, farthest = int(np.argmin(finite)), int(np.argmax(np.where(np.isfinite(to_goal), to_goal, -np.inf)))
    nbr = np.full((Q, k), -1, np.int32)
    ok, ns = np.zeros((Q, k), np.uint8), np.zeros((Q, k), np.int32)
    states = np.zeros((Q, k, MS, 14))
    names = []
    offset = int(rng.integers(len(KINDS)))
    for q in range(Q):
        picks = rng.choice(N, size=k, replace=False) if N >= k else rng.integers(0, N, size=k)
        for r in range(k):
            kind = kinds[q][r] if kinds is not None else KINDS[(offset + q * k + r) % len(KINDS)]
            if kinds is None and kind.startswith("unsettled") and Q > 1 and q % 3 != 1:
                kind = "failed_closer"  # an unsettled slot holds its whole query back: two queries in three have none
            n = int(picks[r])
            names.append(kind)
            if kind == "empty":
                continue
            nbr[q, r] = n
            length = int(rng.integers(2, MS + 1))
            states[q, r, :] = store_joints[n]
            if kind == "reached":
                ok[q, r], ns[q, r] = 1, length
                states[q, r, length - 1] = fresh[q % len(fresh)]
            elif kind == "unsettled_ok2":
                ok[q, r], ns[q, r] = 2, length
            elif kind == "unsettled_long":
                ok[q, r], ns[q, r] = 0, MS + 1
            elif kind == "failed_zero":
                ns[q, r] = 0
            elif kind == "failed_one":
                ns[q, r] = 1
            else:
                ns[q, r] = length
                c = {"failed_closer": nearest, "failed_farther": farthest, "failed_tie": n, "failed_nan": n}[kind]
                states[q, r, length - 1] = store_joints[c]
                if kind == "failed_nan":
                    states[q, r, length - 1, 2] = np.nan
    which = np.arange(Q) % len(fresh)
    vertex_ok = None
    if with_vertex_ok:
        vertex_ok = np.ones(Q, np.uint8)
        vertex_ok[rng.random(Q) < 0.1] = 0
    return {"nbr_idx": nbr, "edge_ok": ok.reshape(-1), "n_states": ns.reshape(-1), "states": states.reshape(Q * k, MS, 14), "max_states": MS,
            "new_joints": np.array(fresh[which]), "new_poses": np.array(fresh_poses[which]), "vertex_ok": vertex_ok, "goal_pose": np.array(goal),
            "roots": tuple(roots), "flags": flags, "kinds": names}


def kind_counts(case):
    """{slot kind: count} over a case's slots"""
    Q, k = case["nbr_idx"].shape
    out = dict.fromkeys(SLOT_KINDS, 0)
    for e in range(Q * k):
        out[slot_kind(case["nbr_idx"].reshape(-1)[e], case["edge_ok"][e], case["n_states"][e], case["max_states"])] += 1
    return out


def commit_args(case):
    """the keyword arguments of commit_ref / Roadmap.commit"""
    return dict(nbr_idx=case["nbr_idx"], edge_ok=case["edge_ok"], n_states=case["n_states"], new_joints=case["new_joints"], new_poses=case["new_poses"],
                states=case["states"], vertex_ok=case["vertex_ok"], goal_pose=case["goal_pose"], roots=case["roots"], flags=case["flags"], max_states=case["max_states"])


BATCH_SHAPES = [(Q, k) for Q in (1, 12, 70) for k in (1, 5, 16)]


def batch_case(Q, k):
    """the batch case of shape (Q, k) on the base store with its initial edges: (graph at entry, case)"""
    joints, poses, fresh, fresh_poses, goal = base_store()
    g = Graph(joints, poses, initial_edges(len(joints)))
    return g, make_case(joints, poses, Q, k, 1000 * Q + k, goal, fresh, fresh_poses)


def bits(a):
    """the bytes of an array, every NaN as one canonical NaN"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    if a.dtype == np.float64:
        a = np.where(np.isnan(a), np.nan, a)
    return np.ascontiguousarray(a).view(np.uint8)


def same_commit(got, want):
    """two commit results (commit_ref's dict shape): integers equal, floats as bytes"""
    for name in ("new_index", "mid_index", "grow_state", "edges_uv"):
        assert np.array_equal(np.asarray(got[name]).reshape(-1), np.asarray(want[name]).reshape(-1)), (name, got[name], want[name])
    for name in ("rows_joints", "rows_poses", "edges_w"):
        assert np.asarray(got[name]).shape == np.asarray(want[name]).shape, name
        assert np.array_equal(bits(got[name]), bits(want[name])), name
