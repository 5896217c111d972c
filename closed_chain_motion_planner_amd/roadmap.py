"""Host mirror of the device-resident roadmap store (include/ccmp.h: ccmp_roadmap_*) and of the planner's tree metric.

The reference's `tree_` ranks on `obj_space_->distance(components[1], components[1])` (stefanBiPRM.h:194-201): the SE3 distance
between the object poses of two vertices.  `Roadmap` keeps the joints (14) and the object pose (x y z qx qy qz qw pad) of every
vertex on the device, so that the planner's append / query / sometimes-remove-the-last loop uploads one vertex per step, and ranks
on that metric (`_lib.METRIC_OBJECT`) or on the joint distance (`_lib.METRIC_JOINT`).

Arguments that are torch tensors are taken as device memory and the calls are asynchronous on the current (or given) stream; numpy
arrays go through the synchronous host forms and come back as numpy arrays.  All arithmetic happens in libccmp.so.
"""
import ctypes as C
import functools

import numpy as np

from . import _lib
from ._arrays import HOST, _stream_handle, _torch, kind_of, kind_on
from ._lib import COMMIT_KEEP_ISOLATED, GROW_GREACHED, GROW_SREACHED, GROW_TRAPPED, GROW_UNSETTLED, METRIC_JOINT, METRIC_OBJECT, check
from .ik import ik_options
from .object import DEFAULT_HI, DEFAULT_LO

__all__ = ["Roadmap", "pose_distance", "pose_from_t_wo", "joint_distance", "graph_labels_ref", "commit_ref", "closest_ref", "shortest_paths_ref", "METRIC_JOINT", "METRIC_OBJECT",
           "GROW_TRAPPED", "GROW_SREACHED", "GROW_GREACHED", "GROW_UNSETTLED", "COMMIT_KEEP_ISOLATED", "Plan", "PLAN_STATUS", "plan_options", "plan_check_ref",
           "plan_prefix_ref", "plan_connected_ref", "RRTConnect", "RRTC_STATUS", "rrtc_options", "rrtc_pick_ref", "rrtc_pick", "rrtc_connected_ref", "nearest_in_tree_ref",
           "rrtc_nearest_shape"]

_arg = HOST.arg


def _pose8(pose):
    """a pose (x y z qx qy qz qw [pad]) from the host or the device as the padded host row the library takes"""
    p8 = np.zeros(8)
    p8[:7] = np.asarray(pose.cpu() if hasattr(pose, "cpu") else pose, dtype=np.float64).reshape(-1)[:7]
    return p8


def pose_distance(a, b):
    """ccmp_pose_distance: OMPL's SE3StateSpace::distance (weights 1 and 1) between two poses (x y z qx qy qz qw [pad]); host only"""
    a8, b8 = np.zeros(8), np.zeros(8)
    a8[:7], b8[:7] = np.asarray(a, dtype=np.float64)[:7], np.asarray(b, dtype=np.float64)[:7]
    return float(_lib.lib().ccmp_pose_distance(_arg(a8), _arg(b8)))


def pose_from_t_wo(t_wo):
    """ccmp_pose_from_t_wo: (..., 12) [R row-major, p] as `compute_t_wo_batch` returns it -> (..., 8) poses; host only"""
    t = np.ascontiguousarray(t_wo, dtype=np.float64)
    flat = t.reshape(-1, 12)
    out = np.empty((flat.shape[0], 8))
    fn = _lib.lib().ccmp_pose_from_t_wo
    for i in range(flat.shape[0]):
        fn(_arg(flat[i]), _arg(out[i]))
    return out.reshape(t.shape[:-1] + (8,))


def joint_distance(a, b):
    """ccmp_joint_distance: the weight of an edge between two joint states (RealVectorStateSpace::distance over the 14 joints in the
    k-NN's rounding); host only"""
    return float(_lib.lib().ccmp_joint_distance(_arg(HOST.expect(a, "float64", 14, "a")), _arg(HOST.expect(b, "float64", 14, "b"))))


def graph_labels_ref(uv, n):
    """ccmp_graph_labels_ref: labels (n,) int32, label[v] = the smallest index of v's component under the edges uv (E,2); host only"""
    uv = HOST.expect(uv, "int32", -1, "uv").reshape(-1, 2)
    labels = np.empty(int(n), dtype=np.int32)
    check(_lib.lib().ccmp_graph_labels_ref(_arg(uv), len(uv), int(n), _arg(labels)), "ccmp_graph_labels_ref")
    return labels


_NO_LIMIT = 2**31 - 1  # max_states of a commit without state lists and without a stated limit: no slot is unsettled by its length


def _commit_inputs(K, nbr_idx, edge_ok, n_states, new_joints, new_poses, states, vertex_ok, goal_pose, roots, max_states):
    """the inputs of `Roadmap.commit` / `commit_ref` as kind K takes them (goal and roots: host arrays in both), then max_states, Q and k.
    The host kind reshapes what it is given; the device kind takes new_joints (n,14) / new_poses (n,8) as they are."""
    nbr = K.expect(nbr_idx, "int32", (None, None), "nbr_idx (Q, k)")
    Q, k = nbr.shape
    S = Q * k
    st, ms = None, _NO_LIMIT if max_states is None else int(max_states)
    if states is not None and S:
        ms = int(np.prod(np.shape(states))) // (S * 14)  # the traversal's list length
        st = K.expect(states, "float64", S * ms * 14, "states (Q * k, max_states, 14)")
    rows = (lambda c: Q * c) if K is HOST else (lambda c: (None, c))
    return (nbr, K.expect(edge_ok, "uint8", S, "edge_ok"), K.expect(n_states, "int32", S, "n_states"), st, K.expect(new_joints, "float64", rows(14), "new_joints"),
            K.expect(new_poses, "float64", rows(8), "new_poses"), None if vertex_ok is None else K.expect(vertex_ok, "uint8", Q, "vertex_ok"),
            None if goal_pose is None else _pose8(goal_pose), HOST.expect(list(roots), "int32", -1, "roots"), ms, Q, k)


def commit_ref(problem, store_joints, store_poses, labels, nbr_idx, edge_ok, n_states, new_joints, new_poses, states=None, vertex_ok=None, goal_pose=None,
               roots=(), flags=0, max_states=None):
    """ccmp_roadmap_commit_ref: `Roadmap.commit`'s rule (csrc/ccmp_graph.h compiled for the host: the kernels' bits) on the store's raw
    arrays — joints (N,14), poses (N,8), labels (N,) — without a device.  Returns new_index (Q,), mid_index (Q,k), grow_state (Q,) and
    the appended rows and edges in index order: rows_joints (V,14), rows_poses (V,8), edges_uv (E,2), edges_w (E,).  `problem`: a
    `CcmpProblem` (needed for mid-stones only).  max_states: the traversal's list length (n_states beyond it = unsettled); taken from
    `states` when those are given."""
    sj, sp = HOST.expect(store_joints, "float64", -1, "store_joints").reshape(-1, 14), HOST.expect(store_poses, "float64", -1, "store_poses").reshape(-1, 8)
    lab = HOST.expect(labels, "int32", -1, "labels")
    nbr, ok, ns, st, nj, npo, vok, goal, rt, ms, Q, k = _commit_inputs(HOST, nbr_idx, edge_ok, n_states, new_joints, new_poses, states, vertex_ok, goal_pose, roots,
                                                                       max_states)
    S = Q * k
    out = {"new_index": np.empty(Q, dtype=np.int32), "mid_index": np.empty((Q, k), dtype=np.int32), "grow_state": np.empty(Q, dtype=np.int32)}
    rj, rp, euv, ew = np.empty((Q + S, 14)), np.empty((Q + S, 8)), np.empty((S, 2), dtype=np.int32), np.empty(S)
    nv, ne = C.c_size_t(), C.c_size_t()
    check(_lib.lib().ccmp_roadmap_commit_ref(C.byref(problem) if problem is not None else None, _arg(sj), _arg(sp), _arg(lab), len(sj), _arg(nbr), _arg(ok),
                                             _arg(ns), _arg(st), ms, _arg(nj), _arg(npo), _arg(vok), Q, k, _arg(goal), _arg(rt), len(rt), int(flags),
                                             _arg(out["new_index"]), _arg(out["mid_index"]), _arg(out["grow_state"]), _arg(rj), _arg(rp), _arg(euv), _arg(ew),
                                             C.byref(nv), C.byref(ne)), "ccmp_roadmap_commit_ref")
    out.update(rows_joints=rj[:nv.value].copy(), rows_poses=rp[:nv.value].copy(), edges_uv=euv[:ne.value].copy(), edges_w=ew[:ne.value].copy())
    return out


def closest_ref(store_poses, labels, froms, target_pose):
    """ccmp_roadmap_closest_ref: `Roadmap.closest` on host arrays, no device: (idx (F,), dist (F,), from_dist (F,))"""
    sp = HOST.expect(store_poses, "float64", -1, "store_poses").reshape(-1, 8)
    lab, fr = HOST.expect(labels, "int32", -1, "labels"), HOST.expect(froms, "int32", -1, "froms")
    idx, dist, fd = np.empty(len(fr), dtype=np.int32), np.empty(len(fr)), np.empty(len(fr))
    check(_lib.lib().ccmp_roadmap_closest_ref(_arg(sp), _arg(lab), len(sp), _arg(fr), len(fr), _arg(_pose8(target_pose)), _arg(idx), _arg(dist), _arg(fd)),
          "ccmp_roadmap_closest_ref")
    return idx, dist, fd


def shortest_paths_ref(uv, w, n, src, dst, max_len=None, full=False):
    """ccmp_graph_shortest_paths_ref: `Roadmap.shortest_paths`' rule (csrc/ccmp_path.h) on host arrays without a device — edges uv (E,2),
    weights w (E,) over n vertices, pairs src (F,), dst (F,), F <= 64.  Distances by heap Dijkstra, hops and predecessors from the rule
    text the kernels compile.  Returns (cost (F,), path_len (F,), paths: a list of F int32 arrays; a path longer than max_len, when
    one is given, is None); full=True adds dist (F,n) and pred (F,n)."""
    uv, w = HOST.expect(uv, "int32", -1, "uv").reshape(-1, 2), HOST.expect(w, "float64", -1, "w")
    sr, ds = HOST.expect(src, "int32", -1, "src"), HOST.expect(dst, "int32", -1, "dst")
    F, n = len(sr), int(n)
    L = int(max_len) if max_len is not None else max(n, 1)
    cost, plen, path = np.empty(F), np.empty(F, dtype=np.int32), np.full((F, L), -1, dtype=np.int32)
    dist = np.empty((F, n)) if full else None
    pred = np.empty((F, n), dtype=np.int32) if full else None
    check(_lib.lib().ccmp_graph_shortest_paths_ref(_arg(uv), _arg(w), len(uv), n, _arg(sr), _arg(ds), F, L, _arg(cost), _arg(plen), _arg(path), _arg(dist),
                                                   _arg(pred)), "ccmp_graph_shortest_paths_ref")
    paths = [path[f, :plen[f]].copy() if plen[f] <= L else None for f in range(F)]
    return (cost, plen, paths, dist, pred) if full else (cost, plen, paths)


def _edge_outputs(K, E, ms):
    """what the traversals of E edges leave, as `connect` and `grow` end their argument lists"""
    return {"states": K.empty((E, ms, 14), "float64"), "n_states": K.empty((E,), "int32"), "ok": K.empty((E,), "uint8"), "newton_iters": K.empty((E,), "int32"),
            "blocked": K.empty((E,), "uint8"), "carry": K.empty((E, 2), "float64")}


# ---- what the two planners on the store share: options, the state block as a dict, the handle's wrapper ------------------------------------
def _options(struct, defaults, what, kw):
    """`struct` with the library's defaults, fields overridden by keyword (a float sequence into an array field); `reserved` is no field"""
    o = struct()
    defaults(C.byref(o))
    for name, v in kw.items():
        if name not in dict(struct._fields_) or name == "reserved":
            raise TypeError("%s has no field %r" % (what, name))
        if isinstance(getattr(o, name), C.Array):
            getattr(o, name)[:] = [float(x) for x in v]
        else:
            setattr(o, name, v)
    return o


def _state_dict(s, scalars, counters):
    """a state block as a dict of plain values: its scalars, starts / goals cut to their lengths, nearest_pose where it has one, counters"""
    d = {n: getattr(s, n) for n in scalars}
    d.update(starts=list(s.starts[:s.n_starts]), goals=list(s.goals[:s.n_goals]))
    if hasattr(s, "nearest_pose"):
        d["nearest_pose"] = list(s.nearest_pose)
    d["counters"] = {n: getattr(s.counters, n) for n in counters}
    return d


def _state_struct(struct, d, scalars, counters):
    s = struct()
    for n in scalars:
        setattr(s, n, d[n])
    s.n_starts, s.n_goals = len(d["starts"]), len(d["goals"])
    s.starts[:], s.goals[:] = [-1] * 8, [-1] * 8  # beyond the lengths: read by nothing
    s.starts[:s.n_starts], s.goals[:s.n_goals] = [int(v) for v in d["starts"]], [int(v) for v in d["goals"]]
    if "nearest_pose" in d:
        s.nearest_pose[:] = [float(v) for v in d["nearest_pose"]]
    for n in counters:
        setattr(s.counters, n, int(d["counters"].get(n, 0)))
    return s


def _connected_ref(name, labels, state, to_struct, to_dict):
    lab = HOST.expect(labels, "int32", -1, "labels")
    s = to_struct(state)
    check(getattr(_lib.lib(), name)(_arg(lab), len(lab), C.byref(s)), name)
    return to_dict(s)


class _PlannerHandle:
    """what `Plan` and `RRTConnect` share: a handle opened by the `Roadmap`, `run`, `state`, `close`.  A subclass names its C entries'
    prefix (_ABI), its report and state structs, its status table and SOLVED value, its state helpers and its counters, and adds its own
    report fields in `_report_more`."""

    def __init__(self, roadmap, scene, handle):
        self.roadmap, self.scene, self._h = roadmap, scene, handle  # the store and the scene outlive the handle
        self.report = None
        self.run(0)

    def _call(self, verb, *args):
        name = "%s_%s" % (self._ABI, verb)
        check(getattr(_lib.lib(), name)(self._h, *args), name)

    def run(self, max_cycles):
        r = self._REPORT()
        self._call("run", int(max_cycles), C.byref(r))
        self.report = {"status": r.status, "status_name": self._STATUS.get(r.status, "?"), "cycles_run": r.cycles_run, "cycles_total": r.cycles_total,
                       "size": int(r.size), "edges": int(r.edges), "solved": (r.solved_start, r.solved_goal) if r.status == self._SOLVED else None}
        self.report.update(self._report_more(r), counters={n: getattr(r.counters, n) for n in self._COUNTERS})
        return self.report

    def state(self):
        s = self._STATE()
        self._call("state_read", C.byref(s))
        return self._state_dict(s)

    def close(self):
        if self._h:
            getattr(_lib.lib(), self._ABI + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- the planner's loop on the store (include/ccmp.h: ccmp_plan_*; the rule: csrc/ccmp_plan.h) -------------------------------------------
PLAN_STATUS = {_lib.PLAN_OPEN: "OPEN", _lib.PLAN_SOLVED: "SOLVED", _lib.PLAN_BUDGET: "BUDGET", _lib.PLAN_FULL: "FULL", _lib.PLAN_INVALID_GOAL: "INVALID_GOAL"}
_PLAN_COUNTERS = [n for n, _ in _lib.CcmpPlanCounters._fields_ if n != "reserved"]
_PLAN_SCALARS = ("nearest", "sprevious", "status", "cycle", "solved_start", "solved_goal", "size_at_check", "next_index", "prev_from_goal", "prev_from_start")


def plan_options(**kw):
    """ccmp_plan_opts with the library's defaults (width 32, k 5, attempts 2, max_states 64, t 0.3, sigma 0.2, inflate 0, lo / hi
    -1e30 / 1e30, max_vertices 2^31 - 1), fields overridden by keyword"""
    return _options(_lib.CcmpPlanOpts, _lib.lib().ccmp_plan_default_opts, "ccmp_plan_opts", kw)


_plan_state_dict = functools.partial(_state_dict, scalars=_PLAN_SCALARS, counters=_PLAN_COUNTERS)
_plan_state_struct = functools.partial(_state_struct, _lib.CcmpPlanState, scalars=_PLAN_SCALARS, counters=_PLAN_COUNTERS)


def _closest3(a, n):
    if a is None:
        return (None, None, None) if n == 0 else (np.full(n, -1, dtype=np.int32), np.full(n, np.inf), np.full(n, np.nan))
    return HOST.expect(a[0], "int32", n, "idx"), HOST.expect(a[1], "float64", n, "dist"), HOST.expect(a[2], "float64", n, "from_dist")


def plan_check_ref(state, size, a, b, store_poses=None):
    """ccmp_plan_check_ref: the check of the planner's loop (the gate, the carry rule of both sides, the thresholds, the state update) on
    a state dict as `Plan.state` returns it — a = `closest`'s (idx, dist, from_dist) for starts towards goals[0], b = the same for goals
    towards starts[0]; store_poses (size, 8): nearest_pose follows.  Returns (the new state, triggers [ran, goal side fired, start side
    fired, the goal side's vertex or -1]); host only."""
    s = _plan_state_struct(state)
    ai, ad, af = _closest3(a, s.n_starts)
    bi, bd, bf = _closest3(b, s.n_goals)
    sp = None if store_poses is None else HOST.expect(store_poses, "float64", int(size) * 8, "store_poses")
    trig = np.zeros(4, dtype=np.int32)
    check(_lib.lib().ccmp_plan_check_ref(C.byref(s), int(size), _arg(ai), _arg(ad), _arg(af), _arg(bi), _arg(bd), _arg(bf), _arg(sp), _arg(trig)), "ccmp_plan_check_ref")
    return _plan_state_dict(s), [int(t) for t in trig]


def plan_prefix_ref(valid, ik_ok):
    """ccmp_plan_prefix_ref: the ladder's prefix — (vertex_ok (9,) uint8, its length) from valid (9,) and ik_ok (9,); host only"""
    v, k = HOST.expect(valid, "uint8", 9, "valid"), HOST.expect(ik_ok, "uint8", 9, "ik_ok")
    out, n = np.zeros(9, dtype=np.uint8), C.c_int32()
    check(_lib.lib().ccmp_plan_prefix_ref(_arg(v), _arg(k), _arg(out), C.byref(n)), "ccmp_plan_prefix_ref")
    return out, int(n.value)


def plan_connected_ref(labels, state):
    """ccmp_plan_connected_ref: the solution test — the first pair (s, g), start-major, whose labels agree makes the state SOLVED with
    that pair.  Returns the new state; host only."""
    return _connected_ref("ccmp_plan_connected_ref", labels, state, _plan_state_struct, _plan_state_dict)


class Plan(_PlannerHandle):
    """ccmp_plan: the planner's loop on a `Roadmap` (`Roadmap.plan` opens one).  `run(max_cycles)` runs cycles until the status is SOLVED,
    FULL or the cycles are spent (BUDGET: run again to resume) and returns the report, also kept as `.report`: a dict with status (a
    PLAN_STATUS key; `status_name` its text), cycles_run, cycles_total, size, edges, solved (start vertex, goal vertex) or None, nearest,
    prev_from_goal, prev_from_start and counters.  The path of a SOLVED plan is `Roadmap.shortest_paths([s], [g])` on that pair.
    `state()`: the state block (ccmp_plan_state) as a dict: starts, goals, nearest, nearest_pose, sprevious, prev_from_goal,
    prev_from_start, size_at_check, next_index, cycle, status, solved_start, solved_goal, counters."""
    _ABI, _REPORT, _STATE, _STATUS, _SOLVED, _COUNTERS = "ccmp_plan", _lib.CcmpPlanReport, _lib.CcmpPlanState, PLAN_STATUS, _lib.PLAN_SOLVED, _PLAN_COUNTERS
    _state_dict = staticmethod(_plan_state_dict)

    def __init__(self, roadmap, checker, scene, handle):
        self.checker = checker  # the object outlives the handle too
        super().__init__(roadmap, scene, handle)

    @staticmethod
    def _report_more(r):
        return {"nearest": r.nearest, "prev_from_goal": r.prev_from_goal, "prev_from_start": r.prev_from_start}


# ---- RRT-Connect on the store (include/ccmp.h: ccmp_rrtc_*; the rule: csrc/ccmp_rrtc.h) --------------------------------------------------
RRTC_STATUS = {_lib.RRTC_OPEN: "OPEN", _lib.RRTC_SOLVED: "SOLVED", _lib.RRTC_BUDGET: "BUDGET", _lib.RRTC_FULL: "FULL"}
_RRTC_COUNTERS = [n for n, _ in _lib.CcmpRrtcCounters._fields_ if n != "reserved"]
_RRTC_SCALARS = ("status", "cycle", "next_index", "solved_start", "solved_goal", "best_a", "best_b", "best_gap")


def rrtc_options(**kw):
    """ccmp_rrtc_opts with the library's defaults (width 32, max_states 64, round_budget 0, range 0.1, max_vertices 2^31 - 1), fields
    overridden by keyword"""
    return _options(_lib.CcmpRrtcOpts, _lib.lib().ccmp_rrtc_default_opts, "ccmp_rrtc_opts", kw)


_rrtc_state_dict = functools.partial(_state_dict, scalars=_RRTC_SCALARS, counters=_RRTC_COUNTERS)
_rrtc_state_struct = functools.partial(_state_struct, _lib.CcmpRrtcState, scalars=_RRTC_SCALARS, counters=_RRTC_COUNTERS)


def rrtc_pick_ref(states, n_states, ok, to, d=None, use=None, range=0.1, mode=0):
    """ccmp_rrtc_pick_ref: the pick of a cycle's step 2 (mode 0: TRAPPED / ADVANCED / REACHED / UNSETTLED from the list, the nearest
    distance d and the range) or step 3 (mode 1: NOTHING / ADDED / JOINED) on host arrays — states (E,max_states,14), n_states (E,), ok
    (E,), to (E,14) the sample rows (mode 1: the vertices v), use (E,) uint8 or None (0: outcome NONE, 2: no nearest vertex).  Returns a
    dict: outcome (E,) int32, row_index (E,) int32 (the listed state that becomes the vertex; -1: the target row or none), row (E,14)
    (zeros without a vertex), gap (E,) (mode 1: the distance of the last stored state to v; NaN without one).  Host only."""
    st = np.ascontiguousarray(states, dtype=np.float64)
    E, ms = st.shape[0], st.shape[1]
    ns, k = HOST.expect(n_states, "int32", E, "n_states"), HOST.expect(ok, "uint8", E, "ok")
    t = HOST.expect(to, "float64", E * 14, "to")
    dd = None if d is None else HOST.expect(d, "float64", E, "d")
    u = None if use is None else HOST.expect(use, "uint8", E, "use")
    out = {"outcome": np.empty(E, dtype=np.int32), "row_index": np.empty(E, dtype=np.int32), "row": np.empty((E, 14)), "gap": np.empty(E)}
    check(_lib.lib().ccmp_rrtc_pick_ref(int(mode), _arg(st.reshape(-1)), _arg(ns), _arg(k), _arg(u), _arg(t), _arg(dd), E, int(ms), float(range),
                                        _arg(out["outcome"]), _arg(out["row_index"]), _arg(out["row"]), _arg(out["gap"])), "ccmp_rrtc_pick_ref")
    return out


def rrtc_pick(ctx, states, n_states, ok, to, d=None, use=None, range=0.1, mode=0, stream=None):
    """ccmp_rrtc_pick_batch: `rrtc_pick_ref` on device tensors (the pick kernel of a cycle on its own) on the `Context` ctx; the same dict,
    as device tensors; asynchronous on the stream"""
    K = kind_of(states)
    st = K.expect(states, "float64", (None, None, 14), "states")
    E, ms = st.shape[0], st.shape[1]
    ns, k, t = K.expect(n_states, "int32", (E,), "n_states"), K.expect(ok, "uint8", (E,), "ok"), K.expect(to, "float64", (E, 14), "to")
    dd = None if d is None else K.expect(d, "float64", (E,), "d")
    u = None if use is None else K.expect(use, "uint8", (E,), "use")
    out = {"outcome": K.empty(E, "int32"), "row_index": K.empty(E, "int32"), "row": K.empty((E, 14), "float64"), "gap": K.empty(E, "float64")}
    check(_lib.lib().ccmp_rrtc_pick_batch(ctx.handle, int(mode), K.arg(st), K.arg(ns), K.arg(k), K.arg(u), K.arg(t), K.arg(dd), E, int(ms), float(range),
                                          *[K.arg(a) for a in out.values()], _stream_handle(stream)), "ccmp_rrtc_pick_batch")
    return out


def rrtc_connected_ref(labels, state):
    """ccmp_rrtc_connected_ref: the solution test on a state dict as `RRTConnect.state` returns it; returns the new state; host only"""
    return _connected_ref("ccmp_rrtc_connected_ref", labels, state, _rrtc_state_struct, _rrtc_state_dict)


def nearest_in_tree_ref(store_joints, labels, roots, queries):
    """ccmp_roadmap_nearest_in_tree_ref: `Roadmap.nearest_in_tree` on host arrays, no device: (idx (Q,), dist (Q,))"""
    sj, lab = HOST.expect(store_joints, "float64", -1, "store_joints").reshape(-1, 14), HOST.expect(labels, "int32", -1, "labels")
    rt, q = HOST.expect(list(roots), "int32", -1, "roots"), HOST.expect(queries, "float64", -1, "queries").reshape(-1, 14)
    idx, dist = np.empty(len(q), dtype=np.int32), np.empty(len(q))
    check(_lib.lib().ccmp_roadmap_nearest_in_tree_ref(_arg(sj, True), _arg(lab, True), len(sj), _arg(rt, True), len(rt), _arg(q, True), len(q), _arg(idx, True),
                                                      _arg(dist, True)), "ccmp_roadmap_nearest_in_tree_ref")
    return idx, dist


def rrtc_nearest_shape(ctx_handle, Q, N):
    """ccmp_rrtc_nearest_shape: (rows per partition, partitions) of a nearest-in-tree call of Q queries on N rows; ctx_handle None: a
    256-CU device.  No result depends on it."""
    part, parts = C.c_uint(), C.c_uint()
    check(_lib.lib().ccmp_rrtc_nearest_shape(ctx_handle, int(Q), int(N), C.byref(part), C.byref(parts)), "ccmp_rrtc_nearest_shape")
    return int(part.value), int(parts.value)


class RRTConnect(_PlannerHandle):
    """ccmp_rrtc: RRT-Connect on a `Roadmap` (`Roadmap.rrt_connect` opens one).  `run(max_cycles)` runs cycles until the status is SOLVED,
    FULL or the cycles are spent (BUDGET: run again to resume) and returns the report, also kept as `.report`: a dict with status (an
    RRTC_STATUS key; `status_name` its text), cycles_run, cycles_total, size, edges, solved (start vertex, goal vertex) or None, best_gap
    and best (its pair, start side first) and counters.  `state()`: the state block (ccmp_rrtc_state) as a dict: starts, goals, status,
    cycle, next_index, solved_start, solved_goal, best_gap, best_a, best_b, counters."""
    _ABI, _REPORT, _STATE, _STATUS, _SOLVED, _COUNTERS = "ccmp_rrtc", _lib.CcmpRrtcReport, _lib.CcmpRrtcState, RRTC_STATUS, _lib.RRTC_SOLVED, _RRTC_COUNTERS
    _state_dict = staticmethod(_rrtc_state_dict)

    @staticmethod
    def _report_more(r):
        return {"best_gap": r.best_gap, "best": (r.best_a, r.best_b)}

    def solution(self, max_len=64, host=False):
        """`Roadmap.shortest_paths` on the solved pair (its dict, one pair), or None while the status is not SOLVED"""
        if self.report is None or self.report["solved"] is None:
            return None
        s, g = self.report["solved"]
        return self.roadmap.shortest_paths(np.array([s], dtype=np.int32), np.array([g], dtype=np.int32), max_len=max_len, host=host)


class Roadmap:
    """ccmp_roadmap on `constraint`'s context.  Indices are positions; only the tail can be removed (`truncate`)."""

    def __init__(self, constraint, capacity_hint=0):
        self.constraint = constraint
        self.ctx = constraint.ctx
        self._h = C.c_void_p(_lib.lib().ccmp_roadmap_create(self.ctx.handle, int(capacity_hint)))
        if not self._h:
            raise _lib.CcmpError(-2, "ccmp_roadmap_create", _lib.lib().ccmp_last_hip_error().decode())

    def _problem(self):
        self.constraint._need_problem()
        return C.byref(self.constraint.problem)

    def __len__(self):
        return int(_lib.lib().ccmp_roadmap_size(self._h))

    def reserve(self, n):
        """room for n vertices in all: appends up to there are asynchronous and never move the rows"""
        check(_lib.lib().ccmp_roadmap_reserve(self._h, int(n)), "ccmp_roadmap_reserve")

    def append(self, joints=None, poses=None, stream=None):
        """New vertices at indices len(self) ...; returns the first.  poses None: derived on the device from the joints; joints
        None: pose-only vertices (NaN joint rows, never a joint-metric neighbour) until `set_joints`."""
        first = C.c_size_t()
        given = joints if joints is not None else poses
        if given is None:
            raise ValueError("joints, poses or both")
        K = kind_of(given)
        j = K.expect(joints, "float64", (None, 14), "joints") if joints is not None else None
        p = K.expect(poses, "float64", (None, 8), "poses") if poses is not None else None
        K.call("ccmp_roadmap_append", "ccmp_roadmap_append_host", self._h, self._problem() if p is None else None, K.arg(j), K.arg(p), len(given),
               C.byref(first), stream=stream)
        return int(first.value)

    def set_joints(self, index, joints, stream=None):
        """the joints of vertex `index` (growTree: after the IK of a pose-only vertex); its pose row stays"""
        K = kind_of(joints)
        j = K.expect(joints.reshape(1, 14), "float64", (1, 14), "joints")
        K.call("ccmp_roadmap_set_joints", "ccmp_roadmap_set_joints_host", self._h, int(index), K.arg(j), stream=stream)

    def truncate(self, n):
        """drops the vertices from index n on (the reference's remove_vertex of the vertex just appended)"""
        check(_lib.lib().ccmp_roadmap_truncate(self._h, int(n)), "ccmp_roadmap_truncate")

    def read(self, first=0, count=None, host=False, stream=None):
        """(joints (count,14), poses (count,8)) of the vertices first ... — device tensors, or numpy arrays with host=True"""
        count = len(self) - int(first) if count is None else int(count)
        K = kind_on(self.ctx, host)
        j, p = K.empty((count, 14), "float64"), K.empty((count, 8), "float64")
        K.call("ccmp_roadmap_read", "ccmp_roadmap_read_host", self._h, int(first), count, K.arg(j), K.arg(p), stream=stream)
        return j, p

    def nearest_k(self, queries, k, metric=METRIC_OBJECT, mode=0, self_base=0, stream=None):
        """The k nearest vertices of every query: (Q,8) poses under METRIC_OBJECT, (Q,14) joints under METRIC_JOINT; modes, ranking
        and empty slots as `KinematicChainConstraint.nearest_k_batch`.  Returns (nbr_idx (Q,k) int32, nbr_dist (Q,k) float64)."""
        cols, k = (14 if metric == METRIC_JOINT else 8), int(k)
        K = kind_of(queries)
        q = K.expect(queries, "float64", (None, cols), "queries")
        idx, dist = K.empty((len(q), k), "int32"), K.empty((len(q), k), "float64")
        K.call("ccmp_roadmap_knn", "ccmp_roadmap_knn_host", self._h, int(metric), K.arg(q), len(q), k, int(mode), int(self_base), K.arg(idx), K.arg(dist),
               stream=stream)
        return idx, dist

    def connect(self, query_joints, k, metric=METRIC_OBJECT, query_poses=None, mode=0, self_base=0, check_target=True, max_states=64,
                round_budget=0, scene=None, margin=None, stream=None):
        """Neighbours from the store by `metric`, then edge e = q * k + r from the store's joints at nbr_idx[q, r] to
        query_joints[q], exactly as `KinematicChainConstraint.connect_batch` runs its edges; the same dict comes back.
        METRIC_OBJECT ranks on `query_poses`, or on the poses derived from `query_joints` when they are None."""
        Q, k, ms = len(query_joints), int(k), int(max_states)
        K = kind_of(query_joints)
        qj = K.expect(query_joints, "float64", (None, 14), "query_joints")
        qp = K.expect(query_poses, "float64", (None, 8), "query_poses") if query_poses is not None else None
        out = {"nbr_idx": K.empty((Q, k), "int32"), "nbr_dist": K.empty((Q, k), "float64"), **_edge_outputs(K, Q * k, ms)}  # in the order the library takes them
        K.call("ccmp_roadmap_connect", "ccmp_roadmap_connect_host", self._h, self._problem(), scene._h if scene is not None else None,
               float(margin) if scene is not None else 0.0, int(metric), K.arg(qj), K.arg(qp), Q, k, int(mode), int(self_base), 1 if check_target else 0, ms,
               int(round_budget), *[K.arg(a) for a in out.values()], stream=stream)
        return out

    def grow(self, query_poses, k, mode=0, self_base=0, rng_seed=0, first_index=0, opts=None, check_target=False, max_states=64, round_budget=0,
             scene=None, margin=None, stream=None, vet=False):
        """growTree's device part for the poses `query_poses` (Q,8) in one call (ccmp_roadmap_grow): the object-metric k-NN on the store,
        the neighbours' joints as seed slots in rank order, `KinematicChainConstraint.pose_ik_batch` on them, then edge e = q * k + r
        from neighbour r to the new state as `connect` runs its edges (check_target False: growTree's discreteGeodesic).  Returns
        `connect`'s dict plus q_new (Q,14), ik_ok (Q,), ik_which (Q,).  A pose without a state (and a neighbour without joints) has
        empty slots.  Nothing is appended: the reference adds the vertex only after an edge succeeded.
        vet=True with a scene: ccmp_roadmap_grow_vetted — the IK vets its candidates and the assembled state against the scene under the
        same margin as the traversals (IKValid inside sampleCalibGoal, on proxies), and the dict also holds ik_clearance (Q,)."""
        Q, k, ms = len(query_poses), int(k), int(max_states)
        opts = opts if opts is not None else ik_options()
        vet = bool(vet) and scene is not None
        K = kind_of(query_poses)
        qp = K.expect(query_poses, "float64", (None, 8), "query_poses")
        out = {"nbr_idx": K.empty((Q, k), "int32"), "nbr_dist": K.empty((Q, k), "float64"), "q_new": K.empty((Q, 14), "float64"), "ik_ok": K.empty((Q,), "uint8"),
               "ik_which": K.empty((Q,), "int32"), **({"ik_clearance": K.empty((Q,), "float64")} if vet else {}),
               **_edge_outputs(K, Q * k, ms)}  # in the order the library takes them
        entries = ("ccmp_roadmap_grow_vetted", "ccmp_roadmap_grow_vetted_host") if vet else ("ccmp_roadmap_grow", "ccmp_roadmap_grow_host")
        K.call(*entries, self._h, self._problem(), scene._h if scene is not None else None, float(margin) if scene is not None else 0.0, C.byref(opts),
               K.arg(qp), Q, k, int(mode), int(self_base), int(rng_seed), int(first_index), 1 if check_target else 0, ms, int(round_budget),
               *[K.arg(a) for a in out.values()], stream=stream)
        return out

    def grow_toward(self, checker, from_poses, goal_pose, k, t=0.3, sigma=0.2, lo=None, hi=None, attempts=2, rng_seed=0, first_index=0, inflate=0.0,
                    **grow_args):
        """The whole of growTree's device part (stefanBiPRM.cpp:255-351): `checker.propose` (an `ObjectChecker`: interpolate from_poses[g]
        towards goal_pose, draw, test the mesh, `attempts` times), then `grow` on the poses that were found.  Indices without a valid
        candidate (which = -1: the reference's TRAPPED) never reach `grow`.  The flags make one small host read in between — growTree
        needs that decision on the host anyway.  Returns `grow`'s dict over the kept poses plus "which" (G,), "rows" (the grow index g of
        every row of the other entries) and "poses" (the kept poses); rng_seed and first_index serve both the draw and the IK restarts
        (row r of `grow` uses first_index + r); grow_args go to `grow`."""
        prop = checker.propose(from_poses, goal_pose, t=t, sigma=sigma, lo=DEFAULT_LO if lo is None else lo, hi=DEFAULT_HI if hi is None else hi,
                               attempts=attempts, rng_seed=rng_seed, first_index=first_index, inflate=inflate)
        which = prop["which"]
        if isinstance(which, np.ndarray):
            rows = np.flatnonzero(which >= 0)
            kept = np.ascontiguousarray(prop["pose"][rows])
        else:
            rows_t = (which >= 0).nonzero().reshape(-1)  # the host read: the flags decide what grows
            kept = prop["pose"][rows_t].contiguous()
            rows = rows_t.cpu().numpy()
        out = self.grow(kept, k, rng_seed=rng_seed, first_index=first_index, **grow_args)
        out.update(which=which, rows=rows, poses=kept)
        return out

    # ---- the graph: edges, component labels, growTree's tail, closestFromGoal (include/ccmp.h; csrc/ccmp_graph.h) ---------------------
    def commit(self, nbr_idx, edge_ok, n_states, new_joints, new_poses, states=None, vertex_ok=None, goal_pose=None, roots=(), flags=0, max_states=None,
               stream=None):
        """What follows the traversals in growTree (stefanBiPRM.cpp:303-372, milestonesToAdd), addMilestone and, with
        COMMIT_KEEP_ISOLATED, startgoalMilestone, on the device (ccmp_roadmap_commit): `grow`'s / `connect`'s nbr_idx (Q,k), ok, n_states
        and states go in unchanged with the new states' joints (Q,14) and poses (Q,8).  Per query: the new vertex stays if an edge
        reached it (or with COMMIT_KEEP_ISOLATED), every reached slot gives an edge weighted by the joint distance, and — with
        `goal_pose` and `states` — a failed slot whose neighbour is in a root's component (`roots`: the planner's start vertices) and
        whose last state is strictly closer to the goal than the neighbour gives a mid-stone vertex and its edge.  The labels are
        updated.  Returns new_index (Q,) (-1: not kept), mid_index (Q,k) (-1: none), grow_state (Q,) (GROW_*), and the counts
        vertices_added / edges_added (ints).  The queries of one call do not see each other.  Synchronous at its end (one small
        read-back), not capturable.  max_states: the traversal's list length (n_states beyond it = unsettled); taken from `states` when
        those are given."""
        nv, ne = C.c_size_t(), C.c_size_t()
        K = kind_of(nbr_idx)
        nbr, ok, ns, st, nj, npo, vok, goal, rt, ms, Q, k = _commit_inputs(K, nbr_idx, edge_ok, n_states, new_joints, new_poses, states, vertex_ok, goal_pose, roots,
                                                                           max_states)
        out = {"new_index": K.empty(Q, "int32"), "mid_index": K.empty((Q, k), "int32"), "grow_state": K.empty(Q, "int32")}
        K.call("ccmp_roadmap_commit", "ccmp_roadmap_commit_host", self._h, self._problem() if (st is not None and goal is not None) else None, K.arg(nbr), K.arg(ok),
               K.arg(ns), K.arg(st), ms, K.arg(nj), K.arg(npo), K.arg(vok), Q, k, _arg(goal), _arg(rt), len(rt), int(flags), *[K.arg(a) for a in out.values()],
               C.byref(nv), C.byref(ne), stream=stream)
        out.update(vertices_added=int(nv.value), edges_added=int(ne.value))
        return out

    def add_edges(self, uv, stream=None):
        """Explicit edges uv (E,2) int32 between existing vertices; the weights (joint distance) are computed on the device and the labels
        updated.  numpy: an endpoint out of range or u == v raises (CCMP_EINVAL), returns 0; a device tensor: such edges are skipped and
        their number is returned."""
        if isinstance(uv, np.ndarray):
            a = HOST.expect(uv, "int32", -1, "uv").reshape(-1, 2)
            check(_lib.lib().ccmp_roadmap_add_edges_host(self._h, _arg(a), len(a)), "ccmp_roadmap_add_edges_host")
            return 0
        uv = kind_of(uv).expect(uv, "int32", (None, 2), "uv")
        rej = C.c_size_t()
        check(_lib.lib().ccmp_roadmap_add_edges(self._h, uv.data_ptr(), uv.shape[0], C.byref(rej), _stream_handle(stream)), "ccmp_roadmap_add_edges")
        return int(rej.value)

    @property
    def num_edges(self):
        return int(_lib.lib().ccmp_roadmap_num_edges(self._h))

    def edges(self, first=0, count=None, host=False, stream=None):
        """(uv (count,2) int32, w (count,) float64) of the edges first ... in insertion order (the path search itself is `shortest_paths`);
        device tensors, or numpy arrays with host=True"""
        count = self.num_edges - int(first) if count is None else int(count)
        K = kind_on(self.ctx, host)
        uv, w = K.empty((count, 2), "int32"), K.empty(count, "float64")
        K.call("ccmp_roadmap_read_edges", "ccmp_roadmap_read_edges_host", self._h, int(first), count, K.arg(uv), K.arg(w), stream=stream)
        return uv, w

    def labels(self, first=0, count=None, host=False, stream=None):
        """labels (count,) int32: label[v] = the smallest vertex index of v's connected component"""
        count = len(self) - int(first) if count is None else int(count)
        K = kind_on(self.ctx, host)
        lab = K.empty(count, "int32")
        K.call("ccmp_roadmap_read_labels", "ccmp_roadmap_read_labels_host", self._h, int(first), count, K.arg(lab), stream=stream)
        return lab

    def closest(self, froms, target_pose, stream=None):
        """closestFromGoal's vertex scan (ccmp_roadmap_closest): for each of froms (F,) int32, F <= 64, the vertex of from's component
        with the smallest (pose distance to target_pose, index): (idx (F,), dist (F,), from_dist (F,)), from_dist = the distance of
        `from` itself.  A NaN distance is never a candidate.  numpy in, numpy out (synchronous); device tensors in (target_pose (8,)),
        device tensors out, asynchronous and capturable."""
        K = kind_of(froms)
        if K is HOST:  # any shape of indices and any pose of seven numbers or more, padded here
            fr, tgt = K.expect(froms, "int32", -1, "froms"), _pose8(target_pose)
        else:
            fr, tgt = K.expect(froms, "int32", (None,), "froms"), K.expect(target_pose, "float64", -1, "target_pose")
            if tgt.numel() < 7:
                raise ValueError("target_pose: a pose of seven numbers or more")
        F = len(fr)
        idx, dist, fd = K.empty(F, "int32"), K.empty(F, "float64"), K.empty(F, "float64")
        K.call("ccmp_roadmap_closest", "ccmp_roadmap_closest_host", self._h, K.arg(fr), F, K.arg(tgt), K.arg(idx), K.arg(dist), K.arg(fd), stream=stream)
        return idx, dist, fd

    def closest_from_goal(self, froms, to):
        """The reference's closestFromGoal(froms, {to}, closest) (stefanBiPRM.cpp:641-690) from `closest`'s per-from answers: closestVal
        is carried across `froms`, each from first offers its own distance, `closest` = the best vertex of the LAST from's component if
        it is strictly better than closestVal, else that from; only tos[0] is used.  Returns (closest, closestVal); (None, inf) for no
        froms.  The one difference: the reference scans the vertices its A* sweep has ranked, and the sweep stops when it reaches `to` —
        so this equals closestFromGoal whenever `to` is not in the component; when it is, both answer distance 0 (the vertex `to`, or a
        lower-indexed vertex with the same pose)."""
        froms = [int(f) for f in froms]
        if not froms:
            return None, float("inf")
        _, pose = self.read(int(to), 1, host=True)
        idx, dist, fd = self.closest(np.array(froms, dtype=np.int32), pose[0])
        closest, val = None, float("inf")
        for f, i, d, h in zip(froms, idx, dist, fd):
            if h < val:
                val = float(h)
            closest = f
            if i >= 0 and d < val:
                closest, val = int(i), float(d)
        return closest, val

    # ---- shortest paths: the planner's solution step (include/ccmp.h; csrc/ccmp_path.h) ------------------------------------------------
    def shortest_paths(self, src, dst, max_len=64, host=False, stream=None, full=False):
        """The cheapest path of every pair (src[f], dst[f]), F <= 64, on the store's graph, on the device (ccmp_roadmap_shortest_paths):
        distances are the least fixed point of d[v] = min fl(d[u] + w), ties go to the fewest hops and then to the smallest predecessor
        (csrc/ccmp_path.h) — the cheapest path, not boost's A* under the reference's inadmissible heuristic.  Returns a dict: cost (F,)
        (+inf: not connected), path_len (F,) (0: not connected), path (F,L) int32 and joints (F,L,14), poses (F,L,8) (the first path_len[f]
        rows of f are the path, start first), L = the buffer's length: max_len, or the longest path when one did not fit — the call is
        then made once more with that length.  Device tensors (src / dst may be given as such: int32, on the device), or numpy arrays
        with host=True (the synchronous host form; an index outside the store raises).  full=True adds dist (F,N) and pred (F,N)."""
        N = len(self)
        K = kind_on(self.ctx, host)

        def pairs(a):
            if host:  # from wherever they are
                return K.expect(a.cpu() if hasattr(a, "cpu") else a, "int32", -1, "src / dst")
            if not hasattr(a, "data_ptr"):
                a = _torch().from_numpy(np.array(a, dtype=np.int32).reshape(-1)).to(K.device)
            return K.expect(a, "int32", (None,), "src / dst")

        sr, ds = pairs(src), pairs(dst)
        F = len(sr)
        if not host and len(ds) != F:
            raise ValueError("src and dst are (F,) each")
        nan = float("nan")
        for ml in (int(max_len), None):
            if ml is None:
                ml = longest
            out = {"cost": K.empty(F, "float64"), "path_len": K.empty(F, "int32"), "path": K.full((F, ml), "int32", -1), "joints": K.full((F, ml, 14), "float64", nan),
                   "poses": K.full((F, ml, 8), "float64", nan), **({"dist": K.empty((F, N), "float64"), "pred": K.empty((F, N), "int32")} if full else {})}
            K.call("ccmp_roadmap_shortest_paths", "ccmp_roadmap_shortest_paths_host", self._h, K.arg(sr), K.arg(ds), F, ml,
                   *[K.arg(out.get(n)) for n in ("cost", "path_len", "path", "joints", "poses", "dist", "pred")], stream=stream)
            longest = int(out["path_len"].max()) if F else 0  # the device form's one host read: did every path fit
            if longest <= ml:
                break
        return out

    def path_rounds(self, F):
        """(F,2) int32: the relaxation and hop rounds the last `shortest_paths` call took for each of its first F pairs; a diagnostic"""
        r = np.empty((int(F), 2), dtype=np.int32)
        check(_lib.lib().ccmp_roadmap_path_rounds_host(self._h, int(F), _arg(r)), "ccmp_roadmap_path_rounds_host")
        return r

    def solution(self, starts, goals, max_len=64):
        """maybeConstructSolution (stefanBiPRM.cpp:480-603) on the device: of the pairs (start, goal) whose component labels agree, the
        cheapest path — one `shortest_paths` call for those pairs (at most 64 of them), the first pair in starts-major order wins a
        tie.  Returns (cost, indices (len,) int32 numpy, joints (len,14) device tensor), or None when no pair is connected.  The joint
        rows are what `KinematicChainConstraint.densify_paths` takes to densify the path (PathGeometric::interpolate): `dense_solution`."""
        starts, goals = [int(s) for s in starts], [int(g) for g in goals]
        if not starts or not goals:
            return None
        lab = self.labels(host=True)
        pairs = [(s, g) for s in starts for g in goals if lab[s] == lab[g]]
        if not pairs:
            return None
        if len(pairs) > _lib.PATH_MAX_PAIRS:
            raise ValueError("more than %d connected (start, goal) pairs" % _lib.PATH_MAX_PAIRS)
        out = self.shortest_paths(np.array([p[0] for p in pairs], dtype=np.int32), np.array([p[1] for p in pairs], dtype=np.int32), max_len=max_len)
        cost = out["cost"].cpu().numpy()
        if not np.isfinite(cost).any():  # connected only through edges that cannot be traversed (a pose-only endpoint)
            return None
        f = int(np.argmin(np.where(np.isfinite(cost), cost, np.inf)))  # argmin: the first of equal costs
        n = int(out["path_len"][f])
        return float(cost[f]), out["path"][f, :n].cpu().numpy(), out["joints"][f, :n].contiguous()

    def approximate_solution(self, starts, goal_pose, max_len=64):
        """constructApproximateSolution (stefanBiPRM.cpp:161-239) on the device: `closest` gives, per start, the vertex of its component
        nearest to goal_pose; the path goes from the start whose vertex is nearest (the first start wins a tie) to that vertex.
        Returns (distance to the goal pose, cost, indices (len,) int32 numpy, joints (len,14) device tensor), or None without starts."""
        starts = [int(s) for s in starts]
        if not starts:
            return None
        idx, dist, _ = self.closest(np.array(starts, dtype=np.int32), _pose8(goal_pose))
        if not (idx >= 0).any():
            return None
        i = int(np.argmin(np.where(idx >= 0, dist, np.inf)))
        out = self.shortest_paths(np.array([starts[i]], dtype=np.int32), np.array([idx[i]], dtype=np.int32), max_len=max_len)
        n = int(out["path_len"][0])
        return float(dist[i]), float(out["cost"][0]), out["path"][0, :n].cpu().numpy(), out["joints"][0, :n].contiguous()

    @staticmethod
    def _dense(constraint, joints, kw):
        """one path's waypoint rows (len,14), on the device, through `KinematicChainConstraint.densify_paths`"""
        torch = _torch()
        n = joints.shape[0]
        plen = torch.full((1,), n, dtype=torch.int32, device=joints.device)
        return constraint.densify_paths(joints.reshape(1, n, 14).contiguous(), plen, **kw)

    def dense_solution(self, constraint, starts, goals, max_len=64, **kw):
        """`solution` followed by `constraint.densify_paths` on its joint rows (PathGeometric::interpolate): the path never leaves the
        device between the two.  Returns (cost, indices, dense) with dense the dict of `densify_paths` (kw: its keyword arguments),
        or None when no pair is connected.  `space.format_path_matrix(dense["joints"].cpu().numpy())` is the reference's <obj>_path.txt."""
        sol = self.solution(starts, goals, max_len=max_len)
        if sol is None:
            return None
        return sol[0], sol[1], self._dense(constraint, sol[2], kw)

    def dense_approximate_solution(self, constraint, starts, goal_pose, max_len=64, **kw):
        """`approximate_solution` followed by `constraint.densify_paths`: (distance to the goal pose, cost, indices, dense), or None"""
        sol = self.approximate_solution(starts, goal_pose, max_len=max_len)
        if sol is None:
            return None
        return sol[0], sol[1], sol[2], self._dense(constraint, sol[3], kw)

    _SHORTCUT_KW = ("scene", "margin", "max_span", "chunk_states", "round_budget", "max_calls", "tile_edges", "pairs")

    def shortcut_solution(self, constraint, starts, goals, max_len=64, **kw):
        """`solution` followed by `constraint.shortcut_paths` on its joint rows (kw: its keyword arguments): interior vertices the
        constraint's checkMotion can do without are removed, on the device.  Returns (cost of the shortcut path, indices of the kept
        vertices (len,) int32 numpy, joints (len,14) device tensor, shortcut) with shortcut the dict of `shortcut_paths`, or None when
        no pair is connected."""
        torch = _torch()
        sol = self.solution(starts, goals, max_len=max_len)
        if sol is None:
            return None
        _, idx, joints = sol
        n = joints.shape[0]
        plen = torch.full((1,), n, dtype=torch.int32, device=joints.device)
        sc = constraint.shortcut_paths(joints.reshape(1, n, 14).contiguous(), plen, **kw)
        m = int(sc["out_len"][0])
        keep = sc["kept"][0, :m].cpu().numpy()
        return float(sc["cost_out"][0]), idx[keep], sc["joints"][0, :m].contiguous(), sc

    def dense_shortcut_solution(self, constraint, starts, goals, max_len=64, **kw):
        """solution -> shortcut -> densify, each step on the device outputs of the one before: `shortcut_solution` (its keyword arguments
        among kw), then `constraint.densify_paths` on the kept rows (the remaining kw; a scene and its margin go to both).  Returns
        (cost, indices, dense, shortcut), or None.  The dense rows are what the host's validity test takes next."""
        skw = {k: v for k, v in kw.items() if k in self._SHORTCUT_KW}
        dkw = {k: v for k, v in kw.items() if k not in ("max_span", "tile_edges", "pairs")}
        sol = self.shortcut_solution(constraint, starts, goals, max_len=max_len, **skw)
        if sol is None:
            return None
        return sol[0], sol[1], self._dense(constraint, sol[2], dkw), sol[3]

    _SMOOTH_KW = ("max_steps", "min_change", "out_max_len", "stats")

    def smooth_solution(self, constraint, starts, goals, max_len=64, **kw):
        """solution -> shortcut -> smooth, each step on the device outputs of the one before: `shortcut_solution` (its keyword arguments
        among kw), then `constraint.smooth_paths` on the kept rows (max_steps, min_change, out_max_len, stats among kw; a scene and its
        margin, chunk_states, round_budget, max_calls and tile_edges go to both).  Returns (length of the smoothed path, indices of the
        vertices the shortcut kept, joints (len,14) device tensor, smooth, shortcut) with smooth the dict of `smooth_paths`, or None when
        no pair is connected.  The smoothed vertices other than the first and the last are not roadmap vertices."""
        torch = _torch()
        skw = {k: v for k, v in kw.items() if k in self._SHORTCUT_KW}
        mkw = {k: v for k, v in kw.items() if k in self._SMOOTH_KW or k in ("scene", "margin", "chunk_states", "round_budget", "max_calls", "tile_edges")}
        sol = self.shortcut_solution(constraint, starts, goals, max_len=max_len, **skw)
        if sol is None:
            return None
        _, idx, joints, sc = sol
        n = joints.shape[0]
        plen = torch.full((1,), n, dtype=torch.int32, device=joints.device)
        sm = constraint.smooth_paths(joints.reshape(1, n, 14).contiguous(), plen, **mkw)
        m = int(sm["out_len"][0])
        return float(sm["length_out"][0]), idx, sm["joints"][0, :m].contiguous(), sm, sc

    def dense_smooth_solution(self, constraint, starts, goals, max_len=64, **kw):
        """solution -> shortcut -> smooth -> densify: `smooth_solution`, then `constraint.densify_paths` on the smoothed rows (the
        remaining kw, `distinct` for one; a scene and its margin go to all three).  Returns (length, indices, dense, smooth, shortcut), or
        None.  The dense rows are what the host's validity test takes next."""
        own = ("max_span", "tile_edges", "pairs") + self._SMOOTH_KW
        dkw = {k: v for k, v in kw.items() if k not in own}
        sol = self.smooth_solution(constraint, starts, goals, max_len=max_len, **{k: v for k, v in kw.items() if k != "distinct"})
        if sol is None:
            return None
        return sol[0], sol[1], self._dense(constraint, sol[2], dkw), sol[3], sol[4]

    def timed_solution(self, constraint, starts, goals, vmax, amax, beta=0.5, count=None, spacing=None, max_rows=65536, max_len=64, **kw):
        """solution -> shortcut -> smooth -> densify -> resample -> time stamps on device tensors: `dense_smooth_solution` (kw: its keyword
        arguments), then `constraint.resample_paths` on the dense result where the library keeps it and `constraint.timestamp_paths` on
        the new rows.  Returns (duration, indices, sampled, stamps, dense, smooth, shortcut) with sampled and stamps the dicts of the two
        calls, or None when no pair is connected.  The resampled rows are new states: put sampled["joints"] to the host's validity test
        before the times are used."""
        sol = self.dense_smooth_solution(constraint, starts, goals, max_len=max_len, keep_handle=True, **kw)
        if sol is None:
            return None
        _, idx, dense, sm, sc = sol
        try:
            sampled = constraint.resample_paths(dense, count=count, spacing=spacing, max_rows=max_rows)
        finally:
            dense.pop("handle").close()  # the dense arrays stay; the library's copy goes
        stamps = constraint.timestamp_paths(sampled["joints"], sampled["path_first"], vmax, amax, beta=beta)
        return float(stamps["duration"][0]), idx, sampled, stamps, dense, sm, sc

    def executable_solution(self, constraint, starts, goals, vmax, amax, period=0.001, max_ticks=65536, audit_scene=None, audit_margin=0.0, fit=False,
                            fit_aim=0.95, fit_max_passes=8, jmax=None, jerk_window=0, jerk_max_window=64, **kw):
        """solution -> shortcut -> smooth -> densify -> resample -> time stamps -> [fit ->] setpoints and audit: `timed_solution` (kw: its
        keyword arguments), then `constraint.setpoint_paths` on its rows and stamps; audit_scene / audit_margin: the proxy scene the ticks'
        clearance is taken against.  Returns (setpoints, duration, indices, sampled, stamps, dense, smooth, shortcut) with setpoints the dict
        of `setpoint_paths`, or None when no pair is connected.  fit=True: the stamps go through `constraint.fit_timestamps` (period,
        max_ticks, fit_aim, fit_max_passes) first, the setpoints are those of the fitted stamps, and the fit's dict is appended to the
        tuple (duration and stamps stay the time-stamp rule's; the fitted ones are the dict's).  jmax (14 numbers): the setpoints are
        `constraint.jerk_setpoint_paths`' (jerk_window, jerk_max_window), after the fit when fit=True — the dict then has window, passes
        and six peaks and no stretch.  The resampled rows are new states: they go to the host's validity test first."""
        sol = self.timed_solution(constraint, starts, goals, vmax, amax, **kw)
        if sol is None:
            return None
        sampled, stamps = sol[2], sol[3]
        if audit_scene is None and kw.get("scene") is not None:  # the scene the path was made against audits it too
            audit_scene, audit_margin = kw["scene"], kw.get("margin", audit_margin)
        time, fitted = stamps["time"], ()
        if fit:
            fitted = (constraint.fit_timestamps(sampled["joints"], sampled["path_first"], time, vmax, amax, period=period, max_ticks=max_ticks, aim=fit_aim,
                                                max_passes=fit_max_passes),)
            time = fitted[0]["time"]
        if jmax is not None:
            sp = constraint.jerk_setpoint_paths(sampled["joints"], sampled["path_first"], time, vmax, amax, jmax, period=period, max_ticks=max_ticks,
                                                window=jerk_window, max_window=jerk_max_window, scene=audit_scene, margin=audit_margin)
        else:
            sp = constraint.setpoint_paths(sampled["joints"], sampled["path_first"], time, vmax, amax, period=period, max_ticks=max_ticks,
                                           scene=audit_scene, margin=audit_margin)
        return (sp,) + tuple(sol) + fitted

    def plan(self, constraint, checker, goal_joints=None, scene=None, margin=0.0, width=32, k=5, max_cycles=0, rng_seed=0, first_index=0, ik_opts=None,
             **opts):
        """The planner's loop on this store (ccmp_plan_create: stefanBiPRM::solve as include/ccmp.h states it): opens a `Plan` from
        `constraint`'s problem — start state problem.start_joint, start and goal object poses obj_start_* / obj_goal_* — and `checker` (an
        `ObjectChecker`); goal_joints (14,): the goal state, else the pose IK towards the goal pose seeded from the start state; scene /
        margin: the proxy scene the IK vets against and the traversals test (the vetted forms).  width candidates per growth step, k
        neighbours; opts: the other fields of ccmp_plan_opts (attempts, max_states, t, sigma, inflate, lo, hi, max_vertices).  Runs
        max_cycles cycles (0: open only) and returns the `Plan`; `Plan.run` resumes it."""
        constraint._need_problem()
        o = plan_options(width=int(width), k=int(k), **opts)
        gj = None if goal_joints is None else HOST.expect(np.asarray(goal_joints.cpu() if hasattr(goal_joints, "cpu") else goal_joints, dtype=np.float64), "float64", 14,
                                                         "goal_joints")
        h = C.c_void_p()
        check(_lib.lib().ccmp_plan_create(self._h, C.byref(constraint.problem), checker._h, scene._h if scene is not None else None, float(margin),
                                          C.byref(ik_opts) if ik_opts is not None else None, C.byref(o), _arg(gj), int(rng_seed), int(first_index), C.byref(h)),
              "ccmp_plan_create")
        pl = Plan(self, checker, scene, h)
        if max_cycles:
            pl.run(max_cycles)
        return pl

    def nearest_in_tree(self, roots, queries, stream=None):
        """The nearest vertex, under the joint distance, of each of queries (Q,14) among the vertices whose label is the label of one of
        roots (at most 8 indices): (idx (Q,) int32, dist (Q,) float64), ranked by (distance, index); idx -1 / dist +inf for an empty tree;
        NaN (pose-only) vertices are never an answer (ccmp_roadmap_nearest_in_tree).  numpy queries: the synchronous host form (a root
        outside the store raises); a device tensor: asynchronous, roots a device int32 tensor or a sequence (uploaded)."""
        K = kind_of(queries)
        q = K.expect(queries, "float64", (None, 14), "queries")
        if K is HOST:
            rt = HOST.expect(list(roots) if not isinstance(roots, np.ndarray) else roots, "int32", -1, "roots")
        elif hasattr(roots, "data_ptr"):
            rt = K.expect(roots, "int32", (None,), "roots")
        else:
            rt = _torch().from_numpy(np.array(list(roots), dtype=np.int32).reshape(-1)).to(K.device)
        Q = len(q)
        idx, dist = K.empty(Q, "int32"), K.empty(Q, "float64")
        K.call("ccmp_roadmap_nearest_in_tree", "ccmp_roadmap_nearest_in_tree_host", self._h, K.arg(rt, True), len(rt), K.arg(q), Q, K.arg(idx), K.arg(dist),
               stream=stream)
        return idx, dist

    def rrt_connect(self, constraint, start_joints=None, goal_joints=None, starts=None, goals=None, scene=None, margin=0.0, width=32, range=0.1,
                    max_cycles=0, rng_seed=0, first_index=0, **opts):
        """RRT-Connect on this store (ccmp_rrtc_create: the cycle include/ccmp.h states, and its differences from OMPL's RRTConnect): two
        trees in joint space grown from `constraint`'s projected sampler, the traversal and — with `scene` / `margin` — the proxy scene's
        validity test; no object checker, no IK.  starts / goals: indices of vertices already in the store (at most 8 each); or
        start_joints / goal_joints, joint rows (14,) or (n,14), which are appended here.  width samples per cycle, extensions clipped at
        `range`; opts: the other fields of ccmp_rrtc_opts (max_states, round_budget, max_vertices).  Runs max_cycles cycles (0: open
        only) and returns the `RRTConnect`; its `run` resumes it, its `solution()` is `shortest_paths` on the solved pair."""
        constraint._need_problem()

        def side(idx, joints, what):
            if (idx is None) == (joints is None):
                raise ValueError("%s: vertex indices or joint rows, one of the two" % what)
            if idx is not None:
                return [int(v) for v in idx]
            rows = np.ascontiguousarray(np.asarray(joints.cpu() if hasattr(joints, "cpu") else joints, dtype=np.float64).reshape(-1, 14))
            first = self.append(joints=rows)
            return list(np.arange(first, first + len(rows)))

        s, g = side(starts, start_joints, "starts"), side(goals, goal_joints, "goals")
        o = rrtc_options(width=int(width), range=float(range), **opts)
        sa, ga = np.array(s, dtype=np.int32), np.array(g, dtype=np.int32)
        h = C.c_void_p()
        check(_lib.lib().ccmp_rrtc_create(self._h, C.byref(constraint.problem), scene._h if scene is not None else None, float(margin), C.byref(o), _arg(sa, True),
                                          len(sa), _arg(ga, True), len(ga), int(rng_seed), int(first_index), C.byref(h)), "ccmp_rrtc_create")
        pl = RRTConnect(self, scene, h)
        if max_cycles:
            pl.run(max_cycles)
        return pl

    def close(self):
        if self._h:
            _lib.lib().ccmp_roadmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
