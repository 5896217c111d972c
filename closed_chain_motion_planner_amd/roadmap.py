"""Host mirror of the device-resident roadmap store (include/ccmp.h: ccmp_roadmap_*) and of the planner's tree metric.

The reference's `tree_` ranks on `obj_space_->distance(components[1], components[1])` (stefanBiPRM.h:194-201): the SE3 distance
between the object poses of two vertices.  `Roadmap` keeps the joints (14) and the object pose (x y z qx qy qz qw pad) of every
vertex on the device, so that the planner's append / query / sometimes-remove-the-last loop uploads one vertex per step, and ranks
on that metric (`_lib.METRIC_OBJECT`) or on the joint distance (`_lib.METRIC_JOINT`).

Arguments that are torch tensors are taken as device memory and the calls are asynchronous on the current (or given) stream; numpy
arrays go through the synchronous host forms and come back as numpy arrays.  All arithmetic happens in libccmp.so.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import METRIC_JOINT, METRIC_OBJECT, check
from .constraint import _stream_handle, _torch

__all__ = ["Roadmap", "pose_distance", "pose_from_t_wo", "METRIC_JOINT", "METRIC_OBJECT"]

_dp = C.POINTER(C.c_double)


def _host(a, cols):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != cols:
        raise ValueError("expected an (n, %d) float64 array, got %s" % (cols, (a.shape,)))
    return a


def _dev(t, cols):
    torch = _torch()
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[1] != cols or not t.is_contiguous() or not t.is_cuda:
        raise ValueError("expected a contiguous (n, %d) float64 tensor on the device" % cols)
    return t


def pose_distance(a, b):
    """ccmp_pose_distance: OMPL's SE3StateSpace::distance (weights 1 and 1) between two poses (x y z qx qy qz qw [pad]); host only"""
    a8, b8 = np.zeros(8), np.zeros(8)
    a8[:7], b8[:7] = np.asarray(a, dtype=np.float64)[:7], np.asarray(b, dtype=np.float64)[:7]
    return float(_lib.lib().ccmp_pose_distance(a8.ctypes.data_as(_dp), b8.ctypes.data_as(_dp)))


def pose_from_t_wo(t_wo):
    """ccmp_pose_from_t_wo: (..., 12) [R row-major, p] as `compute_t_wo_batch` returns it -> (..., 8) poses; host only"""
    t = np.ascontiguousarray(t_wo, dtype=np.float64)
    flat = t.reshape(-1, 12)
    out = np.empty((flat.shape[0], 8))
    fn = _lib.lib().ccmp_pose_from_t_wo
    for i in range(flat.shape[0]):
        fn(flat[i].ctypes.data_as(_dp), out[i].ctypes.data_as(_dp))
    return out.reshape(t.shape[:-1] + (8,))


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
        if isinstance(given, np.ndarray):
            j = _host(joints, 14) if joints is not None else None
            p = _host(poses, 8) if poses is not None else None
            check(_lib.lib().ccmp_roadmap_append_host(self._h, self._problem() if p is None else None, j.ctypes.data_as(_dp) if j is not None else None,
                                                      p.ctypes.data_as(_dp) if p is not None else None, len(given), C.byref(first)),
                  "ccmp_roadmap_append_host")
        else:
            j = _dev(joints, 14) if joints is not None else None
            p = _dev(poses, 8) if poses is not None else None
            check(_lib.lib().ccmp_roadmap_append(self._h, self._problem() if p is None else None, j.data_ptr() if j is not None else None,
                                                 p.data_ptr() if p is not None else None, given.shape[0], C.byref(first), _stream_handle(stream)),
                  "ccmp_roadmap_append")
        return int(first.value)

    def set_joints(self, index, joints, stream=None):
        """the joints of vertex `index` (growTree: after the IK of a pose-only vertex); its pose row stays"""
        if isinstance(joints, np.ndarray):
            j = np.ascontiguousarray(joints, dtype=np.float64).reshape(14)
            check(_lib.lib().ccmp_roadmap_set_joints_host(self._h, int(index), j.ctypes.data_as(_dp)), "ccmp_roadmap_set_joints_host")
        else:
            j = joints.reshape(1, 14)
            check(_lib.lib().ccmp_roadmap_set_joints(self._h, int(index), _dev(j, 14).data_ptr(), _stream_handle(stream)), "ccmp_roadmap_set_joints")

    def truncate(self, n):
        """drops the vertices from index n on (the reference's remove_vertex of the vertex just appended)"""
        check(_lib.lib().ccmp_roadmap_truncate(self._h, int(n)), "ccmp_roadmap_truncate")

    def read(self, first=0, count=None, host=False, stream=None):
        """(joints (count,14), poses (count,8)) of the vertices first ... — device tensors, or numpy arrays with host=True"""
        count = len(self) - int(first) if count is None else int(count)
        if host:
            j, p = np.empty((count, 14)), np.empty((count, 8))
            check(_lib.lib().ccmp_roadmap_read_host(self._h, int(first), count, j.ctypes.data_as(_dp), p.ctypes.data_as(_dp)), "ccmp_roadmap_read_host")
            return j, p
        torch = _torch()
        dev = torch.device("cuda", self.ctx.device)
        j = torch.empty((count, 14), dtype=torch.float64, device=dev)
        p = torch.empty((count, 8), dtype=torch.float64, device=dev)
        check(_lib.lib().ccmp_roadmap_read(self._h, int(first), count, j.data_ptr(), p.data_ptr(), _stream_handle(stream)), "ccmp_roadmap_read")
        return j, p

    def nearest_k(self, queries, k, metric=METRIC_OBJECT, mode=0, self_base=0, stream=None):
        """The k nearest vertices of every query: (Q,8) poses under METRIC_OBJECT, (Q,14) joints under METRIC_JOINT; modes, ranking
        and empty slots as `KinematicChainConstraint.nearest_k_batch`.  Returns (nbr_idx (Q,k) int32, nbr_dist (Q,k) float64)."""
        cols, k = (14 if metric == METRIC_JOINT else 8), int(k)
        if isinstance(queries, np.ndarray):
            q = _host(queries, cols)
            idx, dist = np.empty((len(q), k), dtype=np.int32), np.empty((len(q), k))
            check(_lib.lib().ccmp_roadmap_knn_host(self._h, int(metric), q.ctypes.data_as(_dp), len(q), k, int(mode), int(self_base),
                                                   idx.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(_dp)), "ccmp_roadmap_knn_host")
            return idx, dist
        torch = _torch()
        q = _dev(queries, cols)
        idx = torch.empty((q.shape[0], k), dtype=torch.int32, device=q.device)
        dist = torch.empty((q.shape[0], k), dtype=torch.float64, device=q.device)
        check(_lib.lib().ccmp_roadmap_knn(self._h, int(metric), q.data_ptr(), q.shape[0], k, int(mode), int(self_base), idx.data_ptr(), dist.data_ptr(),
                                          _stream_handle(stream)), "ccmp_roadmap_knn")
        return idx, dist

    def connect(self, query_joints, k, metric=METRIC_OBJECT, query_poses=None, mode=0, self_base=0, check_target=True, max_states=64,
                round_budget=0, scene=None, margin=None, stream=None):
        """Neighbours from the store by `metric`, then edge e = q * k + r from the store's joints at nbr_idx[q, r] to
        query_joints[q], exactly as `KinematicChainConstraint.connect_batch` runs its edges; the same dict comes back.
        METRIC_OBJECT ranks on `query_poses`, or on the poses derived from `query_joints` when they are None."""
        Q, k, ms = len(query_joints), int(k), int(max_states)
        E = Q * k
        shapes = {"nbr_idx": ((Q, k), "int32"), "nbr_dist": ((Q, k), "float64"), "states": ((E, ms, 14), "float64"), "n_states": ((E,), "int32"),
                  "ok": ((E,), "uint8"), "newton_iters": ((E,), "int32"), "blocked": ((E,), "uint8"), "carry": ((E, 2), "float64")}
        order = ["nbr_idx", "nbr_dist", "states", "n_states", "ok", "newton_iters", "blocked", "carry"]
        head = (self._h, self._problem(), scene._h if scene is not None else None, float(margin) if scene is not None else 0.0, int(metric))
        tail = (Q, k, int(mode), int(self_base), 1 if check_target else 0, ms, int(round_budget))
        if isinstance(query_joints, np.ndarray):
            qj = _host(query_joints, 14)
            qp = _host(query_poses, 8) if query_poses is not None else None
            out = {n: np.empty(s, dtype=d) for n, (s, d) in shapes.items()}
            ptr = lambda n: out[n].ctypes.data_as({"int32": C.POINTER(C.c_int32), "float64": _dp, "uint8": C.POINTER(C.c_uint8)}[shapes[n][1]])
            check(_lib.lib().ccmp_roadmap_connect_host(*head, qj.ctypes.data_as(_dp), qp.ctypes.data_as(_dp) if qp is not None else None, *tail,
                                                       *[ptr(n) for n in order]), "ccmp_roadmap_connect_host")
            return out
        torch = _torch()
        qj = _dev(query_joints, 14)
        qp = _dev(query_poses, 8) if query_poses is not None else None
        out = {n: torch.empty(s, dtype=getattr(torch, d), device=qj.device) for n, (s, d) in shapes.items()}
        check(_lib.lib().ccmp_roadmap_connect(*head, qj.data_ptr(), qp.data_ptr() if qp is not None else None, *tail,
                                              *[out[n].data_ptr() for n in order], _stream_handle(stream)), "ccmp_roadmap_connect")
        return out

    def grow(self, query_poses, k, mode=0, self_base=0, rng_seed=0, first_index=0, opts=None, check_target=False, max_states=64, round_budget=0,
             scene=None, margin=None, stream=None):
        """growTree's device part for the poses `query_poses` (Q,8) in one call (ccmp_roadmap_grow): the object-metric k-NN on the store,
        the neighbours' joints as seed slots in rank order, `KinematicChainConstraint.pose_ik_batch` on them, then edge e = q * k + r
        from neighbour r to the new state as `connect` runs its edges (check_target False: growTree's discreteGeodesic).  Returns
        `connect`'s dict plus q_new (Q,14), ik_ok (Q,), ik_which (Q,).  A pose without a state (and a neighbour without joints) has
        empty slots.  Nothing is appended: the reference adds the vertex only after an edge succeeded."""
        from .ik import ik_options

        Q, k, ms = len(query_poses), int(k), int(max_states)
        E = Q * k
        opts = opts if opts is not None else ik_options()
        shapes = {"nbr_idx": ((Q, k), "int32"), "nbr_dist": ((Q, k), "float64"), "q_new": ((Q, 14), "float64"), "ik_ok": ((Q,), "uint8"),
                  "ik_which": ((Q,), "int32"), "states": ((E, ms, 14), "float64"), "n_states": ((E,), "int32"), "ok": ((E,), "uint8"),
                  "newton_iters": ((E,), "int32"), "blocked": ((E,), "uint8"), "carry": ((E, 2), "float64")}
        order = list(shapes)
        head = (self._h, self._problem(), scene._h if scene is not None else None, float(margin) if scene is not None else 0.0, C.byref(opts))
        tail = (Q, k, int(mode), int(self_base), int(rng_seed), int(first_index), 1 if check_target else 0, ms, int(round_budget))
        if isinstance(query_poses, np.ndarray):
            qp = _host(query_poses, 8)
            out = {n: np.empty(s, dtype=d) for n, (s, d) in shapes.items()}
            ptr = lambda n: out[n].ctypes.data_as({"int32": C.POINTER(C.c_int32), "float64": _dp, "uint8": C.POINTER(C.c_uint8)}[shapes[n][1]])
            check(_lib.lib().ccmp_roadmap_grow_host(*head, qp.ctypes.data_as(_dp), *tail, *[ptr(n) for n in order]), "ccmp_roadmap_grow_host")
            return out
        torch = _torch()
        qp = _dev(query_poses, 8)
        out = {n: torch.empty(s, dtype=getattr(torch, d), device=qp.device) for n, (s, d) in shapes.items()}
        check(_lib.lib().ccmp_roadmap_grow(*head, qp.data_ptr(), *tail, *[out[n].data_ptr() for n in order], _stream_handle(stream)), "ccmp_roadmap_grow")
        return out

    def grow_toward(self, checker, from_poses, goal_pose, k, t=0.3, sigma=0.2, lo=None, hi=None, attempts=2, rng_seed=0, first_index=0, inflate=0.0,
                    **grow_args):
        """The whole of growTree's device part (stefanBiPRM.cpp:255-351): `checker.propose` (an `ObjectChecker`: interpolate from_poses[g]
        towards goal_pose, draw, test the mesh, `attempts` times), then `grow` on the poses that were found.  Indices without a valid
        candidate (which = -1: the reference's TRAPPED) never reach `grow`.  The flags make one small host read in between — growTree
        needs that decision on the host anyway.  Returns `grow`'s dict over the kept poses plus "which" (G,), "rows" (the grow index g of
        every row of the other entries) and "poses" (the kept poses); rng_seed and first_index serve both the draw and the IK restarts
        (row r of `grow` uses first_index + r); grow_args go to `grow`."""
        from .object import DEFAULT_HI, DEFAULT_LO

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

    def close(self):
        if self._h:
            _lib.lib().ccmp_roadmap_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
