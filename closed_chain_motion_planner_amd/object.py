"""The head of growTree: object-pose proposal and the mesh-against-workspace test (include/ccmp.h: ccmp_object_*; the arithmetic and
every term order: csrc/ccmp_object.h).

The reference (stefanBiPRM.cpp:255-276) interpolates the object pose 30 % from the nearest vertex towards the goal, draws an SE(3)
Gaussian sample around it (sigma 0.2, two attempts), asks `stefan_checker_->isValid` and only then grows; `checkForSolution`
(:733-752) walks nine interpolated poses towards the goal; `stefanFCL::isFeasible` tests the object's triangle mesh against six
static boxes.  OMPL's interpolate and sampleGaussian are restated from their published definitions; its random numbers and FCL's BVH
and GJK are not — the deviates are this library's counter-based Box-Muller and the mesh test is an exact separating-axis test of a
triangle against an oriented box.  Meshes are the caller's, (M, 9) numbers in the object frame; the library hard-codes no workspace.

`ObjectChecker` is the device form (torch tensors: asynchronous on a stream; numpy arrays: the synchronous host form);
`object_valid_ref` / `object_propose_ref` / `pose_interpolate` run the same text on the host without a device: the same bits.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._arrays import HOST, kind_of
from ._lib import CcmpBox, check

__all__ = ["ObjectChecker", "object_valid_ref", "object_propose_ref", "pose_interpolate", "boxes_from", "DEFAULT_LO", "DEFAULT_HI"]

# position bounds of the draw when the caller gives none: effectively unbounded (the planner passes its object space's bounds)
DEFAULT_LO, DEFAULT_HI = (-1e30,) * 3, (1e30,) * 3


def boxes_from(boxes):
    """[{"c": (3), "half": (3), "R": (9, optional: identity)}] or CcmpBox instances -> a ctypes array of ccmp_box"""
    arr = (CcmpBox * len(boxes))()
    for i, b in enumerate(boxes):
        if isinstance(b, CcmpBox):
            arr[i] = b
            continue
        arr[i].c[:] = [float(v) for v in b["c"]]
        arr[i].half[:] = [float(v) for v in b["half"]]
        arr[i].R[:] = [float(v) for v in np.asarray(b.get("R", np.eye(3)), dtype=np.float64).reshape(9)]
    return arr


def _tri(triangles):
    return HOST.expect(triangles, "float64", -1, "triangles").reshape(-1, 9)


def _poses(K, a, name="poses"):
    """pose rows (n, 8) of kind K; the host kind also takes one pose (8,)"""
    if K is HOST and np.ndim(a) == 1:
        a = np.reshape(a, (1, -1))
    return K.expect(a, "float64", (None, 8), name)


def _vec3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def pose_interpolate(a, b, t):
    """ccmp_pose_interpolate: OMPL's SE3StateSpace::interpolate on pose rows (x y z qx qy qz qw [pad]); host only, the kernels' bits"""
    a8, b8, out = np.zeros(8), np.zeros(8), np.empty(8)
    a8[:7], b8[:7] = np.asarray(a, dtype=np.float64)[:7], np.asarray(b, dtype=np.float64)[:7]
    _lib.lib().ccmp_pose_interpolate(HOST.arg(a8), HOST.arg(b8), float(t), HOST.arg(out))
    return out


def object_valid_ref(triangles, boxes, poses, inflate=0.0, want_mask=False, broad_phase=True):
    """ccmp_object_valid_ref: valid (T,) uint8 and, with want_mask, hit_mask (T,) uint32 — no device"""
    tri, bx, ps = _tri(triangles), boxes_from(boxes), _poses(HOST, poses)
    valid, mask = HOST.empty(len(ps), "uint8"), HOST.empty(len(ps), "uint32") if want_mask else None
    check(_lib.lib().ccmp_object_valid_ref(HOST.arg(tri), len(tri), bx, len(bx), HOST.arg(ps), len(ps), float(inflate), 1 if broad_phase else 0, HOST.arg(valid),
                                           HOST.arg(mask)), "ccmp_object_valid_ref")
    return (valid, mask) if want_mask else valid


def _propose_out(K, G, A, want_candidates):
    return {"pose": K.empty((G, 8), "float64"), "which": K.empty(G, "int32"),
            **({"cand_pose": K.empty((G, A, 8), "float64"), "cand_valid": K.empty((G, A), "uint8")} if want_candidates else {})}


def _propose_args(K, frm, to, t, sigma, lo, hi, attempts, rng_seed, first_index, inflate, out):
    """ccmp_object_propose_*'s arguments behind the mesh and the boxes"""
    if to.shape[0] not in (1, frm.shape[0]):
        raise ValueError("to_poses: one goal pose or one per from pose")
    return (K.arg(frm), K.arg(to), 0 if to.shape[0] == 1 else 8, len(frm), float(t), float(sigma), _vec3(lo), _vec3(hi), int(attempts), int(rng_seed),
            int(first_index), float(inflate), *[K.arg(out.get(n)) for n in ("pose", "which", "cand_pose", "cand_valid")])


def object_propose_ref(triangles, boxes, from_poses, to_poses, t=0.3, sigma=0.2, lo=DEFAULT_LO, hi=DEFAULT_HI, attempts=2, rng_seed=0, first_index=0,
                       inflate=0.0, want_candidates=False):
    """ccmp_object_propose_ref: the dict of `ObjectChecker.propose` — no device"""
    tri, bx, frm, to = _tri(triangles), boxes_from(boxes), _poses(HOST, from_poses, "from_poses"), _poses(HOST, to_poses, "to_poses")
    out = _propose_out(HOST, len(frm), max(int(attempts), 0), want_candidates)
    check(_lib.lib().ccmp_object_propose_ref(HOST.arg(tri), len(tri), bx, len(bx),
                                             *_propose_args(HOST, frm, to, t, sigma, lo, hi, attempts, rng_seed, first_index, inflate, out)), "ccmp_object_propose_ref")
    return out


class ObjectChecker:
    """ccmp_object on a context: the object's mesh (M, 9) on the device and the static workspace boxes.  `constraint_or_ctx`: a
    KinematicChainConstraint (its context is used) or a Context."""

    def __init__(self, constraint_or_ctx, triangles, boxes):
        self.ctx = getattr(constraint_or_ctx, "ctx", constraint_or_ctx)
        tri, bx = _tri(triangles), boxes_from(boxes)
        self._h = C.c_void_p()
        check(_lib.lib().ccmp_object_create(self.ctx.handle, HOST.arg(tri), len(tri), bx, len(bx), C.byref(self._h)), "ccmp_object_create")

    def __len__(self):
        return int(_lib.lib().ccmp_object_num_triangles(self._h))

    def valid(self, poses, inflate=0.0, want_mask=False, stream=None):
        """valid (T,) uint8 — the pose's mesh touches no box — and with want_mask hit_mask (T,) uint32 (torch: int32 with the same bits),
        bit b = box b is hit.  Without the mask a block leaves at its first hit; `valid` is the same."""
        K = kind_of(poses)
        ps = _poses(K, poses)
        valid, mask = K.empty(len(ps), "uint8"), K.empty(len(ps), "uint32") if want_mask else None
        K.call("ccmp_object_valid_batch", "ccmp_object_valid_host", self.ctx.handle, self._h, K.arg(ps), len(ps), float(inflate), K.arg(valid), K.arg(mask),
               stream=stream)
        return (valid, mask) if want_mask else valid

    def propose(self, from_poses, to_poses, t=0.3, sigma=0.2, lo=DEFAULT_LO, hi=DEFAULT_HI, attempts=2, rng_seed=0, first_index=0, inflate=0.0,
                want_candidates=False, stream=None):
        """growTree's head for G grow indices: per index the first of `attempts` candidates — interpolate from_poses[g] towards to_poses[g]
        (or the one goal pose) at t, then the SE(3) Gaussian draw of index (first_index + g) * attempts + a — whose mesh is free.  Returns a
        dict: pose (G, 8) (a NaN row where none was), which (G,) int32 (-1 where none was) and, with want_candidates, cand_pose (G, A, 8)
        and cand_valid (G, A) of every attempt."""
        K = kind_of(from_poses)
        frm = _poses(K, from_poses, "from_poses")
        to = _poses(K, to_poses.reshape(1, 8) if K is not HOST and to_poses.dim() == 1 else to_poses, "to_poses")
        out = _propose_out(K, len(frm), max(int(attempts), 0), want_candidates)
        K.call("ccmp_object_propose_batch", "ccmp_object_propose_host", self.ctx.handle, self._h,
               *_propose_args(K, frm, to, t, sigma, lo, hi, attempts, rng_seed, first_index, inflate, out), stream=stream)
        return out

    def ladder(self, from_pose, goal_pose, steps=9, inflate=0.0):
        """checkForSolution's ladder (stefanBiPRM.cpp:735-752): the poses interpolated at 0.1 * i, i = 1..steps, from `from_pose` towards
        `goal_pose`, and how many of them are valid before the first one that is refused.  Returns (poses (steps, 8), n_leading_valid)."""
        poses = np.stack([pose_interpolate(from_pose, goal_pose, 0.1 * i) for i in range(1, int(steps) + 1)])
        valid = self.valid(poses, inflate=inflate)
        bad = np.flatnonzero(valid == 0)
        return poses, int(bad[0]) if len(bad) else len(poses)

    def close(self):
        if self._h:
            _lib.lib().ccmp_object_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
