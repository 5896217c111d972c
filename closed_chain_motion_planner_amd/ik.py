"""Pose-targeted IK, growTree's sampleCalibGoal step (include/ccmp.h: ccmp_pose_ik_*; the solver and the rule: csrc/ccmp_ik.h).

For every object pose the hand target of arm a is T_obj * t_o7[a]; each seed slot is tried in order, per arm first from the slot's own
seven joints and then from Gaussian restarts around mid-range, of which the converged one closest to the seed is kept; the first slot
on which both arms succeed gives the state.  TRAC-IK is not restated: the solver is this project's damped-least-squares Newton
iteration on the projector's forward kinematics.  `pose_ik_ref` runs the same text on the host (no device); the device forms are
`KinematicChainConstraint.pose_ik_batch` and `Roadmap.grow`.

With a proxy scene the calls are the VETTED forms (ccmp_pose_ik_vetted_*; csrc/ccmp_ik_vet.h): the scene stands where the reference puts
IKValid on every candidate and si_->isValid on the assembled state — a candidate is admissible only if its arm's clearance exceeds the
margin, a slot only if the assembled state's does.  Proxies, not MoveIt: the host's own validity test of the returned state stays.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._arrays import kind_of
from ._lib import CcmpIkOpts
from .scene import scene_arrays

__all__ = ["ik_options", "pose_ik_ref", "pose_ik", "pose_ik_vetted_ref"]


def ik_options(**kw):
    """ccmp_ik_opts with the library's defaults (restarts 14, max_rounds 64, eps 1e-5, lambda_ 0.05, err_clamp 0.5, sigma 0.3), fields
    overridden by keyword"""
    o = CcmpIkOpts()
    _lib.lib().ccmp_ik_opts_default(C.byref(o))
    for name, v in kw.items():
        if name == "lambda":
            name = "lambda_"
        if name not in dict(CcmpIkOpts._fields_):
            raise TypeError("ccmp_ik_opts has no field %r" % name)
        setattr(o, name, v)
    return o


def _inputs(K, target_poses, seeds):
    tp = K.expect(target_poses, "float64", (None, 8), "target_poses (T, 8)")
    sd = K.expect(seeds, "float64", (len(tp), None, 14), "seeds (T, S, 14)")
    return tp, sd, len(tp), int(sd.shape[1])


def _vetted(ctx_handle, problem, target_poses, seeds, rng_seed, first_index, opts, want_candidates, stream, scene, margin):
    """ccmp_pose_ik_vetted_host / _batch / _ref; scene: a ProxyScene, or for the host reference (ctx_handle None) the caller's arrays as a
    tuple (spheres, boxes, allowed)"""
    ref = isinstance(scene, tuple)
    R1 = 1 + int(opts.restarts)
    K = kind_of(target_poses)
    tp, sd, T, S = _inputs(K, target_poses, seeds)
    out = {"q": K.empty((T, 14), "float64"), "ok": K.empty(T, "uint8"), "which": K.empty(T, "int32"), "clearance": K.empty(T, "float64"),
           **({"cand_q": K.empty((T, S, 2, R1, 7), "float64"), "cand_rounds": K.empty((T, S, 2, R1), "int32"), "cand_clear": K.empty((T, S, 2, R1), "float64"),
               "slot_clear": K.empty((T, S), "float64")} if want_candidates else {})}
    K.call("ccmp_pose_ik_vetted_batch", "ccmp_pose_ik_vetted_ref" if ref else "ccmp_pose_ik_vetted_host", *(() if ref else (ctx_handle,)), C.byref(problem),
           C.byref(opts), K.arg(tp), K.arg(sd), T, S, int(rng_seed), int(first_index), *(scene_arrays(*scene) if ref else (scene._h,)),
           0.0 if margin is None else float(margin),
           *[K.arg(out.get(n)) for n in ("q", "ok", "which", "cand_q", "cand_rounds", "cand_clear", "slot_clear", "clearance")], stream=stream)
    return out


def pose_ik(ctx_handle, problem, target_poses, seeds, rng_seed=0, first_index=0, opts=None, want_candidates=False, stream=None, ref=False, scene=None,
            margin=None):
    """The three forms behind one signature.  numpy arrays: ccmp_pose_ik_ref (ref=True, no context) or ccmp_pose_ik_host; torch tensors
    on the device: ccmp_pose_ik_batch on `stream`.  Returns a dict: q (T,14), ok (T,) uint8, which (T,) int32 and, with
    want_candidates, cand_q (T,S,2,1+R,7) and cand_rounds (T,S,2,1+R) int32.
    scene (a ProxyScene) and margin (None = 0): the vetted forms, ccmp_pose_ik_vetted_* — the dict also holds clearance (T,) and, with
    want_candidates, cand_clear (T,S,2,1+R) and slot_clear (T,S).  Without a scene the call is the plain one, as before."""
    opts = opts if opts is not None else ik_options()
    if scene is not None:
        return _vetted(ctx_handle, problem, target_poses, seeds, rng_seed, first_index, opts, want_candidates, stream, scene, margin)
    R1 = 1 + int(opts.restarts)
    K = kind_of(target_poses)
    tp, sd, T, S = _inputs(K, target_poses, seeds)
    out = {"q": K.empty((T, 14), "float64"), "ok": K.empty(T, "uint8"), "which": K.empty(T, "int32"),
           **({"cand_q": K.empty((T, S, 2, R1, 7), "float64"), "cand_rounds": K.empty((T, S, 2, R1), "int32")} if want_candidates else {})}
    K.call("ccmp_pose_ik_batch", "ccmp_pose_ik_ref" if ref else "ccmp_pose_ik_host", *(() if ref else (ctx_handle,)), C.byref(problem), C.byref(opts), K.arg(tp),
           K.arg(sd), T, S, int(rng_seed), int(first_index), *[K.arg(out.get(n)) for n in ("q", "ok", "which", "cand_q", "cand_rounds")], stream=stream)
    return out


def pose_ik_ref(problem, target_poses, seeds, rng_seed=0, first_index=0, opts=None, want_candidates=False):
    """ccmp_pose_ik_ref: the solver's text compiled for the host, one thread, no device — the same bits as the kernels"""
    return pose_ik(None, problem, np.asarray(target_poses, dtype=np.float64), np.asarray(seeds, dtype=np.float64), rng_seed, first_index, opts,
                   want_candidates, ref=True)


def pose_ik_vetted_ref(problem, target_poses, seeds, spheres, boxes=(), allowed=None, margin=0.0, rng_seed=0, first_index=0, opts=None,
                       want_candidates=False):
    """ccmp_pose_ik_vetted_ref: the vetted rule's text compiled for the host on the caller's scene arrays (ProxyScene's tuples), one
    thread, no device — the same bits as the kernels"""
    return _vetted(None, problem, np.asarray(target_poses, dtype=np.float64), np.asarray(seeds, dtype=np.float64), rng_seed, first_index,
                   opts if opts is not None else ik_options(), want_candidates, None, (list(spheres), list(boxes), allowed), margin)
