"""Pose-targeted IK, growTree's sampleCalibGoal step (include/ccmp.h: ccmp_pose_ik_*; the solver and the rule: csrc/ccmp_ik.h).

For every object pose the hand target of arm a is T_obj * t_o7[a]; each seed slot is tried in order, per arm first from the slot's own
seven joints and then from Gaussian restarts around mid-range, of which the converged one closest to the seed is kept; the first slot
on which both arms succeed gives the state.  TRAC-IK is not restated: the solver is this project's damped-least-squares Newton
iteration on the projector's forward kinematics.  `pose_ik_ref` runs the same text on the host (no device); the device forms are
`KinematicChainConstraint.pose_ik_batch` and `Roadmap.grow`.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CcmpIkOpts, check

__all__ = ["ik_options", "pose_ik_ref", "pose_ik"]

_dp, _i32p, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)


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


def _shape(target_poses, seeds):
    if target_poses.ndim != 2 or target_poses.shape[1] != 8:
        raise ValueError("target_poses: expected (T, 8), got %s" % (tuple(target_poses.shape),))
    T = target_poses.shape[0]
    if seeds.ndim != 3 or seeds.shape[0] != T or seeds.shape[2] != 14:
        raise ValueError("seeds: expected (T, S, 14) with T = %d, got %s" % (T, tuple(seeds.shape)))
    return T, int(seeds.shape[1])


def pose_ik(ctx_handle, problem, target_poses, seeds, rng_seed=0, first_index=0, opts=None, want_candidates=False, stream=None, ref=False):
    """The three forms behind one signature.  numpy arrays: ccmp_pose_ik_ref (ref=True, no context) or ccmp_pose_ik_host; torch tensors
    on the device: ccmp_pose_ik_batch on `stream`.  Returns a dict: q (T,14), ok (T,) uint8, which (T,) int32 and, with
    want_candidates, cand_q (T,S,2,1+R,7) and cand_rounds (T,S,2,1+R) int32."""
    L = _lib.lib()
    opts = opts if opts is not None else ik_options()
    R1 = 1 + int(opts.restarts)
    if isinstance(target_poses, np.ndarray):
        tp = np.ascontiguousarray(target_poses, dtype=np.float64)
        sd = np.ascontiguousarray(seeds, dtype=np.float64)
        T, S = _shape(tp, sd)
        out = {"q": np.empty((T, 14)), "ok": np.empty(T, dtype=np.uint8), "which": np.empty(T, dtype=np.int32)}
        if want_candidates:
            out["cand_q"] = np.empty((T, S, 2, R1, 7))
            out["cand_rounds"] = np.empty((T, S, 2, R1), dtype=np.int32)
        tail = (tp.ctypes.data_as(_dp), sd.ctypes.data_as(_dp), T, S, int(rng_seed), int(first_index), out["q"].ctypes.data_as(_dp),
                out["ok"].ctypes.data_as(_u8p), out["which"].ctypes.data_as(_i32p),
                out["cand_q"].ctypes.data_as(_dp) if want_candidates else None, out["cand_rounds"].ctypes.data_as(_i32p) if want_candidates else None)
        if ref:
            check(L.ccmp_pose_ik_ref(C.byref(problem), C.byref(opts), *tail), "ccmp_pose_ik_ref")
        else:
            check(L.ccmp_pose_ik_host(ctx_handle, C.byref(problem), C.byref(opts), *tail), "ccmp_pose_ik_host")
        return out
    from .constraint import _stream_handle, _torch

    torch = _torch()
    for t in (target_poses, seeds):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError("expected contiguous float64 tensors on the device")
    T, S = _shape(target_poses, seeds)
    dev = target_poses.device
    out = {"q": torch.empty((T, 14), dtype=torch.float64, device=dev), "ok": torch.empty(T, dtype=torch.uint8, device=dev),
           "which": torch.empty(T, dtype=torch.int32, device=dev)}
    if want_candidates:
        out["cand_q"] = torch.empty((T, S, 2, R1, 7), dtype=torch.float64, device=dev)
        out["cand_rounds"] = torch.empty((T, S, 2, R1), dtype=torch.int32, device=dev)
    check(L.ccmp_pose_ik_batch(ctx_handle, C.byref(problem), C.byref(opts), target_poses.data_ptr(), seeds.data_ptr(), T, S, int(rng_seed), int(first_index),
                               out["q"].data_ptr(), out["ok"].data_ptr(), out["which"].data_ptr(),
                               out["cand_q"].data_ptr() if want_candidates else None, out["cand_rounds"].data_ptr() if want_candidates else None,
                               _stream_handle(stream)), "ccmp_pose_ik_batch")
    return out


def pose_ik_ref(problem, target_poses, seeds, rng_seed=0, first_index=0, opts=None, want_candidates=False):
    """ccmp_pose_ik_ref: the solver's text compiled for the host, one thread, no device — the same bits as the kernels"""
    return pose_ik(None, problem, np.asarray(target_poses, dtype=np.float64), np.asarray(seeds, dtype=np.float64), rng_seed, first_index, opts,
                   want_candidates, ref=True)
