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
from ._lib import CcmpIkOpts, check

__all__ = ["ik_options", "pose_ik_ref", "pose_ik", "pose_ik_vetted_ref"]

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


def _vetted(ctx_handle, problem, target_poses, seeds, rng_seed, first_index, opts, want_candidates, stream, scene, margin):
    """ccmp_pose_ik_vetted_host / _batch / _ref; scene: a ProxyScene, or for the host reference (ctx_handle None) the caller's arrays as a
    tuple (spheres, boxes, allowed)"""
    L = _lib.lib()
    R1 = 1 + int(opts.restarts)
    margin = 0.0 if margin is None else float(margin)
    head = (int(rng_seed), int(first_index))
    if isinstance(target_poses, np.ndarray):
        tp = np.ascontiguousarray(target_poses, dtype=np.float64)
        sd = np.ascontiguousarray(seeds, dtype=np.float64)
        T, S = _shape(tp, sd)
        out = {"q": np.empty((T, 14)), "ok": np.empty(T, dtype=np.uint8), "which": np.empty(T, dtype=np.int32), "clearance": np.empty(T)}
        if want_candidates:
            out.update(cand_q=np.empty((T, S, 2, R1, 7)), cand_rounds=np.empty((T, S, 2, R1), dtype=np.int32), cand_clear=np.empty((T, S, 2, R1)),
                       slot_clear=np.empty((T, S)))
        ptr = lambda n, t: out[n].ctypes.data_as(t) if n in out else None  # noqa: E731
        outs = (ptr("q", _dp), ptr("ok", _u8p), ptr("which", _i32p), ptr("cand_q", _dp), ptr("cand_rounds", _i32p), ptr("cand_clear", _dp),
                ptr("slot_clear", _dp), ptr("clearance", _dp))
        args = (C.byref(problem), C.byref(opts), tp.ctypes.data_as(_dp), sd.ctypes.data_as(_dp), T, S) + head
        if isinstance(scene, tuple):
            from .scene import scene_arrays

            check(L.ccmp_pose_ik_vetted_ref(*args, *scene_arrays(*scene), margin, *outs), "ccmp_pose_ik_vetted_ref")
        else:
            check(L.ccmp_pose_ik_vetted_host(ctx_handle, *args, scene._h, margin, *outs), "ccmp_pose_ik_vetted_host")
        return out
    from .constraint import _stream_handle, _torch

    torch = _torch()
    for t in (target_poses, seeds):
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()):
            raise ValueError("expected contiguous float64 tensors on the device")
    T, S = _shape(target_poses, seeds)
    dev = target_poses.device
    out = {"q": torch.empty((T, 14), dtype=torch.float64, device=dev), "ok": torch.empty(T, dtype=torch.uint8, device=dev),
           "which": torch.empty(T, dtype=torch.int32, device=dev), "clearance": torch.empty(T, dtype=torch.float64, device=dev)}
    if want_candidates:
        out["cand_q"] = torch.empty((T, S, 2, R1, 7), dtype=torch.float64, device=dev)
        out["cand_rounds"] = torch.empty((T, S, 2, R1), dtype=torch.int32, device=dev)
        out["cand_clear"] = torch.empty((T, S, 2, R1), dtype=torch.float64, device=dev)
        out["slot_clear"] = torch.empty((T, S), dtype=torch.float64, device=dev)
    ptr = lambda n: out[n].data_ptr() if n in out else None  # noqa: E731
    check(L.ccmp_pose_ik_vetted_batch(ctx_handle, C.byref(problem), C.byref(opts), target_poses.data_ptr(), seeds.data_ptr(), T, S, *head, scene._h, margin,
                                      ptr("q"), ptr("ok"), ptr("which"), ptr("cand_q"), ptr("cand_rounds"), ptr("cand_clear"), ptr("slot_clear"),
                                      ptr("clearance"), _stream_handle(stream)), "ccmp_pose_ik_vetted_batch")
    return out


def pose_ik(ctx_handle, problem, target_poses, seeds, rng_seed=0, first_index=0, opts=None, want_candidates=False, stream=None, ref=False, scene=None,
            margin=None):
    """The three forms behind one signature.  numpy arrays: ccmp_pose_ik_ref (ref=True, no context) or ccmp_pose_ik_host; torch tensors
    on the device: ccmp_pose_ik_batch on `stream`.  Returns a dict: q (T,14), ok (T,) uint8, which (T,) int32 and, with
    want_candidates, cand_q (T,S,2,1+R,7) and cand_rounds (T,S,2,1+R) int32.
    scene (a ProxyScene) and margin (None = 0): the vetted forms, ccmp_pose_ik_vetted_* — the dict also holds clearance (T,) and, with
    want_candidates, cand_clear (T,S,2,1+R) and slot_clear (T,S).  Without a scene the call is the plain one, as before."""
    L = _lib.lib()
    opts = opts if opts is not None else ik_options()
    if scene is not None:
        return _vetted(ctx_handle, problem, target_poses, seeds, rng_seed, first_index, opts, want_candidates, stream, scene, margin)
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


def pose_ik_vetted_ref(problem, target_poses, seeds, spheres, boxes=(), allowed=None, margin=0.0, rng_seed=0, first_index=0, opts=None,
                       want_candidates=False):
    """ccmp_pose_ik_vetted_ref: the vetted rule's text compiled for the host on the caller's scene arrays (ProxyScene's tuples), one
    thread, no device — the same bits as the kernels"""
    return _vetted(None, problem, np.asarray(target_poses, dtype=np.float64), np.asarray(seeds, dtype=np.float64), rng_seed, first_index,
                   opts if opts is not None else ik_options(), want_candidates, None, (list(spheres), list(boxes), allowed), margin)
