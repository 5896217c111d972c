"""Smooth solution paths (include/ccmp.h: ccmp_path_smooth; csrc/ccmp_smooth.h): B-spline passes on the manifold — the structure of
OMPL's PathSimplifier::smoothBSpline with this project's midpoint (the blend at half the arc of a pair's dense list, projected).  The
call itself is `KinematicChainConstraint.smooth_paths`; this module holds its body and the two host-only forms of the rule."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CcmpSmoothOpts, check
from .shortcut import _device_inputs, _dp, _host_inputs, _i32p, _ptr

__all__ = ["smooth_mid_ref", "smooth_len_after", "SMOOTH_STATS", "SMOOTH_STOP"]

SMOOTH_STATS = ("projected", "fallback", "degenerate", "refused", "below_min_change")  # the columns of stats
SMOOTH_STOP = ("short", "still", "max_steps", "capacity", "non_finite")  # the values of stop


def smooth_len_after(L, passes):
    """ccmp_smooth_len_after: the vertices of a path of L waypoints after that many passes (each L -> 2L - 1; L < 3 stays)"""
    return int(_lib.lib().ccmp_smooth_len_after(int(L), int(passes)))


def smooth_mid_ref(rows, arcs):
    """ccmp_smooth_mid_ref: the bracket and the blend of one pair's closed list, on the host, no device, no projection: rows (n,14),
    arcs (n,) -> (k, t, blend (14,), fallback row).  A degenerate list (no positive arc) answers (0, 0.0, rows[0], 0)."""
    r = np.ascontiguousarray(rows, dtype=np.float64)
    s = np.ascontiguousarray(arcs, dtype=np.float64).reshape(-1)
    if r.ndim != 2 or r.shape[1] != 14 or len(s) != len(r):
        raise ValueError("rows: (n,14), arcs: (n,)")
    k, fb, t = C.c_int(0), C.c_int(0), C.c_double(0.0)
    blend = np.zeros(14)
    check(_lib.lib().ccmp_smooth_mid_ref(_ptr(r, _dp), _ptr(s, _dp), len(r), C.byref(k), C.byref(t), _ptr(blend, _dp), C.byref(fb)), "ccmp_smooth_mid_ref")
    return k.value, t.value, blend, fb.value


def smooth(ctx, problem, path_joints, path_len, max_steps, min_change, out_max_len, scene, margin, chunk_states, round_budget, max_calls, tile_edges,
           want_stats, stream, torch, stream_handle):
    """the body of `KinematicChainConstraint.smooth_paths`"""
    L = _lib.lib()
    opts = CcmpSmoothOpts(int(max_steps), float(min_change), int(chunk_states), int(round_budget), int(max_calls), int(tile_edges))
    if scene is not None and margin is None:
        raise ValueError("scene needs its margin")
    sc, mg = (scene._h, float(margin)) if scene is not None else (None, 0.0)
    names = ("joints", "out_len", "passes", "moved", "stop", "length_in", "length_out", "stats")
    if torch is not None and isinstance(path_joints, torch.Tensor):
        F, ml = _device_inputs(torch, ctx, path_joints, path_len)
        cap = int(out_max_len) if out_max_len is not None else max(smooth_len_after(ml, max(int(max_steps), 0)), ml)
        dev = path_joints.device
        out = {"joints": torch.zeros((F, max(cap, 0), 14), dtype=torch.float64, device=dev)}
        if cap >= ml:
            out["joints"][:, :ml] = path_joints  # rows behind out_len are not written by the library: they start as the input's rows, zeros behind
        for k in names[1:5]:
            out[k] = torch.zeros(F, dtype=torch.int32, device=dev)
        for k in names[5:7]:
            out[k] = torch.zeros(F, dtype=torch.float64, device=dev)
        if want_stats:
            out["stats"] = torch.zeros((F, 5), dtype=torch.int32, device=dev)
        args = [out[k].data_ptr() if k in out and F else None for k in names]
        check(L.ccmp_path_smooth(ctx.handle, C.byref(problem), sc, mg, path_joints.data_ptr() if F else None, path_len.data_ptr() if F else None, F, ml,
                                 C.byref(opts), cap, *args, stream_handle(stream)), "ccmp_path_smooth")
        return out
    pj, pl, F, ml = _host_inputs(path_joints, path_len)
    cap = int(out_max_len) if out_max_len is not None else max(smooth_len_after(ml, max(int(max_steps), 0)), ml)
    out = {"joints": np.zeros((F, max(cap, 0), 14))}
    if cap >= ml:
        out["joints"][:, :ml] = pj
    for k in names[1:5]:
        out[k] = np.zeros(F, dtype=np.int32)
    for k in names[5:7]:
        out[k] = np.zeros(F)
    if want_stats:
        out["stats"] = np.zeros((F, 5), dtype=np.int32)
    check(L.ccmp_path_smooth_host(ctx.handle, C.byref(problem), sc, mg, _ptr(pj, _dp), _ptr(pl, _i32p), F, ml, C.byref(opts), cap, _ptr(out["joints"], _dp),
                                  _ptr(out["out_len"], _i32p), _ptr(out["passes"], _i32p), _ptr(out["moved"], _i32p), _ptr(out["stop"], _i32p),
                                  _ptr(out["length_in"], _dp), _ptr(out["length_out"], _dp), _ptr(out.get("stats"), _i32p)), "ccmp_path_smooth_host")
    return out
