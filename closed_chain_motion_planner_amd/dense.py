"""Dense solution paths (include/ccmp.h: ccmp_path_densify; csrc/ccmp_dense.h): `PathGeometric::interpolate` as
ConstrainedProblem::solveOnce runs it between the path search and <obj>_path.txt (ConstrainedPlanningCommon.cpp:207-222).  The call
itself is `KinematicChainConstraint.densify_paths`; this module holds its body and the two host-only forms of the rule."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CcmpDenseOpts, check

__all__ = ["dense_layout_ref", "dense_arc_ref", "DENSE_DISTINCT"]

DENSE_DISTINCT = _lib.DENSE_DISTINCT
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None else None


def dense_layout_ref(path_len, max_len, seg_states, distinct=False):
    """ccmp_dense_layout_ref: the layout rule alone, on the host, no device.  path_len (F,), seg_states (F, max_len - 1) = the list
    lengths n_i (entries of slots without a segment are not read).  Returns (path_first (F + 1,), seg_first (F, max_len - 1), rows)."""
    pl = np.ascontiguousarray(path_len, dtype=np.int32).reshape(-1)
    F, ml = len(pl), int(max_len)
    W = max(ml - 1, 0)
    ss = np.ascontiguousarray(seg_states, dtype=np.int32).reshape(F, W) if seg_states is not None else None
    path_first, seg_first = np.zeros(F + 1, dtype=np.int32), np.full((F, W), -1, dtype=np.int32)
    rows = C.c_size_t(0)
    check(_lib.lib().ccmp_dense_layout_ref(_ptr(pl, _i32p), F, ml, _ptr(ss, _i32p) if ss is not None and ss.size else None,
                                           DENSE_DISTINCT if distinct else 0, _ptr(path_first, _i32p), _ptr(seg_first, _i32p) if seg_first.size else None,
                                           C.byref(rows)), "ccmp_dense_layout_ref")
    return path_first, seg_first, int(rows.value)


def dense_arc_ref(rows, path_first):
    """ccmp_dense_arc_ref: the arc rule alone, on the host: arc[first] = +0.0, arc[r] = fl(arc[r-1] + joint_distance(row[r-1], row[r]))
    within a path.  Returns (arc (rows,), length (F,))."""
    pf = np.ascontiguousarray(path_first, dtype=np.int32).reshape(-1)
    F = len(pf) - 1
    r = np.ascontiguousarray(rows, dtype=np.float64).reshape(-1, 14)
    arc, length = np.zeros(len(r)), np.zeros(max(F, 0))
    check(_lib.lib().ccmp_dense_arc_ref(_ptr(r, _dp) if r.size else None, _ptr(pf, _i32p), max(F, 0), _ptr(arc, _dp) if arc.size else None,
                                        _ptr(length, _dp) if length.size else None), "ccmp_dense_arc_ref")
    return arc, length


def densify(ctx, problem, path_joints, path_len, scene, margin, distinct, chunk_states, round_budget, max_calls, stream, torch, stream_handle):
    """the body of `KinematicChainConstraint.densify_paths`"""
    L = _lib.lib()
    opts = CcmpDenseOpts(DENSE_DISTINCT if distinct else 0, int(chunk_states), int(round_budget), int(max_calls))
    if scene is not None and margin is None:
        raise ValueError("scene needs its margin")
    sc, mg = (scene._h, float(margin)) if scene is not None else (None, 0.0)
    h = C.c_void_p()
    on_device = torch is not None and isinstance(path_joints, torch.Tensor)
    if on_device:
        if not (path_joints.is_cuda and path_joints.dtype == torch.float64 and path_joints.dim() == 3 and path_joints.shape[2] == 14
                and path_joints.is_contiguous()):
            raise ValueError("path_joints: a contiguous (F,max_len,14) float64 CUDA tensor")
        F, ml = int(path_joints.shape[0]), int(path_joints.shape[1])
        if not (isinstance(path_len, torch.Tensor) and path_len.is_cuda and path_len.dtype == torch.int32 and path_len.is_contiguous()
                and tuple(path_len.shape) == (F,)):
            raise ValueError("path_len: a contiguous (F,) int32 CUDA tensor")
        if path_joints.device.index != ctx.device:
            raise ValueError("tensor is on cuda:%s, context on cuda:%d" % (path_joints.device.index, ctx.device))
        check(L.ccmp_path_densify(ctx.handle, C.byref(problem), sc, mg, path_joints.data_ptr() if F else None, path_len.data_ptr() if F else None, F, ml,
                                  C.byref(opts), C.byref(h), stream_handle(stream)), "ccmp_path_densify")
    else:
        pj = np.ascontiguousarray(path_joints, dtype=np.float64)
        if pj.ndim != 3 or pj.shape[2] != 14:
            raise ValueError("path_joints: (F,max_len,14)")
        F, ml = pj.shape[0], pj.shape[1]
        pl = np.ascontiguousarray(path_len, dtype=np.int32).reshape(-1)
        if len(pl) != F:
            raise ValueError("path_len: (F,)")
        check(L.ccmp_path_densify_host(ctx.handle, C.byref(problem), sc, mg, _ptr(pj, _dp) if F else None, _ptr(pl, _i32p) if F else None, F, ml,
                                       C.byref(opts), C.byref(h)), "ccmp_path_densify_host")
    try:
        rows, calls = C.c_size_t(0), C.c_int(0)
        check(L.ccmp_dense_paths_info(h, None, None, C.byref(rows), C.byref(calls)), "ccmp_dense_paths_info")
        R, W = int(rows.value), max(ml - 1, 0)
        if on_device:
            dev = path_joints.device
            new = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
            f64, i32, u8 = torch.float64, torch.int32, torch.uint8
        else:
            new = lambda shape, dt: np.empty(shape, dtype=dt)
            f64, i32, u8 = np.float64, np.int32, np.uint8
        out = {"joints": new((R, 14), f64), "path_first": new((F + 1,), i32), "seg_first": new((F, W), i32), "seg_ok": new((F, W), u8),
               "seg_newton": new((F, W), i32), "arc": new((R,), f64), "length": new((F,), f64)}
        if scene is not None:
            out.update(clearance=new((R,), f64), min_clear=new((F,), f64), min_row=new((F,), i32), first_blocked=new((F,), i32))
        names = ("joints", "path_first", "seg_first", "seg_ok", "seg_newton", "arc", "length", "clearance", "min_clear", "min_row", "first_blocked")
        if on_device:
            args = [out[k].data_ptr() if k in out and out[k].numel() else None for k in names]
            check(L.ccmp_dense_paths_copy(h, *args, stream_handle(stream)), "ccmp_dense_paths_copy")
            # the handle goes below: its rows must have left it first
            (torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream).synchronize()
        else:
            types = (_dp, _i32p, _i32p, _u8p, _i32p, _dp, _dp, _dp, _dp, _i32p, _i32p)
            args = [_ptr(out[k], t) if k in out and out[k].size else None for k, t in zip(names, types)]
            check(L.ccmp_dense_paths_copy_host(h, *args), "ccmp_dense_paths_copy_host")
        out["rows"] = R
        out["calls"] = int(calls.value)
        return out
    finally:
        L.ccmp_dense_paths_destroy(h)
