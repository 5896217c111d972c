"""Dense solution paths (include/ccmp.h: ccmp_path_densify; csrc/ccmp_dense.h): `PathGeometric::interpolate` as
ConstrainedProblem::solveOnce runs it between the path search and <obj>_path.txt (ConstrainedPlanningCommon.cpp:207-222).  The call
itself is `KinematicChainConstraint.densify_paths`; this module holds its body and the two host-only forms of the rule."""
import ctypes as C

from . import _lib
from ._arrays import HOST, _torch, kind_of
from ._lib import CcmpDenseOpts, check

__all__ = ["dense_layout_ref", "dense_arc_ref", "DENSE_DISTINCT", "DenseHandle"]

DENSE_DISTINCT = _lib.DENSE_DISTINCT


class DenseHandle:
    """A dense result kept where the library made it (ccmp_dense_paths), for `KinematicChainConstraint.resample_paths`: what
    `densify_paths(..., keep_handle=True)` returns under "handle".  close() (or the garbage collector) releases it."""

    def __init__(self, h):
        self._h = h

    def close(self):
        if self._h:
            _lib.lib().ccmp_dense_paths_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _path_inputs(ctx, path_joints, path_len, K=None):
    """What densify, shortcut and smooth take: (kind, path_joints (F,max_len,14), path_len (F,), F, max_len).  Tensors are the device's
    — the context's device — and anything else the host's, where path_len is F numbers in any shape."""
    if K is None:
        K = kind_of(path_joints) if hasattr(path_joints, "data_ptr") else HOST
    pj = K.expect(path_joints, "float64", (None, None, 14), "path_joints (F,max_len,14)")
    F, ml = int(pj.shape[0]), int(pj.shape[1])
    pl = K.expect(path_len, "int32", F if K is HOST else (F,), "path_len (F,)")
    if K is not HOST and K.device.index != ctx.device:
        raise ValueError("tensor is on cuda:%s, context on cuda:%d" % (K.device.index, ctx.device))
    return K, pj, pl, F, ml


def dense_layout_ref(path_len, max_len, seg_states, distinct=False):
    """ccmp_dense_layout_ref: the layout rule alone, on the host, no device.  path_len (F,), seg_states (F, max_len - 1) = the list
    lengths n_i (entries of slots without a segment are not read).  Returns (path_first (F + 1,), seg_first (F, max_len - 1), rows)."""
    pl = HOST.expect(path_len, "int32", -1, "path_len")
    F, ml = len(pl), int(max_len)
    W = max(ml - 1, 0)
    ss = HOST.expect(seg_states, "int32", F * W, "seg_states") if seg_states is not None else None
    path_first, seg_first = HOST.zeros(F + 1, "int32"), HOST.full((F, W), "int32", -1)
    rows = C.c_size_t(0)
    check(_lib.lib().ccmp_dense_layout_ref(HOST.arg(pl), F, ml, HOST.arg(ss, empty_is_null=True), DENSE_DISTINCT if distinct else 0, HOST.arg(path_first),
                                           HOST.arg(seg_first, empty_is_null=True), C.byref(rows)), "ccmp_dense_layout_ref")
    return path_first, seg_first, int(rows.value)


def dense_arc_ref(rows, path_first):
    """ccmp_dense_arc_ref: the arc rule alone, on the host: arc[first] = +0.0, arc[r] = fl(arc[r-1] + joint_distance(row[r-1], row[r]))
    within a path.  Returns (arc (rows,), length (F,))."""
    pf = HOST.expect(path_first, "int32", -1, "path_first")
    F = max(len(pf) - 1, 0)
    r = HOST.expect(rows, "float64", -1, "rows").reshape(-1, 14)
    arc, length = HOST.zeros(len(r), "float64"), HOST.zeros(F, "float64")
    check(_lib.lib().ccmp_dense_arc_ref(HOST.arg(r, empty_is_null=True), HOST.arg(pf), F, HOST.arg(arc, empty_is_null=True),
                                        HOST.arg(length, empty_is_null=True)), "ccmp_dense_arc_ref")
    return arc, length


def densify(ctx, problem, path_joints, path_len, scene, margin, distinct, chunk_states, round_budget, max_calls, stream, keep_handle=False):
    """the body of `KinematicChainConstraint.densify_paths`"""
    opts = CcmpDenseOpts(DENSE_DISTINCT if distinct else 0, int(chunk_states), int(round_budget), int(max_calls))
    if scene is not None and margin is None:
        raise ValueError("scene needs its margin")
    sc, mg = (scene._h, float(margin)) if scene is not None else (None, 0.0)
    h = C.c_void_p()
    K, pj, pl, F, ml = _path_inputs(ctx, path_joints, path_len)
    K.call("ccmp_path_densify", "ccmp_path_densify_host", ctx.handle, C.byref(problem), sc, mg, K.arg(pj) if F else None, K.arg(pl) if F else None, F, ml,
           C.byref(opts), C.byref(h), stream=stream)
    try:
        rows, calls = C.c_size_t(0), C.c_int(0)
        check(_lib.lib().ccmp_dense_paths_info(h, None, None, C.byref(rows), C.byref(calls)), "ccmp_dense_paths_info")
        R, W = int(rows.value), max(ml - 1, 0)
        out = {"joints": K.empty((R, 14), "float64"), "path_first": K.empty((F + 1,), "int32"), "seg_first": K.empty((F, W), "int32"),
               "seg_ok": K.empty((F, W), "uint8"), "seg_newton": K.empty((F, W), "int32"), "arc": K.empty((R,), "float64"), "length": K.empty((F,), "float64"),
               **({"clearance": K.empty((R,), "float64"), "min_clear": K.empty((F,), "float64"), "min_row": K.empty((F,), "int32"),
                   "first_blocked": K.empty((F,), "int32")} if scene is not None else {})}
        names = ("joints", "path_first", "seg_first", "seg_ok", "seg_newton", "arc", "length", "clearance", "min_clear", "min_row", "first_blocked")
        K.call("ccmp_dense_paths_copy", "ccmp_dense_paths_copy_host", h, *[K.arg(out.get(n), empty_is_null=True) for n in names], stream=stream)
        if K is not HOST:  # the handle goes below: its rows must have left it first
            torch = _torch()
            (torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream).synchronize()
        out["rows"] = R
        out["calls"] = int(calls.value)
        if keep_handle:
            out["handle"], h = DenseHandle(h), None  # the result stays with the caller
        return out
    finally:
        if h is not None:
            _lib.lib().ccmp_dense_paths_destroy(h)
