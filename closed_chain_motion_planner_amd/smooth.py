"""Smooth solution paths (include/ccmp.h: ccmp_path_smooth; csrc/ccmp_smooth.h): B-spline passes on the manifold — the structure of
OMPL's PathSimplifier::smoothBSpline with this project's midpoint (the blend at half the arc of a pair's dense list, projected).  The
call itself is `KinematicChainConstraint.smooth_paths`; this module holds its body and the two host-only forms of the rule."""
import ctypes as C

from . import _lib
from ._arrays import HOST
from ._lib import CcmpSmoothOpts, check
from .dense import _path_inputs
from .shortcut import _args

__all__ = ["smooth_mid_ref", "smooth_len_after", "SMOOTH_STATS", "SMOOTH_STOP"]

SMOOTH_STATS = ("projected", "fallback", "degenerate", "refused", "below_min_change")  # the columns of stats
SMOOTH_STOP = ("short", "still", "max_steps", "capacity", "non_finite")  # the values of stop


def smooth_len_after(L, passes):
    """ccmp_smooth_len_after: the vertices of a path of L waypoints after that many passes (each L -> 2L - 1; L < 3 stays)"""
    return int(_lib.lib().ccmp_smooth_len_after(int(L), int(passes)))


def smooth_mid_ref(rows, arcs):
    """ccmp_smooth_mid_ref: the bracket and the blend of one pair's closed list, on the host, no device, no projection: rows (n,14),
    arcs (n,) -> (k, t, blend (14,), fallback row).  A degenerate list (no positive arc) answers (0, 0.0, rows[0], 0)."""
    r = HOST.expect(rows, "float64", (None, 14), "rows (n,14)")
    s = HOST.expect(arcs, "float64", len(r), "arcs (n,)")
    k, fb, t = C.c_int(0), C.c_int(0), C.c_double(0.0)
    blend = HOST.zeros(14, "float64")
    check(_lib.lib().ccmp_smooth_mid_ref(*_args(HOST, r, s), len(r), C.byref(k), C.byref(t), HOST.arg(blend), C.byref(fb)), "ccmp_smooth_mid_ref")
    return k.value, t.value, blend, fb.value


def smooth(ctx, problem, path_joints, path_len, max_steps, min_change, out_max_len, scene, margin, chunk_states, round_budget, max_calls, tile_edges,
           want_stats, stream):
    """the body of `KinematicChainConstraint.smooth_paths`"""
    opts = CcmpSmoothOpts(int(max_steps), float(min_change), int(chunk_states), int(round_budget), int(max_calls), int(tile_edges))
    if scene is not None and margin is None:
        raise ValueError("scene needs its margin")
    sc, mg = (scene._h, float(margin)) if scene is not None else (None, 0.0)
    K, pj, pl, F, ml = _path_inputs(ctx, path_joints, path_len)
    cap = int(out_max_len) if out_max_len is not None else max(smooth_len_after(ml, max(int(max_steps), 0)), ml)
    out = {"joints": K.zeros((F, max(cap, 0), 14), "float64"), **{n: K.zeros(F, "int32") for n in ("out_len", "passes", "moved", "stop")},
           "length_in": K.zeros(F, "float64"), "length_out": K.zeros(F, "float64"), **({"stats": K.zeros((F, 5), "int32")} if want_stats else {})}
    if cap >= ml:
        out["joints"][:, :ml] = pj  # rows behind out_len are not written by the library: they start as the input's rows, zeros behind
    names = ("joints", "out_len", "passes", "moved", "stop", "length_in", "length_out", "stats")
    K.call("ccmp_path_smooth", "ccmp_path_smooth_host", ctx.handle, C.byref(problem), sc, mg, *_args(K, pj, pl), F, ml, C.byref(opts), cap,
           *_args(K, *[out.get(n) for n in names]), stream=stream)
    return out
