"""Executing a path (include/ccmp.h: ccmp_path_resample, ccmp_path_timestamps; csrc/ccmp_retime.h): a dense path resampled at even
arc — `PathGeometric::interpolate(count)` with this project's blend — and time stamps under joint velocity and acceleration limits, in
place of the reference's "same time slice for every printed row" (scripts/execute_path.py:105-108).  The calls themselves are
`KinematicChainConstraint.resample_paths` and `.timestamp_paths`; this module holds their bodies, the host-only forms of the rule and
the Panda's limits."""
import ctypes as C

from . import _lib
from ._arrays import HOST, _stream_handle, _torch, kind_of
from ._lib import CcmpResampleOpts, check
from .shortcut import _args

__all__ = ["timestamps_ref", "arc_bracket_ref", "resample_targets_ref", "RETIME_STATUS", "SAMPLE_KINDS", "PANDA_VELOCITY_LIMITS",
           "PANDA_ACCELERATION_LIMITS", "PANDA_JERK_LIMITS"]

RETIME_STATUS = ("ok", "empty", "broken", "non_finite", "point", "full")  # the values of status
SAMPLE_KINDS = ("projected", "fallback", "degenerate", "copied")  # the values of kind, the columns of counts

# the robot's data sheet; the reference holds no limits.  Per arm, rad/s, rad/s^2 and rad/s^3; a call takes 14 numbers: the tuple twice
PANDA_VELOCITY_LIMITS = (2.175,) * 4 + (2.61,) * 3
PANDA_ACCELERATION_LIMITS = (15.0, 7.5, 10.0, 12.5, 15.0, 20.0, 20.0)
PANDA_JERK_LIMITS = (7500.0, 3750.0, 5000.0, 6250.0, 7500.0, 10000.0, 10000.0)


def _limits(vmax, amax):
    return HOST.expect(vmax, "float64", 14, "vmax (14,)"), HOST.expect(amax, "float64", 14, "amax (14,)")


def arc_bracket_ref(arcs, h):
    """ccmp_arc_bracket_ref: the bracket of the target arc h on monotone arcs (n,), 0 < h <= arcs[-1], on the host: (k, t, lower) with k
    the smallest k >= 1 with arcs[k] >= h, t = (h - arcs[k-1]) / (arcs[k] - arcs[k-1]), lower = (h - arcs[k-1]) <= (arcs[k] - h)"""
    s = HOST.expect(arcs, "float64", -1, "arcs (n,)")
    k, lower, t = C.c_int(0), C.c_int(0), C.c_double(0.0)
    check(_lib.lib().ccmp_arc_bracket_ref(HOST.arg(s, empty_is_null=True), len(s), float(h), C.byref(k), C.byref(t), C.byref(lower)), "ccmp_arc_bracket_ref")
    return k.value, t.value, bool(lower.value)


def resample_targets_ref(T, count=0, spacing=0.0, max_rows=65536):
    """ccmp_resample_targets_ref: the rows a path of length T gets and their target arcs, on the host: (N, h (N,)) — N = 1 when not
    T > 0, 0 when the path would be over max_rows; h = +0.0, the interior targets, T"""
    n = C.c_int(0)
    args = (float(T), int(count), float(spacing), int(max_rows))
    check(_lib.lib().ccmp_resample_targets_ref(*args, C.byref(n), None), "ccmp_resample_targets_ref")
    h = HOST.zeros(n.value, "float64")
    check(_lib.lib().ccmp_resample_targets_ref(*args, C.byref(n), HOST.arg(h, empty_is_null=True)), "ccmp_resample_targets_ref")
    return n.value, h


def _stamp_inputs(K, rows, path_first):
    r = K.expect(rows, "float64", (None, 14), "rows (R,14)")
    pf = K.expect(path_first, "int32", -1 if K is HOST else (None,), "path_first (F+1,)")
    if len(pf) < 1:
        raise ValueError("path_first: at least one entry")
    return r, pf, len(pf) - 1, int(r.shape[0])


def timestamps_ref(rows, path_first, vmax, amax, beta=0.5):
    """ccmp_path_timestamps_ref: the time-stamp rule as pure host code, no device: rows (R,14), path_first (F+1,) -> dict(time,
    ceiling, envelope (R,), duration (F,), status (F,)); rows of a path that is not OK keep NaN"""
    r, pf, F, R = _stamp_inputs(HOST, rows, path_first)
    v, a = _limits(vmax, amax)
    out = {"time": HOST.full(R, "float64", float("nan")), "duration": HOST.zeros(F, "float64"), "ceiling": HOST.full(R, "float64", float("nan")),
           "envelope": HOST.full(R, "float64", float("nan")), "status": HOST.zeros(F, "int32")}
    check(_lib.lib().ccmp_path_timestamps_ref(HOST.arg(r, empty_is_null=True), HOST.arg(pf), F, R, HOST.arg(v), HOST.arg(a), float(beta),
                                              *_args(HOST, out["time"], out["duration"], out["ceiling"], out["envelope"], out["status"])), "ccmp_path_timestamps_ref")
    return out


def timestamps(ctx, rows, path_first, vmax, amax, beta, profile, stream):
    """the body of `KinematicChainConstraint.timestamp_paths`"""
    K = kind_of(rows)
    r, pf, F, R = _stamp_inputs(K, rows, path_first)
    v, a = _limits(vmax, amax)
    out = {"time": K.zeros(R, "float64"), "duration": K.zeros(F, "float64"),
           **({"ceiling": K.zeros(R, "float64"), "envelope": K.zeros(R, "float64")} if profile else {}), "status": K.zeros(F, "int32")}
    K.call("ccmp_path_timestamps", "ccmp_path_timestamps_host", ctx.handle, K.arg(r, empty_is_null=True), K.arg(pf), F, R, HOST.arg(v), HOST.arg(a), float(beta),
           *_args(K, out["time"], out["duration"], out.get("ceiling"), out.get("envelope"), out["status"]), stream=stream)
    return out


def resample(ctx, problem, dense, count, spacing, max_rows, stream):
    """the body of `KinematicChainConstraint.resample_paths`"""
    handle = dense.get("handle") if isinstance(dense, dict) else dense
    if handle is None or not getattr(handle, "_h", None):
        raise ValueError("resample_paths takes the result of densify_paths(..., keep_handle=True) with its handle open")
    K = kind_of(dense["joints"]) if isinstance(dense, dict) else HOST
    opts = CcmpResampleOpts()
    _lib.lib().ccmp_resample_opts_default(C.byref(problem), C.byref(opts))
    if count is not None:
        opts.count = int(count)
    if spacing is not None:
        opts.spacing = float(spacing)
    opts.max_rows = int(max_rows)
    h = C.c_void_p()
    check(_lib.lib().ccmp_path_resample(ctx.handle, C.byref(problem), handle._h, C.byref(opts), C.byref(h), None if K is HOST else _stream_handle(stream)),
          "ccmp_path_resample")
    try:
        F, rows = C.c_size_t(0), C.c_size_t(0)
        check(_lib.lib().ccmp_sampled_paths_info(h, C.byref(F), C.byref(rows)), "ccmp_sampled_paths_info")
        F, R = int(F.value), int(rows.value)
        out = {"joints": K.empty((R, 14), "float64"), "path_first": K.empty((F + 1,), "int32"), "arc": K.empty((R,), "float64"), "length": K.empty((F,), "float64"),
               "kind": K.empty((R,), "uint8"), "status": K.empty((F,), "int32"), "counts": K.empty((F, 4), "int32")}
        K.call("ccmp_sampled_paths_copy", "ccmp_sampled_paths_copy_host", h, *_args(K, *out.values()), stream=stream)
        if K is not HOST:  # the handle goes below: its rows must have left it first
            torch = _torch()
            (torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream).synchronize()
        out["rows"] = R
        return out
    finally:
        _lib.lib().ccmp_sampled_paths_destroy(h)
