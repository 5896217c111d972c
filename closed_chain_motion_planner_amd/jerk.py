"""Executing a path on a robot that limits jerk (include/ccmp.h: ccmp_path_jerk_setpoints; csrc/ccmp_jerk.h): the setpoints of
`KinematicChainConstraint.setpoint_paths` are a C1 piecewise cubic whose acceleration jumps at every row; this unit delivers a moving
average of W consecutive ticks of that interpolant, measures jerk at the controller's rate and chooses W per path.  The call itself is
`KinematicChainConstraint.jerk_setpoint_paths`; this module holds its body and the host-only form of the rule.  By construction the speed
and acceleration peaks cannot rise and the jerk is at most 2 A / (W period).  It is a bound at the ticks of the stated period on the qd
sequence, not a third difference of positions; the filtered ticks lag by (W - 1) / 2 ticks and cut corners (the gap, isSatisfied and
clearance figures of the same call say whether that matters); it is not a jerk-optimal profile."""
import ctypes as C

from . import _lib
from ._arrays import HOST, kind_of
from ._lib import CcmpJerkOpts, check
from .retime import _limits
from .setpoints import _collect, _inputs
from .shortcut import _args

__all__ = ["jerk_setpoints_ref", "jerk_next_window_ref", "JERK_STATUS", "JERK_PEAKS"]

JERK_STATUS = ("ok", "empty", "non_finite", "unordered", "point", "full", "window")  # the values of status
JERK_PEAKS = ("speed", "acceleration", "jerk", "dp", "angle", "clearance")  # the columns of peak and peak_tick


def _opts(period, max_ticks, window, max_window, aim, tile_ticks):
    return CcmpJerkOpts(float(period), int(max_ticks), int(window), int(max_window), float(aim), int(tile_ticks))


def _jmax(jmax):
    return HOST.expect(jmax, "float64", 14, "jmax (14,)")


def jerk_setpoints_ref(rows, path_first, time, vmax, amax, jmax, period=0.001, max_ticks=65536, window=0, max_window=64, aim=0.95):
    """ccmp_jerk_setpoints_ref: the rule and the speed, acceleration and jerk audit as pure host code, no device, by its two calls (sizes,
    then arrays): dict(q, qd (ticks,14), tau (ticks,), tick_first (F+1,), status (F,) (JERK_STATUS), window (F,), passes (F,), peak (F,3),
    peak_tick (F,3) — speed, acceleration, jerk —, ticks).  The gap f and the clearance are other units' rules and not part of it."""
    r, pf, t, F, R = _inputs(HOST, rows, path_first, time)
    v, a = _limits(vmax, amax)
    j = _jmax(jmax)
    o = _opts(period, max_ticks, window, max_window, aim, 0)
    out = {"tick_first": HOST.zeros(F + 1, "int32"), "status": HOST.zeros(F, "int32"), "window": HOST.zeros(F, "int32"), "passes": HOST.zeros(F, "int32")}
    head = (HOST.arg(r, empty_is_null=True), HOST.arg(pf), HOST.arg(t, empty_is_null=True), F, R, HOST.arg(v), HOST.arg(a), HOST.arg(j), C.byref(o),
            HOST.arg(out["tick_first"]), *[HOST.arg(out[n], empty_is_null=True) for n in ("status", "window", "passes")])
    check(_lib.lib().ccmp_jerk_setpoints_ref(*head, None, None, None, None, None), "ccmp_jerk_setpoints_ref")
    M = int(out["tick_first"][F])
    out.update(q=HOST.zeros((M, 14), "float64"), qd=HOST.zeros((M, 14), "float64"), tau=HOST.zeros(M, "float64"), peak=HOST.zeros((F, 3), "float64"),
               peak_tick=HOST.zeros((F, 3), "int32"))
    check(_lib.lib().ccmp_jerk_setpoints_ref(*head, *_args(HOST, out["q"], out["qd"], out["tau"], out["peak"], out["peak_tick"])), "ccmp_jerk_setpoints_ref")
    out["ticks"] = M
    return out


def jerk_next_window_ref(W, P, aim=0.95, max_window=64):
    """ccmp_jerk_next_window_ref: the window that follows W < max_window when the jerk ratio P was measured for it"""
    nxt = C.c_int(0)
    check(_lib.lib().ccmp_jerk_next_window_ref(int(W), float(P), float(aim), int(max_window), C.byref(nxt)), "ccmp_jerk_next_window_ref")
    return nxt.value


def jerk_setpoints(ctx, problem, rows, path_first, time, vmax, amax, jmax, period, max_ticks, window, max_window, aim, tile_ticks, scene, margin, stream):
    """the body of `KinematicChainConstraint.jerk_setpoint_paths`"""
    K = kind_of(rows)
    r, pf, t, F, R = _inputs(K, rows, path_first, time)
    v, a = _limits(vmax, amax)
    j = _jmax(jmax)
    o = _opts(period, max_ticks, window, max_window, aim, tile_ticks)
    h = C.c_void_p()
    K.call("ccmp_path_jerk_setpoints", "ccmp_path_jerk_setpoints_host", ctx.handle, C.byref(problem), scene._h if scene is not None else None, float(margin),
           K.arg(r, empty_is_null=True), K.arg(pf), K.arg(t, empty_is_null=True), F, R, HOST.arg(v), HOST.arg(a), HOST.arg(j), C.byref(o), C.byref(h),
           stream=stream)
    return _collect(K, h, "ccmp_jerk_setpoints", lambda M: {
        "q": ((M, 14), "float64"), "qd": ((M, 14), "float64"), "tau": ((M,), "float64"), "tick_first": ((F + 1,), "int32"), "f": ((M, 2), "float64"),
        "satisfied": ((M,), "uint8"), "clearance": ((M,), "float64"), "status": ((F,), "int32"), "window": ((F,), "int32"), "passes": ((F,), "int32"),
        "peak": ((F, 6), "float64"), "peak_tick": ((F, 6), "int32"), "counts": ((F, 2), "int32")}, stream)
