"""Executing a path, the last step (include/ccmp.h: ccmp_path_setpoints; csrc/ccmp_setpoints.h): packed rows with one time per row — what
`KinematicChainConstraint.timestamp_paths` ends at — turned into what a controller is commanded at every tick of its period, and an audit of
that motion between the rows: speed and acceleration against the limits, the constraint gap, the clearance.  The reference hands
positions-only points to its trajectory controller (scripts/execute_path.py:96-110).  The call itself is
`KinematicChainConstraint.setpoint_paths`; this module holds its body and the host-only forms of the rule.  Setpoints are not projected:
the knob for the gap is the resample spacing, and the audit says whether it is fine enough."""
import ctypes as C

from . import _lib
from ._arrays import HOST, _torch, kind_of
from ._lib import CcmpSetpointOpts, check
from .retime import _limits, _stamp_inputs
from .shortcut import _args

__all__ = ["setpoints_ref", "setpoint_tangents_ref", "SETPOINT_STATUS", "SETPOINT_PEAKS"]

SETPOINT_STATUS = ("ok", "empty", "non_finite", "unordered", "point", "full")  # the values of status
SETPOINT_PEAKS = ("speed", "acceleration", "dp", "angle", "clearance")  # the columns of peak and peak_tick


def _opts(period, max_ticks):
    return CcmpSetpointOpts(float(period), int(max_ticks))


def _inputs(K, rows, path_first, time):
    r, pf, F, R = _stamp_inputs(K, rows, path_first)
    t = K.expect(time, "float64", R if K is HOST else (R,), "time (R,)")
    return r, pf, t, F, R


def setpoint_tangents_ref(rows, time):
    """ccmp_setpoint_tangents_ref: the PCHIP (Fritsch-Butland) tangents of ONE path on the host, no device: rows (R,14), time (R,) -> (R,14),
    zero at both ends and wherever the slopes on either side do not share a sign"""
    r = HOST.expect(rows, "float64", (None, 14), "rows (R,14)")
    t = HOST.expect(time, "float64", len(r), "time (R,)")
    w = HOST.zeros((len(r), 14), "float64")
    check(_lib.lib().ccmp_setpoint_tangents_ref(*_args(HOST, r, t), len(r), *_args(HOST, w)), "ccmp_setpoint_tangents_ref")
    return w


def setpoints_ref(rows, path_first, time, vmax, amax, period=0.001, max_ticks=65536):
    """ccmp_setpoints_ref: the interpolation and the speed and acceleration audit as pure host code, no device, by its two calls (sizes,
    then arrays): dict(q, qd (ticks,14), tau (ticks,), tick_first (F+1,), status (F,), peak (F,2), peak_tick (F,2) — speed, acceleration —,
    stretch (F,), ticks).  The gap f and the clearance are other units' rules and not part of it."""
    r, pf, t, F, R = _inputs(HOST, rows, path_first, time)
    v, a = _limits(vmax, amax)
    o = _opts(period, max_ticks)
    out = {"tick_first": HOST.zeros(F + 1, "int32"), "status": HOST.zeros(F, "int32")}
    head = (HOST.arg(r, empty_is_null=True), HOST.arg(pf), HOST.arg(t, empty_is_null=True), F, R, HOST.arg(v), HOST.arg(a), C.byref(o))
    check(_lib.lib().ccmp_setpoints_ref(*head, HOST.arg(out["tick_first"]), HOST.arg(out["status"], empty_is_null=True), None, None, None, None, None, None),
          "ccmp_setpoints_ref")
    M = int(out["tick_first"][F])
    out.update(q=HOST.zeros((M, 14), "float64"), qd=HOST.zeros((M, 14), "float64"), tau=HOST.zeros(M, "float64"), peak=HOST.zeros((F, 2), "float64"),
               peak_tick=HOST.zeros((F, 2), "int32"), stretch=HOST.zeros(F, "float64"))
    check(_lib.lib().ccmp_setpoints_ref(*head, HOST.arg(out["tick_first"]), *_args(HOST, out["status"], out["q"], out["qd"], out["tau"], out["peak"],
                                                                                     out["peak_tick"], out["stretch"])), "ccmp_setpoints_ref")
    out["ticks"] = M
    return out


def _collect(K, h, prefix, arrays, stream):
    """what follows a call that answered with the result handle h of the C type `prefix` (this unit's and the jerk unit's): its info, the
    arrays allocated by name — arrays(ticks) -> {name: (shape, dtype)} in the order `prefix`_copy takes them —, copied, the stream waited
    for, and the handle destroyed whatever happened"""
    try:
        nF, ticks = C.c_size_t(0), C.c_size_t(0)
        check(getattr(_lib.lib(), prefix + "_info")(h, C.byref(nF), C.byref(ticks)), prefix + "_info")
        M = int(ticks.value)
        out = {n: K.empty(shape, dtype) for n, (shape, dtype) in arrays(M).items()}
        K.call(prefix + "_copy", prefix + "_copy_host", h, *_args(K, *out.values()), stream=stream)
        if K is not HOST:  # the handle goes below: its arrays must have left it first
            torch = _torch()
            (torch.cuda.current_stream() if stream is None else torch.cuda.ExternalStream(stream) if isinstance(stream, int) else stream).synchronize()
        out["ticks"] = M
        return out
    finally:
        getattr(_lib.lib(), prefix + "_destroy")(h)


def setpoints(ctx, problem, rows, path_first, time, vmax, amax, period, max_ticks, scene, margin, stream):
    """the body of `KinematicChainConstraint.setpoint_paths`"""
    K = kind_of(rows)
    r, pf, t, F, R = _inputs(K, rows, path_first, time)
    v, a = _limits(vmax, amax)
    o = _opts(period, max_ticks)
    h = C.c_void_p()
    K.call("ccmp_path_setpoints", "ccmp_path_setpoints_host", ctx.handle, C.byref(problem), scene._h if scene is not None else None, float(margin),
           K.arg(r, empty_is_null=True), K.arg(pf), K.arg(t, empty_is_null=True), F, R, HOST.arg(v), HOST.arg(a), C.byref(o), C.byref(h), stream=stream)
    return _collect(K, h, "ccmp_setpoints", lambda M: {
        "q": ((M, 14), "float64"), "qd": ((M, 14), "float64"), "tau": ((M,), "float64"), "tick_first": ((F + 1,), "int32"), "f": ((M, 2), "float64"),
        "satisfied": ((M,), "uint8"), "clearance": ((M,), "float64"), "status": ((F,), "int32"), "peak": ((F, 5), "float64"), "peak_tick": ((F, 5), "int32"),
        "counts": ((F, 2), "int32"), "stretch": ((F,), "float64")}, stream)
