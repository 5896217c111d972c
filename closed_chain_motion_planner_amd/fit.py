"""Executing a path, the step between the time stamps and the setpoints (include/ccmp.h: ccmp_path_fit_timestamps; csrc/ccmp_fit.h): the
time-stamp rule bounds its profile at the rows, the setpoints' audit measures what a controller is commanded between them, and this step
closes the loop — it measures the commanded motion at the ticks of the stated period, dilates only the row intervals in which it exceeds
a limit, measures again and repeats until the audit passes.  The call itself is `KinematicChainConstraint.fit_timestamps`; this module
holds its body and the host-only form of the rule.  It is not TOPP-RA, it has no jerk limit, it bounds the motion only at the ticks of the
stated period, and its convergence is observed, not proven: `status` says which paths are fitted."""
import ctypes as C

from . import _lib
from ._arrays import HOST, kind_of
from ._lib import CcmpFitOpts, check
from .retime import _limits
from .setpoints import _inputs
from .shortcut import _args

__all__ = ["fit_timestamps_ref", "FIT_STATUS"]

FIT_STATUS = ("fitted", "empty", "non_finite", "unordered", "point", "full", "passes")  # the values of status
_OUT_ORDER = ("time", "status", "passes", "peak", "duration", "factor")


def _opts(period, max_ticks, aim, max_passes):
    return CcmpFitOpts(float(period), int(max_ticks), float(aim), int(max_passes))


def _outputs(K, t, F, R):
    """time starts as the input's stamps (a row outside every path keeps them), factor as ones"""
    return {"time": K.copy_of(t), "status": K.zeros((F,), "int32"), "passes": K.zeros((F,), "int32"), "peak": K.zeros((F, 2), "float64"),
            "duration": K.zeros((F,), "float64"), "factor": K.full((R,), "float64", 1.0)}


def fit_timestamps_ref(rows, path_first, time, vmax, amax, period=0.001, max_ticks=65536, aim=0.95, max_passes=8):
    """ccmp_path_fit_timestamps_ref: the fit as pure host code, no device: dict(time (R,) the fitted stamps, status (F,) (FIT_STATUS), passes
    (F,), peak (F,2) — speed and acceleration ratios of the last measurement —, duration (F,), factor (R,))"""
    r, pf, t, F, R = _inputs(HOST, rows, path_first, time)
    v, a = _limits(vmax, amax)
    o = _opts(period, max_ticks, aim, max_passes)
    out = _outputs(HOST, t, F, R)
    check(_lib.lib().ccmp_path_fit_timestamps_ref(HOST.arg(r, empty_is_null=True), HOST.arg(pf), HOST.arg(t, empty_is_null=True), F, R, HOST.arg(v), HOST.arg(a),
                                                  C.byref(o), *[HOST.arg(out[n], empty_is_null=True) for n in _OUT_ORDER]), "ccmp_path_fit_timestamps_ref")
    return out


def fit(ctx, rows, path_first, time, vmax, amax, period, max_ticks, aim, max_passes, stream):
    """the body of `KinematicChainConstraint.fit_timestamps`"""
    K = kind_of(rows)
    r, pf, t, F, R = _inputs(K, rows, path_first, time)
    v, a = _limits(vmax, amax)
    o = _opts(period, max_ticks, aim, max_passes)
    out = _outputs(K, t, F, R)
    K.call("ccmp_path_fit_timestamps", "ccmp_path_fit_timestamps_host", ctx.handle, K.arg(r, empty_is_null=True), K.arg(pf), K.arg(t, empty_is_null=True), F, R,
           HOST.arg(v), HOST.arg(a), C.byref(o), *_args(K, *[out[n] for n in _OUT_ORDER]), stream=stream)
    return out
