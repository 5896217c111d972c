"""Shortcut solution paths (include/ccmp.h: ccmp_path_shortcut, ccmp_shortcut_select; csrc/ccmp_shortcut.h): the removal of interior
vertices from a roadmap path — every pair of waypoints put to one checkMotion in one batch, then the cheapest path over the pairs that
passed.  The call itself is `KinematicChainConstraint.shortcut_paths`; this module holds its body, the selection alone and the two
host-only forms of the rule."""
import ctypes as C

from . import _lib
from ._arrays import HOST
from ._lib import CcmpShortcutOpts, check
from .dense import _path_inputs

__all__ = ["shortcut_select", "shortcut_select_ref", "shortcut_pairs_ref", "SHORTCUT_MAX_LEN"]

SHORTCUT_MAX_LEN = _lib.SHORTCUT_MAX_LEN


def _outputs(K, pj, F, ml):
    # rows behind out_len are not written by the library: they start as the input's rows
    return {"joints": K.copy_of(pj), "out_len": K.zeros(F, "int32"), "kept": K.full((F, ml), "int32", -1), "cost_in": K.zeros(F, "float64"),
            "cost_out": K.zeros(F, "float64")}


def _pair_ok(K, pair_ok, F, ml):
    """pair_ok (F,max_len,max_len) uint8; the host kind takes that many numbers in any shape"""
    return K.expect(pair_ok, "uint8", F * ml * ml if K is HOST else (F, ml, ml), "pair_ok (F,max_len,max_len)")


def _args(K, *arrays):
    """an array of no elements goes as NULL"""
    return [K.arg(a, empty_is_null=True) for a in arrays]


def shortcut_pairs_ref(path_joints, path_len, max_span=0):
    """ccmp_shortcut_pairs_ref: the candidate enumeration alone, on the host, no device: the (f, i, j) triples in order, (n,3) int32"""
    K, pj, pl, F, ml = _path_inputs(None, path_joints, path_len, HOST)
    L = _lib.lib()
    count = C.c_size_t(0)
    check(L.ccmp_shortcut_pairs_ref(*_args(K, pj, pl), F, ml, int(max_span), None, 0, C.byref(count)), "ccmp_shortcut_pairs_ref")
    out = K.zeros((int(count.value), 3), "int32")
    check(L.ccmp_shortcut_pairs_ref(*_args(K, pj, pl), F, ml, int(max_span), *_args(K, out), len(out), C.byref(count)), "ccmp_shortcut_pairs_ref")
    return out


def shortcut_select_ref(path_joints, path_len, pair_ok):
    """ccmp_shortcut_select_ref: the selection alone on a caller's pair_ok (F,max_len,max_len) uint8, on the host, one thread, no device.
    Returns a dict of numpy arrays: joints (F,max_len,14) (the kept rows first; rows behind out_len are the input's), out_len (F,),
    kept (F,max_len), cost_in (F,), cost_out (F,)."""
    K, pj, pl, F, ml = _path_inputs(None, path_joints, path_len, HOST)
    out = _outputs(K, pj, F, ml)
    check(_lib.lib().ccmp_shortcut_select_ref(*_args(K, pj, pl), F, ml, *_args(K, _pair_ok(K, pair_ok, F, ml), *out.values())), "ccmp_shortcut_select_ref")
    return out


def shortcut_select(ctx, path_joints, path_len, pair_ok, stream=None):
    """ccmp_shortcut_select: the selection kernel alone on a caller's pair_ok — any edge test will do, the host's MoveIt verdicts for one.
    Device tensors in, device tensors out, asynchronous on the stream; numpy arrays go through the synchronous host form.  The dict of
    `shortcut_select_ref`."""
    K, pj, pl, F, ml = _path_inputs(ctx, path_joints, path_len)
    ok = _pair_ok(K, pair_ok, F, ml)
    out = _outputs(K, pj, F, ml)
    K.call("ccmp_shortcut_select", "ccmp_shortcut_select_host", ctx.handle, *_args(K, pj, pl), F, ml, *_args(K, ok, *out.values()), stream=stream)
    return out


def shortcut(ctx, problem, path_joints, path_len, scene, margin, max_span, chunk_states, round_budget, max_calls, tile_edges, want_pairs, stream):
    """the body of `KinematicChainConstraint.shortcut_paths`"""
    opts = CcmpShortcutOpts(int(max_span), int(chunk_states), int(round_budget), int(max_calls), int(tile_edges))
    if scene is not None and margin is None:
        raise ValueError("scene needs its margin")
    sc, mg = (scene._h, float(margin)) if scene is not None else (None, 0.0)
    K, pj, pl, F, ml = _path_inputs(ctx, path_joints, path_len)
    out = {**_outputs(K, pj, F, ml), **({"pair_ok": K.zeros((F, ml, ml), "uint8"), "pair_states": K.zeros((F, ml, ml), "int32"),
                                         "pair_newton": K.zeros((F, ml, ml), "int32")} if want_pairs else {})}
    names = ("joints", "out_len", "kept", "cost_in", "cost_out", "pair_ok", "pair_states", "pair_newton")
    K.call("ccmp_path_shortcut", "ccmp_path_shortcut_host", ctx.handle, C.byref(problem), sc, mg, *_args(K, pj, pl), F, ml, C.byref(opts),
           *_args(K, *[out.get(n) for n in names]), stream=stream)
    return out
