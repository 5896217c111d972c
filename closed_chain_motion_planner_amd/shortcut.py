"""Shortcut solution paths (include/ccmp.h: ccmp_path_shortcut, ccmp_shortcut_select; csrc/ccmp_shortcut.h): the removal of interior
vertices from a roadmap path — every pair of waypoints put to one checkMotion in one batch, then the cheapest path over the pairs that
passed.  The call itself is `KinematicChainConstraint.shortcut_paths`; this module holds its body, the selection alone and the two
host-only forms of the rule."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import CcmpShortcutOpts, check

__all__ = ["shortcut_select", "shortcut_select_ref", "shortcut_pairs_ref", "SHORTCUT_MAX_LEN"]

SHORTCUT_MAX_LEN = _lib.SHORTCUT_MAX_LEN
_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


def _ptr(a, typ):
    return a.ctypes.data_as(typ) if a is not None and a.size else None


def _host_inputs(path_joints, path_len):
    pj = np.ascontiguousarray(path_joints, dtype=np.float64)
    if pj.ndim != 3 or pj.shape[2] != 14:
        raise ValueError("path_joints: (F,max_len,14)")
    pl = np.ascontiguousarray(path_len, dtype=np.int32).reshape(-1)
    if len(pl) != pj.shape[0]:
        raise ValueError("path_len: (F,)")
    return pj, pl, pj.shape[0], pj.shape[1]


def _host_outputs(pj, F, ml):
    # rows behind out_len are not written by the library: they start as the input's rows
    return {"joints": pj.copy(), "out_len": np.zeros(F, dtype=np.int32), "kept": np.full((F, ml), -1, dtype=np.int32), "cost_in": np.zeros(F),
            "cost_out": np.zeros(F)}


def _device_inputs(torch, ctx, path_joints, path_len):
    if not (path_joints.is_cuda and path_joints.dtype == torch.float64 and path_joints.dim() == 3 and path_joints.shape[2] == 14
            and path_joints.is_contiguous()):
        raise ValueError("path_joints: a contiguous (F,max_len,14) float64 CUDA tensor")
    F, ml = int(path_joints.shape[0]), int(path_joints.shape[1])
    if not (isinstance(path_len, torch.Tensor) and path_len.is_cuda and path_len.dtype == torch.int32 and path_len.is_contiguous()
            and tuple(path_len.shape) == (F,)):
        raise ValueError("path_len: a contiguous (F,) int32 CUDA tensor")
    if path_joints.device.index != ctx.device:
        raise ValueError("tensor is on cuda:%s, context on cuda:%d" % (path_joints.device.index, ctx.device))
    return F, ml


def _device_outputs(torch, path_joints, F, ml):
    dev = path_joints.device
    return {"joints": path_joints.clone(), "out_len": torch.zeros(F, dtype=torch.int32, device=dev),
            "kept": torch.full((F, ml), -1, dtype=torch.int32, device=dev), "cost_in": torch.zeros(F, dtype=torch.float64, device=dev),
            "cost_out": torch.zeros(F, dtype=torch.float64, device=dev)}


def shortcut_pairs_ref(path_joints, path_len, max_span=0):
    """ccmp_shortcut_pairs_ref: the candidate enumeration alone, on the host, no device: the (f, i, j) triples in order, (n,3) int32"""
    pj, pl, F, ml = _host_inputs(path_joints, path_len)
    L = _lib.lib()
    count = C.c_size_t(0)
    check(L.ccmp_shortcut_pairs_ref(_ptr(pj, _dp), _ptr(pl, _i32p), F, ml, int(max_span), None, 0, C.byref(count)), "ccmp_shortcut_pairs_ref")
    out = np.zeros((int(count.value), 3), dtype=np.int32)
    check(L.ccmp_shortcut_pairs_ref(_ptr(pj, _dp), _ptr(pl, _i32p), F, ml, int(max_span), _ptr(out, _i32p), len(out), C.byref(count)),
          "ccmp_shortcut_pairs_ref")
    return out


def shortcut_select_ref(path_joints, path_len, pair_ok):
    """ccmp_shortcut_select_ref: the selection alone on a caller's pair_ok (F,max_len,max_len) uint8, on the host, one thread, no device.
    Returns a dict of numpy arrays: joints (F,max_len,14) (the kept rows first; rows behind out_len are the input's), out_len (F,),
    kept (F,max_len), cost_in (F,), cost_out (F,)."""
    pj, pl, F, ml = _host_inputs(path_joints, path_len)
    ok = np.ascontiguousarray(pair_ok, dtype=np.uint8).reshape(F, ml, ml)
    out = _host_outputs(pj, F, ml)
    check(_lib.lib().ccmp_shortcut_select_ref(_ptr(pj, _dp), _ptr(pl, _i32p), F, ml, _ptr(ok, _u8p), _ptr(out["joints"], _dp), _ptr(out["out_len"], _i32p),
                                              _ptr(out["kept"], _i32p), _ptr(out["cost_in"], _dp), _ptr(out["cost_out"], _dp)), "ccmp_shortcut_select_ref")
    return out


def shortcut_select(ctx, path_joints, path_len, pair_ok, stream=None):
    """ccmp_shortcut_select: the selection kernel alone on a caller's pair_ok — any edge test will do, the host's MoveIt verdicts for one.
    Device tensors in, device tensors out, asynchronous on the stream; numpy arrays go through the synchronous host form.  The dict of
    `shortcut_select_ref`."""
    from .constraint import _stream_handle, _torch

    torch = _torch()
    L = _lib.lib()
    if torch is not None and isinstance(path_joints, torch.Tensor):
        F, ml = _device_inputs(torch, ctx, path_joints, path_len)
        if not (isinstance(pair_ok, torch.Tensor) and pair_ok.is_cuda and pair_ok.dtype == torch.uint8 and pair_ok.is_contiguous()
                and tuple(pair_ok.shape) == (F, ml, ml)):
            raise ValueError("pair_ok: a contiguous (F,max_len,max_len) uint8 CUDA tensor")
        out = _device_outputs(torch, path_joints, F, ml)
        check(L.ccmp_shortcut_select(ctx.handle, path_joints.data_ptr() if F else None, path_len.data_ptr() if F else None, F, ml,
                                     pair_ok.data_ptr() if F else None, out["joints"].data_ptr() if F else None, out["out_len"].data_ptr() if F else None,
                                     out["kept"].data_ptr() if F else None, out["cost_in"].data_ptr() if F else None,
                                     out["cost_out"].data_ptr() if F else None, _stream_handle(stream)), "ccmp_shortcut_select")
        return out
    pj, pl, F, ml = _host_inputs(path_joints, path_len)
    ok = np.ascontiguousarray(pair_ok, dtype=np.uint8).reshape(F, ml, ml)
    out = _host_outputs(pj, F, ml)
    check(L.ccmp_shortcut_select_host(ctx.handle, _ptr(pj, _dp), _ptr(pl, _i32p), F, ml, _ptr(ok, _u8p), _ptr(out["joints"], _dp), _ptr(out["out_len"], _i32p),
                                      _ptr(out["kept"], _i32p), _ptr(out["cost_in"], _dp), _ptr(out["cost_out"], _dp)), "ccmp_shortcut_select_host")
    return out


def shortcut(ctx, problem, path_joints, path_len, scene, margin, max_span, chunk_states, round_budget, max_calls, tile_edges, want_pairs, stream, torch,
             stream_handle):
    """the body of `KinematicChainConstraint.shortcut_paths`"""
    L = _lib.lib()
    opts = CcmpShortcutOpts(int(max_span), int(chunk_states), int(round_budget), int(max_calls), int(tile_edges))
    if scene is not None and margin is None:
        raise ValueError("scene needs its margin")
    sc, mg = (scene._h, float(margin)) if scene is not None else (None, 0.0)
    if torch is not None and isinstance(path_joints, torch.Tensor):
        F, ml = _device_inputs(torch, ctx, path_joints, path_len)
        out = _device_outputs(torch, path_joints, F, ml)
        if want_pairs:
            dev = path_joints.device
            out.update(pair_ok=torch.zeros((F, ml, ml), dtype=torch.uint8, device=dev), pair_states=torch.zeros((F, ml, ml), dtype=torch.int32, device=dev),
                       pair_newton=torch.zeros((F, ml, ml), dtype=torch.int32, device=dev))
        names = ("joints", "out_len", "kept", "cost_in", "cost_out", "pair_ok", "pair_states", "pair_newton")
        args = [out[k].data_ptr() if k in out and F else None for k in names]
        check(L.ccmp_path_shortcut(ctx.handle, C.byref(problem), sc, mg, path_joints.data_ptr() if F else None, path_len.data_ptr() if F else None, F, ml,
                                   C.byref(opts), *args, stream_handle(stream)), "ccmp_path_shortcut")
        return out
    pj, pl, F, ml = _host_inputs(path_joints, path_len)
    out = _host_outputs(pj, F, ml)
    if want_pairs:
        out.update(pair_ok=np.zeros((F, ml, ml), dtype=np.uint8), pair_states=np.zeros((F, ml, ml), dtype=np.int32),
                   pair_newton=np.zeros((F, ml, ml), dtype=np.int32))
    check(L.ccmp_path_shortcut_host(ctx.handle, C.byref(problem), sc, mg, _ptr(pj, _dp), _ptr(pl, _i32p), F, ml, C.byref(opts), _ptr(out["joints"], _dp),
                                    _ptr(out["out_len"], _i32p), _ptr(out["kept"], _i32p), _ptr(out["cost_in"], _dp), _ptr(out["cost_out"], _dp),
                                    _ptr(out.get("pair_ok"), _u8p), _ptr(out.get("pair_states"), _i32p), _ptr(out.get("pair_newton"), _i32p)),
          "ccmp_path_shortcut_host")
    return out
