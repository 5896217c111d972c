"""Smooth solution paths on the device (ccmp_path_smooth: the pass loop over the dense unit's densify, the projector, the shortcut unit's
tile loop and the smooth_* kernels) through the device form and the host form.  Expected values are never the code under test: the
plain-Python restatement of tests/smooth_cases.py on the det oracle's discrete_geodesic, project, is_satisfied and interpolate, with
distances in the library's rounding.  Comparisons are bit for bit: rows, out_len, passes, moved, stop, stats, lengths.  Calls through the
C ABI give every output a guard element that must survive, and rows behind out_len must keep their guard value."""
import ctypes as C

import numpy as np
import pytest

from dense_path_cases import RECORDED, recorded_roadmap
from shortcut_cases import recorded_waypoints
from smooth_cases import BELOW, DEGENERATE, FALLBACK, PROJECTED, REFUSED, Restatement, expect, mirror_fill, same_f64, same_result
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
EINVAL, EOVERFLOW = -1, -8
GUARD_F64, GUARD_I32 = -7.0, -77
NAMES = ("joints", "out_len", "passes", "moved", "stop", "length_in", "length_out", "stats")


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def cons(gpu_ctx):
    """one constraint per (object, Jacobian mode), delta as the object's file was recorded with"""
    made = {}

    def get(obj, mode):
        if (obj, mode) not in made:
            c = _constraint(obj, gpu_ctx, mode)
            c.problem.delta = RECORDED[obj]["delta"]
            made[(obj, mode)] = c
        return made[(obj, mode)]

    return get


def _guarded(c, pj, pl, cap, opts=None, scene=None, margin=0.0):
    """ccmp_path_smooth through the C ABI: every output one element longer than the call is told, pre-filled with a guard value.
    Returns (rc, outputs as numpy without the guard, True if every guard survived, raw buffers)."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    F, ml = pj.shape[0], pj.shape[1]
    full = lambda n, dt, v: torch.full((n + 1,), v, dtype=dt, device=pj.device)
    buf = {"joints": full(F * cap * 14, torch.float64, GUARD_F64), "length_in": full(F, torch.float64, GUARD_F64), "length_out": full(F, torch.float64, GUARD_F64),
           "stats": full(F * 5, torch.int32, GUARD_I32)}
    for k in ("out_len", "passes", "moved", "stop"):
        buf[k] = full(F, torch.int32, GUARD_I32)
    o = _lib.CcmpSmoothOpts(*opts) if opts is not None else None
    rc = _lib.lib().ccmp_path_smooth(c.ctx.handle, C.byref(c.problem), scene._h if scene is not None else None, float(margin), pj.data_ptr(), pl.data_ptr(), F, ml,
                                     C.byref(o) if o is not None else None, cap, *[buf[k].data_ptr() for k in NAMES], None)
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in buf.items()}
    intact = all(host[k][-1] == (GUARD_F64 if host[k].dtype == np.float64 else GUARD_I32) for k in host)
    shapes = {"joints": (F, cap, 14), "stats": (F, 5)}
    return rc, {k: host[k][:-1].reshape(shapes.get(k, (F,))) for k in host}, intact, host


def _untouched(raw):
    return all((v == (GUARD_F64 if v.dtype == np.float64 else GUARD_I32)).all() for v in raw.values())


# ---- 1. the recorded files' waypoints, projected ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded(oracle_det):
    made = {}

    def get(obj, mode, max_steps=3):
        key = (obj, mode, max_steps)
        if key not in made:
            P, pj, pl = recorded_waypoints(oracle_det, obj, mode, True)
            R = Restatement(oracle_det, P)
            cap = 2 ** max_steps * (pj.shape[1] - 1) + 1
            made[key] = (P, pj, pl, R, cap, expect(R, pj, pl, max_steps, 0.005, cap, mirror_fill(pj, cap)))
        return made[key]

    return get


@pytest.mark.parametrize("budget", [0, 8])
@pytest.mark.parametrize("chunk", [2, 16])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("obj", ["Wine_Bottle", "dumbbell"])
def test_recorded_waypoints(cons, recorded, oracle_det, obj, mode, chunk, budget):
    from closed_chain_motion_planner_amd import smooth_len_after

    c = cons(obj, mode)
    P, pj, pl, R, cap, want = recorded(obj, mode)
    assert bytes(_oracle_problem(oracle_det, c)) == bytes(P) and cap == smooth_len_after(pj.shape[1], 3)
    assert (want["passes"] == 3).all() and (want["moved"] > 0).all() and (want["length_out"] < want["length_in"]).all()
    if chunk == 2:
        assert max(R.list_lengths) > 2  # a list longer than one extend call holds: at least one list needed a continuation
    got = c.smooth_paths(_dev(pj), _dev(pl), max_steps=3, chunk_states=chunk, round_budget=budget, stats=True)
    same_result(got, want, (obj, mode, chunk, budget, "device"))
    host = c.smooth_paths(pj, pl, max_steps=3, chunk_states=chunk, round_budget=budget, stats=True)
    same_result(host, want, (obj, mode, chunk, budget, "host"))
    if obj == OBJ and chunk == 16 and budget == 0:
        n = int(got["out_len"][0])
        dense = c.densify_paths(got["joints"][:, :n].contiguous(), got["out_len"], distinct=True)
        assert n == 33 and bool((dense["seg_ok"][0, : n - 1] == 1).all())  # every segment of the smoothed path is traversable


def test_five_passes_converge(cons, recorded):
    c = cons(OBJ, 0)
    P, pj, pl, R, cap, want = recorded(OBJ, 0, 5)
    assert want["stop"][0] == 1 and want["passes"][0] == 5 and want["out_len"][0] == 129 and want["stats"][0, BELOW] > 0
    same_result(c.smooth_paths(_dev(pj), _dev(pl), stats=True), want, "defaults")


# ---- 2. every branch of the rule --------------------------------------------------------------------------------------------------------
def test_every_branch(gpu_ctx, oracle_det):
    c = _constraint(OBJ, gpu_ctx, 0)
    c.problem.delta = RECORDED[OBJ]["delta"]
    c.problem.max_iter = 12  # (setMaxIterations sets the base-class field the reference's project() never reads)
    P = _oracle_problem(oracle_det, c)
    assert P.max_iter == 12
    P0, pj, pl = recorded_waypoints(oracle_det, OBJ, 0, True)  # projected under the stock iteration cap
    want = expect(Restatement(oracle_det, P), pj, pl, 3, 0.005, 33, mirror_fill(pj, 33))
    s = want["stats"][0]
    assert min(s[PROJECTED], s[FALLBACK], s[DEGENERATE], s[REFUSED], s[BELOW]) >= 1 and want["moved"][0] >= 1, s
    same_result(c.smooth_paths(_dev(pj), _dev(pl), max_steps=3, stats=True), want, "device")
    same_result(c.smooth_paths(pj, pl, max_steps=3, stats=True), want, "host")


# ---- 3. a ragged batch --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ragged(oracle_det, recorded):
    P = recorded(OBJ, 0)[0]
    nodes, _ = recorded_roadmap()
    proj = np.array([oracle_det.project(P, q)[1] for q in nodes])
    lens = [0, 1, 2, 3, 5, 10, 6]
    pj = np.full((7, 10, 14), np.nan)  # rows behind a path's length are never read
    for f, L in enumerate(lens):
        pj[f, :L] = proj[:L]
    pj[6, 3, 4] = np.nan  # a NaN row in the interior
    pl = np.array(lens, dtype=np.int32)
    R = Restatement(oracle_det, P)
    return P, pj, pl, R, expect(R, pj, pl, 3, 0.005, 19, GUARD_F64)


def test_ragged_batch(cons, ragged):
    c = cons(OBJ, 0)
    P, pj, pl, R, want = ragged
    assert want["stop"].tolist() == [0, 0, 0, 2, 3, 3, 4] and want["passes"].tolist() == [0, 0, 0, 3, 2, 1, 0]
    assert want["out_len"].tolist() == [0, 1, 2, 17, 17, 19, 6] and np.isnan(want["length_in"][6]) and np.isnan(want["length_out"][6])
    results = []
    for tile in (1, 7, 65536):
        rc, out, intact, _ = _guarded(c, _dev(pj), _dev(pl), 19, opts=(3, 0.005, 16, 128, 4096, tile))
        assert rc == 0 and intact, tile
        same_result(out, want, tile)  # rows behind out_len keep the guard value: `want` was filled with it
        results.append(out)
    for r in results[1:]:
        for k in r:
            assert same_f64(r[k], results[0][k]) if r[k].dtype == np.float64 else np.array_equal(r[k], results[0][k]), k
    host = c.smooth_paths(pj, pl, max_steps=3, out_max_len=19, stats=True)
    alone_fill = mirror_fill(pj, 19)
    for f in range(7):  # each path equals the same path run alone
        alone = c.smooth_paths(_dev(pj[f : f + 1]), _dev(pl[f : f + 1]), max_steps=3, out_max_len=19, stats=True)
        n = int(want["out_len"][f])
        w = {k: v[f : f + 1].copy() for k, v in want.items()}
        w["joints"][0, n:] = alone_fill[f, n:]
        same_result(alone, w, ("alone", f))
        same_result({k: v[f : f + 1] for k, v in host.items()}, w, ("host", f))


# ---- 4. limits ----------------------------------------------------------------------------------------------------------------------------
def test_limits(cons, recorded, oracle_det):
    c = cons(OBJ, 0)
    P, pj, pl, R, _, _ = recorded(OBJ, 0)
    got = c.smooth_paths(_dev(pj), _dev(pl), max_steps=0, stats=True)  # the identity
    assert got["joints"].shape == (1, 5, 14) and same_f64(got["joints"].cpu().numpy(), pj)
    assert (int(got["stop"][0]), int(got["passes"][0]), int(got["moved"][0]), int(got["out_len"][0])) == (2, 0, 0, 5)
    assert int(got["stats"].sum()) == 0 and same_f64(got["length_in"].cpu().numpy(), got["length_out"].cpu().numpy())
    same_result(got, expect(R, pj, pl, 0, 0.005, 5, mirror_fill(pj, 5)), "max_steps 0")
    inf = float("inf")
    want = expect(R, pj, pl, 3, inf, 33, mirror_fill(pj, 33))
    assert (want["passes"][0], want["moved"][0], want["stop"][0], want["out_len"][0]) == (1, 0, 1, 9)
    assert same_f64(want["joints"][0, 0:9:2], pj[0]) and want["stats"][0, REFUSED] + want["stats"][0, BELOW] == 3  # the subdivided path
    same_result(c.smooth_paths(_dev(pj), _dev(pl), max_steps=3, min_change=inf, stats=True), want, "min_change inf")


# ---- 5. with a proxy scene ----------------------------------------------------------------------------------------------------------------
def test_scene_case(cons, recorded, oracle_det):
    from closed_chain_motion_planner_amd import scene as S
    from test_gpu_geodesic_scene import OracleScene

    c = cons(OBJ, 0)
    P, pj, pl, _, cap, plain = recorded(OBJ, 0)
    sc = S.ProxyValidityChecker(c).scene
    clear = lambda x: oracle_det.clearance(P, sc.spheres, sc.boxes, sc.allowed, x)[0]
    # the margin from the observed clearances of the candidates and their neighbours: the endpoints of every checkMotion of two plain passes
    seen = []
    spy = Restatement(oracle_det, P)
    inner = spy.check_motion
    spy.check_motion = lambda a, b: (seen.extend([np.array(a), np.array(b)]), inner(a, b))[1]
    spy.smooth(pj[0, :5], 2, 0.005, cap)
    margin = float(np.quantile([clear(x) for x in seen], 0.25))
    orc = OracleScene(oracle_det, P, sc, margin)
    blocked = []

    def edge(a, b):
        r, _, n, _, _, bl, _ = orc.edge(a, b, 4096)
        assert n <= 4096
        blocked.append(bl)
        return r

    R = Restatement(oracle_det, P, valid=edge, clearance=clear, margin=margin)
    want = expect(R, pj, pl, 3, 0.005, cap, mirror_fill(pj, cap))
    # with the oracle's checker alone: some candidate is refused by clearance or by a cut traversal, and some are accepted
    assert want["stats"][0, REFUSED] >= 1 and want["moved"][0] >= 1 and not same_f64(want["joints"], plain["joints"])
    for chunk in (2, 16):
        for budget in (0, 8):
            got = c.smooth_paths(_dev(pj), _dev(pl), max_steps=3, scene=sc, margin=margin, chunk_states=chunk, round_budget=budget, stats=True)
            same_result(got, want, ("scene", chunk, budget))
    same_result(c.smooth_paths(pj, pl, max_steps=3, scene=sc, margin=margin, stats=True), want, "scene host")


# ---- 6. max_calls spent: nothing is written; bad arguments ------------------------------------------------------------------------------------
def test_overflow_leaves_the_outputs_untouched_and_bad_arguments_are_refused(cons, recorded):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, _lib
    from closed_chain_motion_planner_amd import scene as S

    c = cons(OBJ, 0)
    P, pj, pl, R, cap, _ = recorded(OBJ, 0)
    assert max(R.list_lengths) > 2  # a list that one extend call of two entries cannot finish
    pj_d, pl_d = _dev(pj), _dev(pl)
    rc, _, _, raw = _guarded(c, pj_d, pl_d, cap, opts=(3, 0.005, 2, 128, 1, 65536))
    assert rc == EOVERFLOW and _untouched(raw)
    with pytest.raises(CcmpError) as e:
        c.smooth_paths(pj_d, pl_d, chunk_states=2, max_calls=1)
    assert e.value.code == EOVERFLOW
    nan = float("nan")
    for bad in (dict(max_steps=-1), dict(min_change=-0.5), dict(min_change=nan), dict(out_max_len=4), dict(out_max_len=0), dict(tile_edges=0),
                dict(chunk_states=1), dict(round_budget=-1), dict(max_calls=0)):
        with pytest.raises(CcmpError) as e:
            c.smooth_paths(pj_d, pl_d, **bad)
        assert e.value.code == EINVAL, bad
    sc = S.ProxyValidityChecker(c).scene
    with pytest.raises(CcmpError) as e:  # the scene errors of the sibling calls
        c.smooth_paths(pj_d, pl_d, scene=sc, margin=nan)
    assert e.value.code == EINVAL
    with pytest.raises(ValueError):
        c.smooth_paths(pj_d, pl_d, scene=sc)
    for bad_len in (pj.shape[1] + 1, -1):
        rc, _, _, raw = _guarded(c, pj_d, _dev(np.array([bad_len], dtype=np.int32)), cap)
        assert rc == EINVAL and _untouched(raw)
    L = _lib.lib()
    out = [torch.zeros(n, dtype=dt, device="cuda") for n, dt in ((5 * 14, torch.float64), (1, torch.int32), (1, torch.int32), (1, torch.int32), (1, torch.int32),
                                                                 (1, torch.float64), (1, torch.float64), (5, torch.int32))]
    o = _lib.CcmpSmoothOpts(0, 0.005, 16, 128, 4096, 65536)
    head = [c.ctx.handle, C.byref(c.problem), None, 0.0, pj_d.data_ptr(), pl_d.data_ptr(), 1, 5, C.byref(o), 5]
    ptrs = [t.data_ptr() for t in out]
    assert L.ccmp_path_smooth(*(head + ptrs + [None])) == 0
    assert L.ccmp_path_smooth(*(head + ptrs[:7] + [None, None])) == 0  # stats is optional
    for k, alias in ((0, pj_d.data_ptr() + 14 * 8), (1, pl_d.data_ptr()), (7, pj_d.data_ptr())):  # an output overlapping an input
        p = list(ptrs)
        p[k] = alias
        assert L.ccmp_path_smooth(*(head + p + [None])) == EINVAL, k
    for k in range(7):  # a NULL required pointer
        p = list(ptrs)
        p[k] = None
        assert L.ccmp_path_smooth(*(head + p + [None])) == EINVAL, k
    assert L.ccmp_path_smooth(*(head[:4] + [None] + head[5:] + ptrs + [None])) == EINVAL
    assert L.ccmp_path_smooth(*(head[:5] + [None] + head[6:] + ptrs + [None])) == EINVAL
    assert L.ccmp_path_smooth(*(head[:7] + [0] + head[8:] + ptrs + [None])) == EINVAL  # max_len < 1
    empty = c.smooth_paths(pj_d[:0], pl_d[:0], stats=True)  # F == 0 touches nothing
    assert empty["out_len"].numel() == 0 and empty["joints"].shape == (0, 129, 14)
    assert L.ccmp_path_smooth(*(head[:4] + [None, None, 0, 5, None, 5] + [None] * 9)) == 0


# ---- 7. solution -> shortcut -> smooth -> densify -------------------------------------------------------------------------------------------
def test_dense_smooth_solution(cons):
    from closed_chain_motion_planner_amd import Roadmap

    c = cons(OBJ, 0)
    nodes, uv = recorded_roadmap()
    rm = Roadmap(c, capacity_hint=4)
    try:
        rm.append(_dev(nodes))
        assert rm.add_edges(_dev(uv)) == 0
        _, idx, joints = rm.solution([0, 1], [9, 6])
        n = len(idx)
        sc = c.shortcut_paths(joints.reshape(1, n, 14).contiguous(), _dev(np.array([n], dtype=np.int32)))
        m = int(sc["out_len"][0])
        sm = c.smooth_paths(sc["joints"][:, :m].contiguous(), sc["out_len"], max_steps=2, stats=True)
        k = int(sm["out_len"][0])
        ref = c.densify_paths(sm["joints"][:, :k].contiguous(), sm["out_len"], distinct=True)
        length, idx2, dense, sm2, sc2 = rm.dense_smooth_solution(c, [0, 1], [9, 6], max_steps=2, stats=True, distinct=True)
        assert np.array_equal(idx2, idx[sc["kept"][0, :m].cpu().numpy()]) and length == float(sm["length_out"][0])
        for key in ("joints", "arc", "length"):
            assert same_f64(dense[key].cpu().numpy(), ref[key].cpu().numpy()), key
        for key in ("path_first", "seg_first", "seg_ok", "seg_newton"):
            assert np.array_equal(dense[key].cpu().numpy(), ref[key].cpu().numpy()), key
        for key in NAMES:
            a, b = sm2[key].cpu().numpy(), sm[key].cpu().numpy()
            assert same_f64(a, b) if a.dtype == np.float64 else np.array_equal(a, b), key
        length3, idx3, joints3, _, _ = rm.smooth_solution(c, [0, 1], [9, 6], max_steps=2)
        assert length3 == length and np.array_equal(idx3, idx2) and same_f64(joints3.cpu().numpy(), sm["joints"][0, :k].cpu().numpy())
    finally:
        rm.close()
