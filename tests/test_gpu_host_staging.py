"""The planner-side *_host entry points share one staging helper (csrc/ccmp_stage.h: StagedCall on the context's staging block, CallArena
for a call's own memory).  These tests aim at what a shared helper can get wrong and a single entry point's own test does not see:
offsets that survive from an unlike call, a block regrown between calls, an optional output's piece, a piece of no bytes, caller memory
the call must leave alone.  Every expectation is the same entry point run another way — first on a fresh context, with the optional
outputs present, or as the device form — and comparisons are byte for byte.  State lists are compared up to what each edge stored: rows
beyond n_states are not written by the kernels, and the host form copies the whole piece down."""
import ctypes as C

import numpy as np
import pytest

from object_cases import box_mesh, random_poses, workspace
from test_gpu_parity import _constraint

from closed_chain_motion_planner_amd import _lib
from closed_chain_motion_planner_amd._lib import METRIC_OBJECT

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
MS, K, N_STORE = 8, 2, 6
SENTINEL = -7.0
_dp, _i32p, _u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
_TYPES = {np.dtype(np.float64): _dp, np.dtype(np.int32): _i32p, np.dtype(np.uint8): _u8p}


def _p(a):
    return a.ctypes.data_as(_TYPES[a.dtype]) if a is not None else None


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same(a, b, what=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), what


def _same_edges(a, b, names, what=""):
    """two connect / grow results: the named arrays as bytes, the state lists up to what each edge stored"""
    for name in names:
        _same(a[name], b[name], (what, name))
    for e, n in enumerate(a["n_states"].reshape(-1)):
        m = min(int(n), MS)
        _same(a["states"][e, :m], b["states"][e, :m], (what, "states", e))


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """valid projected states and their object poses as the device derives them; a small mesh, the fixture workspace, a few object poses"""
    from closed_chain_motion_planner_amd import Roadmap

    c = _constraint(OBJ, gpu_ctx)
    q, ok, _, _ = c.sample_project_batch(0x4B4E, 0, 1024, want_iters=False)
    good = np.ascontiguousarray(q[ok != 0].cpu().numpy()[:24])
    assert len(good) == 24
    rm = Roadmap(c, 32)
    rm.append(_dev(good))
    poses = np.ascontiguousarray(rm.read()[1].cpu().numpy())
    rm.close()
    return {"joints": good, "poses": poses, "mesh": box_mesh(0.04, 0.04, 0.1), "boxes": workspace(), "obj_poses": random_poses(np.random.default_rng(5), 3)}


def _store(c, w, edges=True):
    """six vertices and the chain 0-1-2-3-4-5, filled through the device forms (nothing here touches the staging block)"""
    from closed_chain_motion_planner_amd import Roadmap

    rm = Roadmap(c, 64)
    rm.append(_dev(w["joints"][:N_STORE]))
    if edges:
        assert rm.add_edges(_dev(np.array([[i, i + 1] for i in range(N_STORE - 1)], dtype=np.int32))) == 0
    return rm


# ---- the entry points with every optional output absent or present ---------------------------------------------------------------------
def _connect(c, rm, w, Q, optional):
    E = Q * K
    out = {"nbr_idx": np.empty((Q, K), np.int32), "nbr_dist": np.empty((Q, K)), "states": np.empty((E, MS, 14)), "n_states": np.empty(E, np.int32),
           "ok": np.empty(E, np.uint8), "newton_iters": np.empty(E, np.int32), "blocked": np.empty(E, np.uint8), "carry": np.empty((E, 2))}
    opt = lambda n: _p(out[n]) if optional else None
    qj = w["joints"][N_STORE:N_STORE + Q]
    rc = _lib.lib().ccmp_roadmap_connect_host(rm._h, C.byref(c.problem), None, 0.0, METRIC_OBJECT, _p(qj), None, Q, K, 0, 0, 1, MS, 0, _p(out["nbr_idx"]),
                                              opt("nbr_dist"), _p(out["states"]), _p(out["n_states"]), _p(out["ok"]), opt("newton_iters"), opt("blocked"),
                                              opt("carry"))
    assert rc == 0
    return out


def _grow(c, rm, w, Q, optional):
    from closed_chain_motion_planner_amd.ik import ik_options

    E = Q * K
    out = {"nbr_idx": np.empty((Q, K), np.int32), "nbr_dist": np.empty((Q, K)), "q_new": np.empty((Q, 14)), "ik_ok": np.empty(Q, np.uint8),
           "ik_which": np.empty(Q, np.int32), "states": np.empty((E, MS, 14)), "n_states": np.empty(E, np.int32), "ok": np.empty(E, np.uint8),
           "newton_iters": np.empty(E, np.int32), "blocked": np.empty(E, np.uint8), "carry": np.empty((E, 2))}
    opt = lambda n: _p(out[n]) if optional else None
    qp = w["poses"][N_STORE:N_STORE + Q]
    opts = ik_options(restarts=2)
    rc = _lib.lib().ccmp_roadmap_grow_host(rm._h, C.byref(c.problem), None, 0.0, C.byref(opts), _p(qp), Q, K, 0, 0, 11, 3, 0, MS, 0, _p(out["nbr_idx"]),
                                           opt("nbr_dist"), _p(out["q_new"]), _p(out["ik_ok"]), _p(out["ik_which"]), _p(out["states"]), _p(out["n_states"]),
                                           _p(out["ok"]), opt("newton_iters"), opt("blocked"), opt("carry"))
    assert rc == 0
    return out


def _paths(rm, src, dst, max_len, optional, prefill=-1):
    """ccmp_roadmap_shortest_paths_host through the C ABI: (rc, outputs); path / joints / poses start as `prefill`"""
    sr, ds = np.array(src, dtype=np.int32), np.array(dst, dtype=np.int32)
    F, N = len(sr), len(rm)
    out = {"cost": np.empty(F), "path_len": np.empty(F, np.int32), "path": np.full((F, max_len), int(prefill), np.int32),
           "joints": np.full((F, max_len, 14), float(prefill)), "poses": np.full((F, max_len, 8), float(prefill)), "dist": np.empty((F, N)),
           "pred": np.empty((F, N), np.int32)}
    opt = lambda n: _p(out[n]) if optional else None
    rc = _lib.lib().ccmp_roadmap_shortest_paths_host(rm._h, _p(sr), _p(ds), F, max_len, _p(out["cost"]), _p(out["path_len"]), _p(out["path"]), opt("joints"),
                                                     opt("poses"), opt("dist"), opt("pred"))
    return rc, out


def _ik(c, w, T, S, want):
    from closed_chain_motion_planner_amd.ik import ik_options

    tp = np.ascontiguousarray(w["poses"][10:10 + T])
    seeds = np.ascontiguousarray(w["joints"][13:13 + T * S].reshape(T, S, 14))
    return c.pose_ik_batch(tp, seeds, rng_seed=7, first_index=2, opts=ik_options(restarts=2), want_candidates=want)


# ---- 1. block growth between unlike calls ----------------------------------------------------------------------------------------------
def _sequence(w):
    """(name, call(c, rm, checker) -> dict of numpy arrays), staging needs small -> large -> small"""
    return [("object.valid", lambda c, rm, ch: dict(zip(("valid", "mask"), ch.valid(w["obj_poses"][:1], want_mask=True)))),
            ("roadmap.connect", lambda c, rm, ch: rm.connect(w["joints"][N_STORE:N_STORE + 3], K, METRIC_OBJECT, max_states=MS)),
            ("roadmap.closest", lambda c, rm, ch: dict(zip(("idx", "dist", "from_dist"), rm.closest(np.array([0], np.int32), w["poses"][9])))),
            ("pose_ik", lambda c, rm, ch: _ik(c, w, 2, 1, True)),
            ("roadmap.shortest_paths", lambda c, rm, ch: rm.shortest_paths([0, 1], [2, 4], max_len=4, host=True, full=True))]


def _compare(name, got, want):
    if name == "roadmap.connect":
        _same_edges(got, want, ("nbr_idx", "nbr_dist", "n_states", "ok", "newton_iters", "blocked", "carry"), name)
    else:
        assert set(got) == set(want)
        for key in want:
            _same(got[key], want[key], (name, key))


def test_block_growth_between_unlike_calls(world):
    """every call of the sequence on ONE context gives the bytes of the same call made first on a fresh context: no offset survives from
    the call before, and the block that grows for connect serves the smaller calls behind it"""
    from closed_chain_motion_planner_amd import Context
    from closed_chain_motion_planner_amd.object import ObjectChecker

    def fresh():
        ctx = Context(0)
        c = _constraint(OBJ, ctx)
        return ctx, c, _store(c, world), ObjectChecker(ctx, world["mesh"], world["boxes"])

    def done(ctx, rm, ch):
        rm.close()
        ch.close()
        ctx.close()

    seq = _sequence(world)
    first = []
    for name, call in seq:
        ctx, c, rm, ch = fresh()
        first.append(call(c, rm, ch))
        done(ctx, rm, ch)
    ctx, c, rm, ch = fresh()
    for (name, call), want in zip(seq, first):
        _compare(name, call(c, rm, ch), want)
    for (name, call), want in zip(seq, first):  # and once more, the block at its final size
        _compare(name, call(c, rm, ch), want)
    done(ctx, rm, ch)
    assert first[4]["path_len"].tolist() == [3, 4] and first[4]["path"][1].tolist() == [1, 2, 3, 4]


# ---- 2. every optional output absent, then present -------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", [1, 3])
def test_optional_outputs_absent_then_present(world, gpu_ctx, Q):
    """the mandatory outputs do not depend on which optional ones the caller asked for"""
    from closed_chain_motion_planner_amd.object import ObjectChecker

    c = _constraint(OBJ, gpu_ctx)
    rm = _store(c, world)
    # connect: nbr_dist, newton_iters, blocked, carry_out
    a, b = _connect(c, rm, world, Q, False), _connect(c, rm, world, Q, True)
    _same_edges(a, b, ("nbr_idx", "n_states", "ok"), "connect")
    _same_edges(b, rm.connect(world["joints"][N_STORE:N_STORE + Q], K, METRIC_OBJECT, max_states=MS), ("nbr_idx", "nbr_dist", "n_states", "ok", "carry"), "connect wrapper")
    # grow: the same four
    ga, gb = _grow(c, rm, world, Q, False), _grow(c, rm, world, Q, True)
    _same_edges(ga, gb, ("nbr_idx", "q_new", "ik_ok", "ik_which", "n_states", "ok"), "grow")
    # commit: states, vertex_ok (each run on a store of its own: a commit appends)
    qj, qp = world["joints"][N_STORE:N_STORE + Q], world["poses"][N_STORE:N_STORE + Q]
    runs = []
    for states, vok in ((None, None), (b["states"], np.ones(Q, np.uint8))):
        s = _store(c, world)
        runs.append(s.commit(b["nbr_idx"], b["ok"], b["n_states"], qj, qp, states=states, vertex_ok=vok, max_states=MS))
        runs[-1]["rows"] = s.read(host=True)[0]
        s.close()
    for key in ("new_index", "mid_index", "grow_state", "rows"):
        _same(runs[0][key], runs[1][key], ("commit", key))
    assert runs[0]["vertices_added"] == runs[1]["vertices_added"] and runs[0]["edges_added"] == runs[1]["edges_added"]
    # pose_ik: cand_q, cand_rounds
    ia, ib = _ik(c, world, Q, K, False), _ik(c, world, Q, K, True)
    for key in ("q", "ok", "which"):
        _same(ia[key], ib[key], ("pose_ik", key))
    # object.propose: cand_pose, cand_valid
    ch = ObjectChecker(gpu_ctx, world["mesh"], world["boxes"])
    kw = dict(attempts=2, rng_seed=3, first_index=1)
    pa, pb = ch.propose(world["obj_poses"][:Q], world["obj_poses"][2], **kw), ch.propose(world["obj_poses"][:Q], world["obj_poses"][2], want_candidates=True, **kw)
    for key in ("pose", "which"):
        _same(pa[key], pb[key], ("propose", key))
    ch.close()
    # shortest_paths: path_joints / path_poses, dist / pred
    src, dst = [0, 1, 5][:Q], [2, 4, 3][:Q]
    (ra, sa), (rb, sb) = _paths(rm, src, dst, 4, False), _paths(rm, src, dst, 4, True)
    assert ra == 0 and rb == 0
    for key in ("cost", "path_len", "path"):
        _same(sa[key], sb[key], ("shortest_paths", key))
    assert (sa["joints"] == -1).all() and (sa["poses"] == -1).all()  # absent: never touched
    rm.close()


# ---- 3. zero-length pieces -------------------------------------------------------------------------------------------------------------
def test_zero_length_pieces(world, gpu_ctx):
    from closed_chain_motion_planner_amd import Roadmap

    c = _constraint(OBJ, gpu_ctx)
    j, p = world["joints"][:3], world["poses"][:3]
    # append with poses only, and with joints only: the store of the device form
    host, dev = Roadmap(c, 8), Roadmap(c, 8)
    assert host.append(None, p) == 0 and dev.append(None, _dev(p)) == 0
    assert host.append(j) == 3 and dev.append(_dev(j)) == 3
    for a, b in zip(host.read(host=True), dev.read()):
        _same(a, b.cpu().numpy(), "append")
    assert np.isnan(host.read(host=True)[0][:3]).all()
    host.close()
    dev.close()
    # commit with Q = 1, k = 1 and neither states nor vertex_ok; add_edges with E = 1
    host, dev = _store(c, world, edges=False), _store(c, world, edges=False)
    args = (np.array([[2]], np.int32), np.array([1], np.uint8), np.array([2], np.int32), world["joints"][6:7], world["poses"][6:7])
    a, b = host.commit(*args, max_states=MS), dev.commit(*[_dev(x) for x in args], max_states=MS)
    for key in ("new_index", "mid_index", "grow_state"):
        _same(a[key], b[key].cpu().numpy(), ("commit", key))
    assert a["new_index"].tolist() == [N_STORE] and a["vertices_added"] == b["vertices_added"] == 1 and a["edges_added"] == b["edges_added"] == 1
    assert host.add_edges(np.array([[0, 1]], np.int32)) == 0 and dev.add_edges(_dev(np.array([[0, 1]], np.int32))) == 0
    for x, y in zip(host.edges(host=True), dev.edges()):
        _same(x, y.cpu().numpy(), "edges")
    _same(host.labels(host=True), dev.labels().cpu().numpy(), "labels")
    assert host.num_edges == 2
    # a path of one vertex (no pair, no segment) and of two, through the store and as the host forms of the same rows
    for goal, n in ((0, 1), (1, 2)):
        cost, idx, sc_joints, sc = host.shortcut_solution(c, [0], [goal], max_len=4)
        assert idx.tolist() == list(range(n)) and int(sc["out_len"][0]) == n and sc["kept"][0, :n].cpu().tolist() == list(range(n))
        _same(sc_joints.cpu().numpy(), world["joints"][:n], "shortcut rows")
        _, didx, dense = host.dense_solution(c, [0], [goal], max_len=4)
        assert didx.tolist() == list(range(n)) and dense["path_first"].cpu().tolist() == [0, dense["rows"]] and dense["rows"] >= n
        pj, pl = np.ascontiguousarray(world["joints"][:n].reshape(1, n, 14)), np.array([n], np.int32)
        hs, hd = c.shortcut_paths(pj, pl), c.densify_paths(pj, pl)
        for key in ("joints", "out_len", "kept", "cost_in", "cost_out"):
            _same(hs[key], sc[key].cpu().numpy(), ("shortcut host", n, key))
        for key in ("joints", "path_first", "seg_first", "seg_ok", "seg_newton", "arc", "length"):
            _same(hd[key], dense[key].cpu().numpy(), ("densify host", n, key))
        assert hd["rows"] == dense["rows"]
        if n == 1:
            assert dense["rows"] == 1 and float(hs["cost_in"][0]) == 0.0
    host.close()
    dev.close()


# ---- 4. untouched caller memory --------------------------------------------------------------------------------------------------------
def test_untouched_caller_memory(world, gpu_ctx):
    c = _constraint(OBJ, gpu_ctx)
    rm = _store(c, world)
    # a path longer than max_len leaves its rows of path / joints / poses as the caller filled them; one that fits writes its entries alone
    rc, out = _paths(rm, [0, 0], [5, 2], 4, True, prefill=SENTINEL)
    assert rc == 0 and out["path_len"].tolist() == [6, 3]
    assert (out["path"][0] == int(SENTINEL)).all() and (out["joints"][0] == SENTINEL).all() and (out["poses"][0] == SENTINEL).all()
    assert out["path"][1].tolist() == [0, 1, 2, int(SENTINEL)]
    _same(out["joints"][1, :3], world["joints"][:3], "path joints")
    assert (out["joints"][1, 3:] == SENTINEL).all() and (out["poses"][1, 3:] == SENTINEL).all() and not (out["poses"][1, :3] == SENTINEL).any()
    rm.close()
    # the shortcut host forms: rows of out_joints behind out_len keep the caller's values
    L = _lib.lib()
    F, ml, n = 1, 4, 3
    pj = np.ascontiguousarray(world["joints"][:ml].reshape(F, ml, 14))
    pl = np.array([n], np.int32)
    for select in (False, True):
        oj = np.full((F, ml, 14), SENTINEL)
        olen, kept, ci, co = np.zeros(F, np.int32), np.full((F, ml), -5, np.int32), np.zeros(F), np.zeros(F)
        if select:
            pair_ok = np.ones((F, ml, ml), np.uint8)
            rc = L.ccmp_shortcut_select_host(c.ctx.handle, _p(pj), _p(pl), F, ml, _p(pair_ok), _p(oj), _p(olen), _p(kept), _p(ci), _p(co))
        else:
            rc = L.ccmp_path_shortcut_host(c.ctx.handle, C.byref(c.problem), None, 0.0, _p(pj), _p(pl), F, ml, None, _p(oj), _p(olen), _p(kept), _p(ci), _p(co),
                                           None, None, None)
        m = int(olen[0])
        assert rc == 0 and 2 <= m <= n and (not select or m == 2), (select, rc, m)
        assert (oj[0, m:] == SENTINEL).all(), select
        _same(oj[0, :m], pj[0, kept[0, :m]], ("kept rows", select))
        assert kept[0, 0] == 0 and kept[0, m - 1] == n - 1 and (kept[0, m:] == -1).all()
