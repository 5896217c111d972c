"""ccmp_connect_batch / ccmp_connect_host — neighbours and their traversals in one call — against the entry points it composes
(ccmp_knn_batch, ccmp_check_motion_batch, ccmp_geodesic_batch_ex, ccmp_geodesic_scene_batch) on the gathered pairs, bit for bit,
and against the CPU checker directly.  No test asserts a share of reached edges: counts are printed."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_roadmap
from test_gpu_parity import _constraint, _oracle_problem

from closed_chain_motion_planner_amd import _lib

pytestmark = pytest.mark.gpu

N, Q, K, MAXS = 400, 24, 5, 16


def _world(gpu_ctx, mode):
    import torch

    c = _constraint("Wine_Bottle", gpu_ctx, mode=mode)
    q, ok, _, _ = c.sample_project_batch(0xC0EC, 0, 4096, want_iters=False)
    good = q[ok != 0]
    assert good.shape[0] >= N + Q
    return c, good[:N].contiguous(), good[N: N + Q].contiguous(), torch


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _gathered(nodes, queries, idx):
    """(from, to, occupied) of the edges e = q * k + r"""
    flat = idx.reshape(-1).long()
    occ = flat >= 0
    to = queries.repeat_interleave(idx.shape[1], dim=0)
    frm = to.clone()
    frm[occ] = nodes[flat[occ]]
    return frm.contiguous(), to.contiguous(), occ.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _check_edges(got, want_states, want_n, want_ok, want_its, want_carry, occ):
    for e in np.flatnonzero(occ):
        assert got["n_states"][e] == want_n[e] and got["ok"][e] == want_ok[e] and got["newton_iters"][e] == want_its[e], e
        m = min(int(want_n[e]), MAXS)
        assert _same_bits(got["states"][e, :m], want_states[e, :m]), e
        if want_carry is not None:
            assert _same_bits(got["carry"][e], want_carry[e]), e


def _check_empty(got, occ):
    emp = ~occ
    for key in ("ok", "n_states", "newton_iters", "blocked"):
        assert not got[key][emp].any(), key
    assert not got["carry"][emp].any()


@pytest.mark.parametrize("mode", [0, 1])
def test_connect_equals_its_parts(gpu_ctx, oracle_det, mode):
    c, nodes, queries, torch = _world(gpu_ctx, mode)
    P = _oracle_problem(oracle_det, c)
    idx, dist = c.nearest_k_batch(nodes, queries, K)
    frm, to, occ = _gathered(nodes, queries, idx)
    assert occ.all()
    E = Q * K
    # check_target = 1: addMilestone's checkMotion
    a = _np(c.connect_batch(nodes, queries, K, check_target=True, max_states=MAXS))
    assert np.array_equal(a["nbr_idx"], idx.cpu().numpy()) and _same_bits(a["nbr_dist"], dist.cpu().numpy())
    st = torch.empty((E, MAXS, 14), dtype=torch.float64, device="cuda")
    n = torch.empty(E, dtype=torch.int32, device="cuda")
    ok = torch.empty(E, dtype=torch.uint8, device="cuda")
    its = torch.empty(E, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib().ccmp_check_motion_batch(c.ctx.handle, C.byref(c.problem), frm.data_ptr(), to.data_ptr(), E, MAXS, st.data_ptr(), n.data_ptr(),
                                                  ok.data_ptr(), its.data_ptr(), None), "ccmp_check_motion_batch")
    carry = c.discrete_geodesic_batch(frm, to, MAXS, check_target=True, want_carry=True)[4]
    _check_edges(a, st.cpu().numpy(), n.cpu().numpy(), ok.cpu().numpy(), its.cpu().numpy(), carry.cpu().numpy(), occ)
    assert not a["blocked"].any()
    # check_target = 0 with a round budget: growTree's discreteGeodesic, resumable
    b = _np(c.connect_batch(nodes, queries, K, check_target=False, max_states=MAXS, round_budget=32))
    w = [t.cpu().numpy() for t in c.discrete_geodesic_batch(frm, to, MAXS, check_target=False, want_carry=True, round_budget=32)]
    _check_edges(b, w[0], w[1], w[2], w[3], w[4], occ)
    print("mode %d: %d / %d edges reached (check_target), %d suspended at 32 rounds, %d lists full" %
          (mode, int((a["ok"] == 1).sum()), E, int((b["ok"] == 2).sum()), int((a["n_states"] == MAXS + 1).sum())))
    # the CPU checker directly, eight slots
    fn, tn = frm.cpu().numpy(), to.cpu().numpy()
    for e in range(0, E, E // 8)[:8]:
        if not oracle_det.is_satisfied(P, tn[e]):  # checkMotion's first test
            assert a["ok"][e] == 0 and a["n_states"][e] == 1 and a["newton_iters"][e] == 0 and _same_bits(a["states"][e, 0], fn[e])
            continue
        ok_cpu, st_cpu, its_cpu = oracle_det.discrete_geodesic(P, fn[e], tn[e], interpolate=True, max_states=MAXS)
        if a["n_states"][e] > MAXS:
            assert a["n_states"][e] == MAXS + 1 and a["ok"][e] == 0 and len(st_cpu) > MAXS
            assert _same_bits(a["states"][e], st_cpu[:MAXS])
        else:
            assert a["n_states"][e] == len(st_cpu) and bool(a["ok"][e]) == ok_cpu and a["newton_iters"][e] == its_cpu
            assert _same_bits(a["states"][e, : len(st_cpu)], st_cpu)


@pytest.mark.parametrize("mode", [0, 1])
def test_empty_slots_and_unsatisfied_target(gpu_ctx, mode):
    c, nodes, queries, torch = _world(gpu_ctx, mode)
    # three nodes, five slots
    got = _np(c.connect_batch(nodes[:3].contiguous(), queries, K, check_target=True, max_states=MAXS, round_budget=32))
    occ = got["nbr_idx"].reshape(-1) >= 0
    assert occ.reshape(Q, K)[:, :3].all() and not occ.reshape(Q, K)[:, 3:].any()
    _check_empty(got, occ)
    frm, to, _ = _gathered(nodes[:3], queries, torch.as_tensor(got["nbr_idx"]).cuda())
    w = [t.cpu().numpy() for t in c.discrete_geodesic_batch(frm[torch.as_tensor(occ).cuda()].contiguous(), to[torch.as_tensor(occ).cuda()].contiguous(), MAXS,
                                                             check_target=True, want_carry=True, round_budget=32)]
    sub = {k: (v.reshape(Q * K, *v.shape[2:]) if k.startswith("nbr") else v)[occ] for k, v in got.items()}
    _check_edges(sub, w[0], w[1], w[2], w[3], w[4], np.ones(int(occ.sum()), dtype=bool))
    assert got["newton_iters"].sum() == w[3].sum() > 0  # the empty slots cost no Newton work
    # no node at all
    none = _np(c.connect_batch(nodes[:0], queries, K, check_target=True, max_states=MAXS))
    assert np.all(none["nbr_idx"] == -1) and np.all(np.isinf(none["nbr_dist"]))
    _check_empty(none, np.zeros(Q * K, dtype=bool))
    # a target off the manifold (an IK milestone of the recorded roadmap): checkMotion refuses all its slots without traversing
    qs = queries.clone()
    qs[7] = torch.as_tensor(load_roadmap("Wine_Bottle")[0][2]).cuda()
    off = _np(c.connect_batch(nodes, qs, K, check_target=True, max_states=MAXS))
    sl = slice(7 * K, 8 * K)
    assert np.all(off["nbr_idx"][7] >= 0) and not off["ok"][sl].any() and np.all(off["n_states"][sl] == 1) and not off["newton_iters"][sl].any()
    assert _same_bits(off["states"][sl, 0], nodes.cpu().numpy()[off["nbr_idx"][7]])


@pytest.mark.parametrize("mode", [0, 1])
def test_connect_with_a_scene(gpu_ctx, mode):
    from closed_chain_motion_planner_amd.scene import ProxyScene, default_allowed, skeleton_spheres

    c, nodes, queries, torch = _world(gpu_ctx, mode)
    scene = ProxyScene(c, skeleton_spheres(c.problem), (), default_allowed())
    idx, _ = c.nearest_k_batch(nodes, queries, K)
    frm, to, occ = _gathered(nodes, queries, idx)
    for margin in (-0.03, 0.02):  # the default skeleton's margin, and one that refuses more
        got = _np(c.connect_batch(nodes, queries, K, check_target=True, max_states=MAXS, round_budget=32, scene=scene, margin=margin))
        w = [t.cpu().numpy() for t in c.discrete_geodesic_scene_batch(frm, to, scene, margin, MAXS, check_target=True, want_carry=True, round_budget=32)]
        _check_edges(got, w[0], w[1], w[2], w[3], w[5], occ)
        assert np.array_equal(got["blocked"], w[4])
        print("mode %d: scene margin %.2f blocks %d of %d edges" % (mode, margin, int(w[4].sum()), Q * K))
    # margin = -inf: the scene-less call
    free = _np(c.connect_batch(nodes, queries, K, check_target=True, max_states=MAXS, round_budget=32, scene=scene, margin=-np.inf))
    plain = _np(c.connect_batch(nodes, queries, K, check_target=True, max_states=MAXS, round_budget=32))
    _check_edges(free, plain["states"], plain["n_states"], plain["ok"], plain["newton_iters"], plain["carry"], occ)
    assert not free["blocked"].any() and not plain["blocked"].any()


def test_host_form_and_mirror(gpu_ctx):
    from closed_chain_motion_planner_amd import jy_ProjectedStateSpace

    c, nodes, queries, torch = _world(gpu_ctx, 0)
    dev = _np(c.connect_batch(nodes, queries, K, check_target=True, max_states=MAXS, round_budget=32))
    nd, qs = nodes.cpu().numpy(), queries.cpu().numpy()
    E = Q * K
    h = {"nbr_idx": np.zeros((Q, K), np.int32), "nbr_dist": np.zeros((Q, K)), "states": np.zeros((E, MAXS, 14)), "n_states": np.zeros(E, np.int32),
         "ok": np.zeros(E, np.uint8), "newton_iters": np.zeros(E, np.int32), "blocked": np.ones(E, np.uint8), "carry": np.zeros((E, 2))}
    dp, ip, bp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    _lib.check(_lib.lib().ccmp_connect_host(gpu_ctx.handle, C.byref(c.problem), None, 0.0, nd.ctypes.data_as(dp), N, qs.ctypes.data_as(dp), Q, K, 0, 0, 1, MAXS, 32,
                                            h["nbr_idx"].ctypes.data_as(ip), h["nbr_dist"].ctypes.data_as(dp), h["states"].ctypes.data_as(dp),
                                            h["n_states"].ctypes.data_as(ip), h["ok"].ctypes.data_as(bp), h["newton_iters"].ctypes.data_as(ip),
                                            h["blocked"].ctypes.data_as(bp), h["carry"].ctypes.data_as(dp)), "ccmp_connect_host")
    assert np.array_equal(h["nbr_idx"], dev["nbr_idx"]) and _same_bits(h["nbr_dist"], dev["nbr_dist"]) and not h["blocked"].any()
    _check_edges(h, dev["states"], dev["n_states"], dev["ok"], dev["newton_iters"], dev["carry"], np.ones(E, dtype=bool))
    # arguments: a round budget without carries, a one-entry list with carries
    assert _lib.lib().ccmp_connect_host(gpu_ctx.handle, C.byref(c.problem), None, 0.0, nd.ctypes.data_as(dp), N, qs.ctypes.data_as(dp), Q, K, 0, 0, 1, MAXS, 32,
                                        h["nbr_idx"].ctypes.data_as(ip), None, h["states"].ctypes.data_as(dp), h["n_states"].ctypes.data_as(ip),
                                        h["ok"].ctypes.data_as(bp), None, None, None) == -1
    # the mirror: the same neighbours; reached = the bool of the whole traversal (cut and suspended lists are continued there)
    space = jy_ProjectedStateSpace(c, max_states=64)
    assert np.array_equal(space.nearestK(nd, qs[0], K), dev["nbr_idx"][0])
    nbr, reached, lists = space.connectMilestones(nd, qs[:6], K, check_target=True)
    assert np.array_equal(nbr, dev["nbr_idx"][:6])
    whole = _np(c.connect_batch(nodes, queries[:6].contiguous(), K, check_target=True, max_states=64))
    done = whole["n_states"] <= 64
    assert done.sum() >= 10
    assert np.array_equal(reached.reshape(-1)[done], whole["ok"][done] == 1)
    for e in np.flatnonzero(done):
        assert _same_bits(lists[e // K][e % K], whole["states"][e, : whole["n_states"][e]])
