"""The planner-side steps — the plain analytic extend step, connect, grow and the store's poses, densify, shortcut and smooth (with and
without a scene) — on arms that are not the stock model (tests/arm_model_cases.py: tilted, calibrated, calibrated_tilted).  Their own suites
(test_gpu_connect.py, test_gpu_grow_store.py, test_gpu_pose_ik.py, test_gpu_dense.py, test_gpu_shortcut.py, test_gpu_smooth.py) run Wine_Bottle and the
recorded files, which is the stock model; the continuation loops of these calls hand carry and round_budget to whichever extend kernel
the model selects.  Bit for bit against the det oracle and against the composition of the entry points, uint64 views, NaN equal to NaN,
no tolerance; sizes and seeds from arm_model_cases (the seeds chosen in tests/test_arm_model_cases.py on the oracle alone).  The table
of what each test fills is at the top of tests/test_gpu_arm_models_scene.py.

Mutation check (the builds and the run are described there; none faulted or hung).  What failed here:
  ccmp_kernels_geo_scene.hip: the launcher always takes            test_connect_equals_its_parts_and_the_oracle[0-calibrated],
  CCMP_LAUNCH_GEO_SCENE(true)                                      test_densify_and_shortcut[0-calibrated-scene]
  ccmp_kernels_fast.hip: CCMP_LAUNCH_GEO_ROW16_SCENE always        test_connect_equals_its_parts_and_the_oracle[1-tilted],
  takes DIAG = true                                                test_densify_and_shortcut[1-tilted-scene]
  ccmp_clearance.h: the world transform takes K.base_R[0]          test_connect_equals_its_parts_and_the_oracle[0-tilted], [1-tilted]
  for both arms                                                    (test_densify_and_shortcut[*-tilted-scene] passes: the flags, list lengths and
                                                                   Newton totals of its eleven pairs stay)
  ccmp_kernels_scene.hip: likewise in clearance_kernel and         test_densify_and_shortcut[0-tilted-scene], [1-tilted-scene] (the margin and the
  clearance_state_kernel                                           clearance summary come from clearance_batch)
The plain analytic extend step, grow and the store's poses run no code these mutations touch (ccmp_ik.cpp is out of their scope).

test_smooth (smooth_paths, added after the units above): eight cases, 0.03 to 0.11 s each on the MI355X, 0.5 s together, of which the
restatement takes 0.01 to 0.04 s per case.  Mutation check of test_smooth alone, scratch builds, one run each, all wrong answers, none a
fault or a hang.  The world transform of the last two rows above is one text now (ccmp_scene_math.h: scene_base_to_world), so they are
one mutant:
  ccmp_kernels_geo_scene.hip: the launcher always takes            test_smooth[0-calibrated-scene]
  CCMP_LAUNCH_GEO_SCENE(true)
  ccmp_kernels_fast.hip: CCMP_LAUNCH_GEO_ROW16_SCENE always        test_smooth[1-tilted-scene]
  takes DIAG = true
  ccmp_scene_math.h: scene_base_to_world takes K.base_R[0]         test_smooth[0-tilted-scene], [1-tilted-scene]
  for both arms
  (test_smooth[*-plain] runs no scene kernel.)  The six mutants of csrc/ccmp_kernels_smooth.hip listed in tests/test_gpu_smooth_shapes.py:
  the bracket's fallback row, the gather's pair_path and the dropped guard of the length sum fail all eight cases; where[0] for where[f]
  in smooth_store_kernel or smooth_length_kernel fails the four scene cases (without a scene every active path of these four runs both
  passes, so all lie in the same buffer); clear_m at the wrong segment fails none of them (tests/test_gpu_smooth_shapes.py::
  test_scene_reads_the_incoming_midpoint holds that one)."""
import time

import numpy as np
import pytest

import arm_model_cases as A
from conftest import NCPU
from dense_path_cases import bits, join, oracle_segments, same_paths
from pose_ik_cases import pose_of
from shortcut_cases import expect, oracle_pairs, pairs_py, same_selection
from smooth_cases import BELOW, PROJECTED, REFUSED, Restatement, mirror_fill, same_result, scene_restatement
from smooth_cases import expect as smooth_expect
from test_gpu_analytic_extend import _same_lists
from test_gpu_connect import _check_edges, _gathered, _np, _same_bits
from test_gpu_geodesic_scene import OracleScene, _pick_margin
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu

N, Q, K, MAXS = 200, 9, 5, 16  # MAXS: test_gpu_connect's helpers read its own 16
RNG_SEED = 0x51CB


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


def _scene_and_margin(c, model, mode):
    """the default scene of the model and the margin of the scene extend test (test_gpu_arm_models_scene.test_extend_with_a_scene)"""
    from closed_chain_motion_planner_amd import scene as S

    sc = S.ProxyValidityChecker(c).scene
    frm, to = A.edges(c, A.E_SCENE, A.EXTEND_SEED[(model, mode)])
    return sc, _pick_margin(c, sc, frm, to, A.MS_SCENE)[0]


@pytest.mark.parametrize("model", ["calibrated", "calibrated_tilted"])
def test_plain_analytic_extend_on_calibrated_arms(gpu_ctx, oracle_det, model):
    """discrete_geodesic_batch in analytic mode (geodesic_row16_kernel, one launch): lists, counts, flags and Newton counts of 64 edges
    with lists of 8 equal the oracle's"""
    c = _constraint(A.OBJ, gpu_ctx, mode=1)
    E, ms = A.E_PLAIN, A.MS_PLAIN
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        assert P.jacobian_mode == 1
        frm, to = A.edges(c, E, A.PLAIN_SEED)
        st, n, ok, its = [x.cpu().numpy() for x in c.discrete_geodesic_batch(frm, to, ms)]
    so, no, oko, ito = oracle_det.discrete_geodesic_batch(P, frm.cpu().numpy(), to.cpu().numpy(), ms, NCPU)
    assert _same_lists(st, n, so, no, ms) and np.array_equal(ok, oko) and np.array_equal(its, ito)
    print("%s: %d of %d edges arrived, %d lists full" % (model, int((oko == 1).sum()), E, int((no > ms).sum())))
    assert 0 < int((oko == 1).sum()) < E  # both flags occur


def _world(c):
    q, ok, _, _ = c.sample_project_batch(0xC0ED, 0, 2048, want_iters=False)
    good = q[(ok != 0) & (c.joint_valid_batch(q) != 0)]
    assert good.shape[0] >= N + Q
    return good[:N].contiguous(), good[N: N + Q].contiguous()


@pytest.mark.parametrize("model", ["tilted", "calibrated"])
@pytest.mark.parametrize("mode", [0, 1])
def test_connect_equals_its_parts_and_the_oracle(gpu_ctx, oracle_det, mode, model):
    """connect_batch(scene=, margin=) = nearest_k_batch, then discrete_geodesic_scene_batch on the gathered pairs — without a round
    budget (four of its slots against the oracle directly) and with one (the resumable form); Roadmap.connect on the joint metric gives
    the same dict"""
    import torch
    from closed_chain_motion_planner_amd import Roadmap
    from closed_chain_motion_planner_amd._lib import METRIC_JOINT

    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        sc, margin = _scene_and_margin(c, model, mode)
        nodes, queries = _world(c)
        idx, dist = c.nearest_k_batch(nodes, queries, K)
        frm, to, occ = _gathered(nodes, queries, idx)
        assert occ.all()
        rm = Roadmap(c, capacity_hint=N)
        rm.append(joints=nodes)
        for budget in (0, 32):
            got = _np(c.connect_batch(nodes, queries, K, check_target=True, max_states=MAXS, round_budget=budget, scene=sc, margin=margin))
            w = [t.cpu().numpy() for t in c.discrete_geodesic_scene_batch(frm, to, sc, margin, MAXS, check_target=True, want_carry=True, round_budget=budget)]
            assert np.array_equal(got["nbr_idx"], idx.cpu().numpy()) and _same_bits(got["nbr_dist"], dist.cpu().numpy())
            _check_edges(got, w[0], w[1], w[2], w[3], w[5], occ)
            assert np.array_equal(got["blocked"], w[4])
            store = _np(rm.connect(queries, K, metric=METRIC_JOINT, check_target=True, max_states=MAXS, round_budget=budget, scene=sc, margin=margin))
            assert np.array_equal(store["nbr_idx"], got["nbr_idx"]) and np.array_equal(store["blocked"], got["blocked"])
            _check_edges(store, got["states"], got["n_states"], got["ok"], got["newton_iters"], got["carry"], occ)
            if budget == 0:
                whole = got
        torch.cuda.synchronize()
        rm.close()
    print("%s mode %d: margin %.6f, %d of %d edges reached, %d blocked" % (model, mode, margin, int((whole["ok"] == 1).sum()), Q * K, int(whole["blocked"].sum())))
    # the CPU checker directly, four slots: checkMotion's isSatisfied(to), then the traversal behind the validity callback
    orc = OracleScene(oracle_det, P, sc, margin)
    fn, tn = frm.cpu().numpy(), to.cpu().numpy()
    for e in range(0, Q * K, Q * K // 4)[:4]:
        assert oracle_det.is_satisfied(P, tn[e])  # the queries are valid projected states
        ok_o, st_o, n_o, its_o, c_o, bl_o, _ = orc.edge(fn[e], tn[e], MAXS)
        assert (whole["n_states"][e], whole["ok"][e], whole["newton_iters"][e], whole["blocked"][e]) == (n_o, ok_o, its_o, bl_o), e
        assert _same_bits(whole["states"][e, : min(n_o, MAXS)], st_o) and _same_bits(whole["carry"][e], c_o), e


@pytest.mark.parametrize("model", ["tilted", "calibrated"])
@pytest.mark.parametrize("mode", [0, 1])
def test_grow_and_the_store(gpu_ctx, oracle_det, mode, model):
    """the store's poses (pose_from_joints_kernel under the model) equal the oracle's compute_t_wo of the joints; Roadmap.grow for nine
    poses, one of them out of reach, equals the composition nearest_k -> pose_ik_batch -> discrete_geodesic_batch
    (test_gpu_pose_ik.test_grow_equals_the_composition on stock)"""
    import torch
    from closed_chain_motion_planner_amd import Roadmap

    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    k, ms = K, MAXS
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        nodes, queries = _world(c)
        rm = Roadmap(c, capacity_hint=N)
        rm.append(joints=nodes)
        joints, poses = rm.read()
        nodes_h = nodes.cpu().numpy()
        want = np.array([pose_of(oracle_det, P, x) for x in nodes_h])
        assert _same_bits(joints.cpu().numpy(), nodes_h) and _same_bits(poses.cpu().numpy(), want)
        # the targets: object poses of states that exist on this model (the queries'), the last one moved out of reach
        qp = np.array([pose_of(oracle_det, P, x) for x in queries.cpu().numpy()])
        qp[Q - 1, 0] += 10.0
        qpd = _dev(qp)
        out = rm.grow(qpd, k, rng_seed=RNG_SEED, first_index=5, max_states=ms)
        idx, dist = rm.nearest_k(qpd, k)
        seeds = joints[idx.long().clamp(min=0)].contiguous()
        ik = c.pose_ik_batch(qpd, seeds, rng_seed=RNG_SEED, first_index=5)
        torch.cuda.synchronize()
        assert torch.equal(out["nbr_idx"], idx) and torch.equal(out["nbr_dist"], dist)
        assert torch.equal(out["ik_ok"], ik["ok"]) and torch.equal(out["ik_which"], ik["which"])
        assert np.array_equal(out["q_new"].cpu().numpy().view(np.uint64), ik["q"].cpu().numpy().view(np.uint64))
        okq = ik["ok"].bool().cpu().numpy()
        print("%s mode %d: IK found a state for %d of %d poses" % (model, mode, int(okq.sum()), Q))
        assert okq[0] and not okq[Q - 1]
        for q in range(Q):
            rows = slice(q * k, (q + 1) * k)
            if not okq[q]:  # the empty-slot outputs
                for name in ("n_states", "ok", "newton_iters", "blocked"):
                    assert (out[name][rows] == 0).all(), name
                assert (out["carry"][rows] == 0).all() and torch.isnan(out["q_new"][q]).all()
                continue
            frm = joints[idx[q].long()].contiguous()
            to = ik["q"][q:q + 1].expand(k, 14).contiguous()
            states, n, ok, its = c.discrete_geodesic_batch(frm, to, max_states=ms)
            torch.cuda.synchronize()
            assert torch.equal(out["n_states"][rows], n) and torch.equal(out["ok"][rows], ok) and torch.equal(out["newton_iters"][rows], its)
            for e in range(k):
                m = min(int(n[e]), ms)
                assert torch.equal(out["states"][q * k + e, :m], states[e, :m])
            assert (out["blocked"][rows] == 0).all()
        rm.close()


def _zero_row_calls(c, pj_d, pl):
    """extend calls that contribute no row to their segment when every call stores one state (lists of 2, round budget 1): from plain
    discrete_geodesic_batch calls alone, as test_gpu_dense.test_ragged_chains counts them"""
    import torch

    sel = [(f, i) for f in range(len(pl)) for i in range(int(pl[f]) - 1)]
    frm = torch.stack([pj_d[f, i] for f, i in sel]).contiguous()
    to = torch.stack([pj_d[f, i + 1] for f, i in sel]).contiguous()
    s, n, ok, _, carry = c.discrete_geodesic_batch(frm, to, 2, want_carry=True, round_budget=1)
    zero_row, calls = 0, 1
    for _ in range(256):
        open_ = torch.nonzero((n > 2) | (ok == 2)).flatten()
        if open_.numel() == 0:
            break
        last = (n.clamp(max=2)[open_] - 1).long()
        frm, to = s[open_, last].contiguous(), to[open_].contiguous()
        s, n, ok, _, carry = c.discrete_geodesic_batch(frm, to, 2, carry_in=carry[open_].contiguous(), want_carry=True, round_budget=1)
        zero_row += int((n == 1).sum())
        calls += 1
    return zero_row, calls


@pytest.mark.parametrize("with_scene", [False, True], ids=["plain", "scene"])
@pytest.mark.parametrize("model", ["tilted", "calibrated"])
@pytest.mark.parametrize("mode", [0, 1])
def test_densify_and_shortcut(gpu_ctx, oracle_det, mode, model, with_scene):
    """four synthetic solution paths of 2, 3, 6 and 1 waypoints on the model's own manifold.  densify_paths with lists of 2, of 2 with
    one state per call (round budget 1: a segment that ends unreached behind a stored state ends in a call that contributes no row) and
    of 16 equals the oracle's uninterrupted segments joined by the rule's restatement; with a scene the rows stay and the clearance
    summary equals the oracle's clearance of the rows.  shortcut_paths(pairs=True) equals the oracle's checkMotion per pair (behind the
    validity callback with a scene) and the restated selection"""
    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        pj, pl = A.waypoint_paths(c, oracle_det, P, A.F_PATHS, A.L_PATHS, A.PATH_SEED[(model, mode)])
        pj_d, pl_d = _dev(pj), _dev(pl)
        sc, margin = _scene_and_margin(c, model, mode) if with_scene else (None, None)
        dense = [_np_all(c.densify_paths(pj_d, pl_d, scene=sc, margin=margin, chunk_states=ch, **kw))
                 for ch, kw in ((2, {}), (2, dict(round_budget=1)), (16, {}))]
        short = _np_all(c.shortcut_paths(pj_d, pl_d, scene=sc, margin=margin, pairs=True))
        short2 = _np_all(c.shortcut_paths(pj_d, pl_d, scene=sc, margin=margin, chunk_states=2, round_budget=1, pairs=True))
        zero_row, calls = _zero_row_calls(c, pj_d, pl) if not with_scene else (None, None)
    segs = oracle_segments(oracle_det, P, pj, pl)
    want = join(pj, pl, A.L_PATHS, segs)
    seg_ok = [s[0] for s in segs.values()]
    assert 0 in seg_ok and 1 in seg_ok
    for got, what in zip(dense, ("lists of 2", "lists of 2, one state per call", "lists of 16")):
        same_paths(got, want, (model, mode, with_scene, what))
    if not with_scene:
        print("%s mode %d: %d extend calls at one state per call, %d of them stored no new state" % (model, mode, calls, zero_row))
        assert zero_row >= 1 and calls == dense[1]["calls"]
    blocked = []
    orc = OracleScene(oracle_det, P, sc, margin) if with_scene else None
    if with_scene:
        clr_o = oracle_det.clearance_batch(P, sc.spheres, sc.boxes, sc.allowed, want["rows"])[0]
        pf = want["path_first"]
        for got in dense:
            assert np.array_equal(bits(got["clearance"]), bits(clr_o))
            for f in range(A.F_PATHS):
                v = clr_o[pf[f]: pf[f + 1]]
                below = np.flatnonzero(v < margin)
                assert bits(got["min_clear"][f: f + 1])[0] == bits(v.min())[0] and got["min_row"][f] == pf[f] + int(np.argmin(v))
                assert got["first_blocked"][f] == (pf[f] + int(below[0]) if len(below) else -1)
    ok, ns, nw = oracle_pairs(oracle_det, P, pj, pl, edge=A.scene_edge(orc, blocked) if with_scene else None)
    flags = [int(ok[f, i, j]) for f, i, j in pairs_py(pj, pl)]
    print("%s mode %d scene %d: seg_ok 1 / 0 = %d / %d, pair_ok 1 / 0 = %d / %d, blocked by the scene %d"
          % (model, mode, with_scene, seg_ok.count(1), seg_ok.count(0), flags.count(1), flags.count(0), sum(blocked)))
    assert 0 in flags and 1 in flags
    sel = expect(pj, pl, ok)
    for got, what in ((short, "default"), (short2, "lists of 2, one state per call")):
        for name, w in (("pair_ok", ok), ("pair_states", ns), ("pair_newton", nw)):
            assert np.array_equal(got[name], w), (model, mode, with_scene, what, name, np.argwhere(got[name] != w)[:5])
        same_selection(got, sel, (model, mode, with_scene, what))


def _np_all(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


@pytest.mark.parametrize("with_scene", [False, True], ids=["plain", "scene"])
@pytest.mark.parametrize("model", ["tilted", "calibrated"])
@pytest.mark.parametrize("mode", [0, 1])
def test_smooth(gpu_ctx, oracle_det, mode, model, with_scene):
    """smooth_paths on the four synthetic paths of the model's own manifold, two passes for a result of 21 vertices: the pass loop hands
    its own option struct to densify, the projector, the pair tests and clearance_batch, each of which chooses its kernel by the model.
    The device form at the defaults and with lists of 2 at one state per call, and the host form, equal the restatement on the oracle
    (with a scene: checkMotion behind the oracle's validity callback and the oracle's clearance of the midpoints and candidates)"""
    from closed_chain_motion_planner_amd import smooth_len_after

    assert smooth_len_after(A.L_PATHS, A.SMOOTH_STEPS) == A.SMOOTH_CAP
    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        pj, pl = A.waypoint_paths(c, oracle_det, P, A.F_PATHS, A.L_PATHS, A.SMOOTH_SEED[(model, mode)])
        pj_d, pl_d = _dev(pj), _dev(pl)
        sc, margin = _scene_and_margin(c, model, mode) if with_scene else (None, None)
        kw = dict(max_steps=A.SMOOTH_STEPS, out_max_len=A.SMOOTH_CAP, scene=sc, margin=margin, stats=True)
        got = [(c.smooth_paths(pj_d, pl_d, **kw), "device form"), (c.smooth_paths(pj_d, pl_d, chunk_states=2, round_budget=1, **kw), "lists of 2, one state per call"),
               (c.smooth_paths(pj, pl, **kw), "host form")]
    t = time.perf_counter()
    R = scene_restatement(oracle_det, P, sc, margin) if with_scene else Restatement(oracle_det, P)
    want = smooth_expect(R, pj, pl, A.SMOOTH_STEPS, 0.005, A.SMOOTH_CAP, mirror_fill(pj, A.SMOOTH_CAP))
    s = want["stats"].sum(axis=0)
    print("%s mode %d scene %d: moved %d, stats (projected, fallback, degenerate, refused, below) %s, stop %s; restated in %.2f s"
          % (model, mode, with_scene, want["moved"].sum(), s.tolist(), want["stop"].tolist(), time.perf_counter() - t))
    assert want["moved"].sum() >= 1 and s[REFUSED] + s[BELOW] >= 1 and s[PROJECTED] >= 1
    for g, what in got:
        same_result(g, want, (model, mode, with_scene, what))
