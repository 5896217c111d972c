"""Pose-targeted IK on the device on arms that are not the stock model (tests/arm_model_cases.py): tilted — the stock instantiation of
ik_solve_kernel with a non-diagonal base frame, which no host form runs (ccmp_pose_ik_ref is the general one) —, calibrated_tilted and
general_kernels.  tests/test_gpu_pose_ik.py and tests/test_gpu_ik_vet.py run stock and calibrated arms on targets sampled on the stock
model; here every model solves targets sampled on its own manifold (pose_ik_cases.sampled_case(obj, model)).

  plain rule    pose_ik_batch equals ccmp_pose_ik_ref bit for bit — q, ok, which, every candidate's last iterate and round count — at
                T = 3 and 40 targets x 5 seed slots x 0 and 14 restarts (a ragged last wavefront, several blocks per arm), one slot of the
                last target NaN; the host form of the call at T = 3.
  one step      with max_rounds = 1 the device's records are compared DIRECTLY with pose_ik_cases.restated_step on the oracle's forward
                kinematics, not through the host form: candidate 0 of every fourth target's slots and the first and the last restart
                of one slot each (started from pose_ik_cases.restart_start), at T = 40, R = 14.  The tolerance is measured here, on these
                rows: 200 x the largest difference between the restatement at difference step sizes 2e-3 and 4e-3, at most 1e-6
                (pose_ik_cases.step_tolerance).  Measured on an MI355X, 138 rows of which 40 restarts: reference spread 8.9e-12,
                tolerance 1.8e-9, device - restatement 8.7e-12 (tilted); 9.4e-12, 1.9e-9, 7.7e-12 (calibrated_tilted).
  vetted rule   tests/test_gpu_ik_vet.py's comparison with ccmp_pose_ik_vetted_ref at T = 3, R = 14 on the model's default scene.
  grow          Roadmap.grow(vet=True) on tilted arms equals the composition of its parts (tests/test_gpu_grow_vetted.py on stock): nine
                poses, one of them out of reach.

Mutation check: tests/test_pose_ik_models_host.py (the mutations are of csrc/ccmp_ik.h, which host and device share; the host module
names what fails).  Here test_one_step_on_the_device fails for the same reasons as its host counterpart under (a), (b), (c), (d) and (f),
and its restart rows under (e); the bit-for-bit tests compare one text with itself and cannot."""
import numpy as np
import pytest

import arm_model_cases as A
import ik_vet_cases as V
import pose_ik_cases as K
from pose_ik_cases import pose_of
from test_gpu_arm_models_planner import _world
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
OBJ = A.OBJ
RNG_SEED = 0x51CC
S = 5
VET_KEYS = ("q", "ok", "which", "clearance", "cand_q", "cand_rounds", "cand_clear", "slot_clear")


def _inputs(model, T):
    """the first T of the model's own 40 targets and their 5 pose-nearest seeds; one slot of the last target is NaN"""
    targets, seeds = K.sampled_case(OBJ, model)[4:]
    tp, sd = np.array(targets[:T]), np.array(seeds[:T, :S])
    sd[T - 1, 0, 5] = np.nan
    return tp, sd


def _bytes(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def _same(dev, ref, keys):
    for k in keys:
        assert np.array_equal(_bytes(dev[k]), _bytes(ref[k])), k


@pytest.mark.parametrize("model", ["tilted", "calibrated_tilted", "general_kernels"])
@pytest.mark.parametrize("R", [0, 14])
@pytest.mark.parametrize("T", [3, 40])
def test_plain_rule_bit_for_bit(gpu_ctx, T, R, model):
    import torch
    from closed_chain_motion_planner_amd import ik_options, pose_ik_ref

    c = _constraint(OBJ, gpu_ctx)
    tp, sd = _inputs(model, T)
    opts = ik_options(restarts=R)
    keys = ("q", "ok", "which", "cand_q", "cand_rounds")
    with A.apply(c, gpu_ctx, model):
        assert bytes(c.problem) == bytes(K.model_problem(OBJ, model))  # the targets were sampled on this very model
        ref = pose_ik_ref(c.problem, tp, sd, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True)
        dev = c.pose_ik_batch(torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda(), rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True)
        torch.cuda.synchronize()
        _same(dev, ref, keys)
        if T == 3:
            host = c.pose_ik_batch(tp, sd, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True)  # the host form: the same launches
            _same(host, ref, keys)
    rounds = ref["cand_rounds"]
    assert (rounds[T - 1, 0] == -2).all() and (rounds[:T - 1] != -2).all()
    if T == 40 and R == 14:
        print("%s: %d of %d targets solved" % (model, int(ref["ok"].sum()), T))
        assert ref["ok"].sum() >= 30 and (rounds == -1).any() and (rounds > 0).any()


@pytest.mark.parametrize("model", ["tilted", "calibrated_tilted"])
def test_one_step_on_the_device(gpu_ctx, model):
    import torch
    from closed_chain_motion_planner_amd import ik_options

    T, R, FIRST = 40, 14, 11
    c = _constraint(OBJ, gpu_ctx)
    orc, OP = K.sampled_case(OBJ, model)[:2]
    tp, sd = _inputs(model, T)
    opts = ik_options(restarts=R, max_rounds=1)
    with A.apply(c, gpu_ctx, model):
        assert bytes(c.problem) == bytes(K.model_problem(OBJ, model))
        dev = c.pose_ik_batch(torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda(), rng_seed=RNG_SEED, first_index=FIRST, opts=opts, want_candidates=True)
        torch.cuda.synchronize()
    cq, cr = dev["cand_q"].cpu().numpy(), dev["cand_rounds"].cpu().numpy()
    assert (cr[T - 1, 0] == -2).all() and np.isnan(cq[T - 1, 0]).all() and (cr[:T - 1] != -2).all()
    lo, hi = K.joint_box(OP)
    where, items = [], []
    for t in range(3, T, 4):  # every fourth target, the last one among them
        for s in range(S):
            if cr[t, s, 0, 0] == -2:
                continue
            cands = [0] + ([1, R] if s == t % S else [])
            starts = {r: K.restart_start(orc, OP, opts, RNG_SEED, FIRST, t, s, S, r) for r in cands if r > 0}
            for a in (0, 1):
                for r in cands:
                    if cr[t, s, a, r] == 0:  # converged at once: no step was taken
                        continue
                    q0 = np.clip(sd[t, s, 7 * a:7 * a + 7], lo, hi) if r == 0 else starts[r][7 * a:7 * a + 7]
                    where.append((t, s, a, r))
                    items.append((a, tp[t], q0))
    fine = np.array([K.restated_step(orc, OP, a, pose, q, opts, K.H_FINE)[0] for a, pose, q in items])
    coarse = np.array([K.restated_step(orc, OP, a, pose, q, opts, K.H_COARSE)[0] for a, pose, q in items])
    tol, spread = K.step_tolerance(fine, coarse)
    got = np.array([cq[t, s, a, r] for t, s, a, r in where])
    worst = float(np.abs(got - fine).max())
    n_restart = sum(1 for w in where if w[3] > 0)
    print("%s: %d rows (%d of them restarts), reference spread %.3g, tolerance %.3g, device - restatement %.3g" % (model, len(where), n_restart, spread, tol, worst))
    assert len(where) >= 100 and n_restart >= 30
    assert worst <= tol, (worst, tol, [where[i] for i in np.flatnonzero(np.abs(got - fine).max(axis=1) > tol)[:8]])


@pytest.mark.parametrize("model", ["tilted", "calibrated_tilted"])
def test_vetted_bit_for_bit(gpu_ctx, model):
    import torch
    from closed_chain_motion_planner_amd import ProxyScene, ik_options, pose_ik_vetted_ref

    T, R = 3, 14
    c = _constraint(OBJ, gpu_ctx)
    tp, sd = _inputs(model, T)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    opts = ik_options(restarts=R)
    refused = solved = 0
    with A.apply(c, gpu_ctx, model):
        sc = A.default_scene_host(c.problem)
        scene = ProxyScene(c, sc.spheres, sc.boxes, sc.allowed)
        for margin in (V.DEFAULT_MARGIN, 0.05):  # the skeleton scene's own margin, and one near the median clearance of the model's answers
            kw = dict(rng_seed=RNG_SEED, first_index=11, opts=opts)
            ref = pose_ik_vetted_ref(c.problem, tp, sd, sc.spheres, sc.boxes, sc.allowed, margin, want_candidates=True, **kw)
            dev = c.pose_ik_batch(tpd, sdd, want_candidates=True, scene=scene, margin=margin, **kw)
            torch.cuda.synchronize()
            _same(dev, ref, VET_KEYS)
            lean = c.pose_ik_batch(tpd, sdd, scene=scene, margin=margin, **kw)  # without the nullable outputs
            torch.cuda.synchronize()
            _same(lean, ref, ("q", "ok", "which", "clearance"))
            host = c.pose_ik_batch(tp, sd, want_candidates=True, scene=scene, margin=margin, **kw)
            _same(host, ref, VET_KEYS)
            refused += int(((ref["cand_rounds"] >= 0) & ~(ref["cand_clear"] > margin)).sum())
            solved += int(ref["ok"].sum())
        scene.close()
    assert refused > 0 and solved > 0  # the scene refuses converged candidates, and targets are solved all the same


@pytest.mark.parametrize("mode", [0, 1], ids=["fd", "analytic"])
def test_grow_vetted_on_tilted_arms(gpu_ctx, oracle_det, mode):
    """tests/test_gpu_grow_vetted.py's composition — the object-metric k-NN, the store's joint rows as seeds, ccmp_pose_ik_vetted_ref on the
    host, the masked traversal through discrete_geodesic_scene_batch — on a store of 200 states of the tilted model"""
    import torch
    from closed_chain_motion_planner_amd import ProxyScene, Roadmap, pose_ik_vetted_ref

    k, ms, margin, Q = 5, 16, V.DEFAULT_MARGIN, 9
    names = ("n_states", "ok", "newton_iters", "blocked", "carry")
    c = _constraint(OBJ, gpu_ctx, mode=mode)
    with A.apply(c, gpu_ctx, "tilted"):
        P = _oracle_problem(oracle_det, c)
        nodes, queries = _world(c)
        qp = np.array([pose_of(oracle_det, P, x) for x in queries.cpu().numpy()])
        qp[Q - 1, 0] += 10.0  # out of reach
        qpd = torch.from_numpy(qp).cuda()
        sc = A.default_scene_host(c.problem)
        scene = ProxyScene(c, sc.spheres, sc.boxes, sc.allowed)
        rm = Roadmap(c, capacity_hint=len(nodes))
        rm.append(joints=nodes)
        out = rm.grow(qpd, k, rng_seed=RNG_SEED, first_index=5, max_states=ms, scene=scene, margin=margin, vet=True)
        torch.cuda.synchronize()
        idx, dist = rm.nearest_k(qpd, k)
        sj, _ = rm.read()
        seeds = sj[idx.long()].contiguous().cpu().numpy()
        assert (idx >= 0).all() and np.isfinite(seeds).all()
        ik = pose_ik_vetted_ref(c.problem, qp, seeds, sc.spheres, sc.boxes, sc.allowed, margin, rng_seed=RNG_SEED, first_index=5)
        assert torch.equal(out["nbr_idx"], idx) and torch.equal(out["nbr_dist"], dist)
        assert np.array_equal(out["ik_ok"].cpu().numpy(), ik["ok"]) and np.array_equal(out["ik_which"].cpu().numpy(), ik["which"])
        assert np.array_equal(_bytes(out["q_new"]), _bytes(ik["q"])) and np.array_equal(_bytes(out["ik_clearance"]), _bytes(ik["clearance"]))
        print("tilted mode %d: the vetted IK found a state for %d of %d poses" % (mode, int(ik["ok"].sum()), Q))
        assert ik["ok"][:Q - 1].sum() >= 4 and not ik["ok"][Q - 1] and np.isnan(ik["clearance"][Q - 1])
        got = {n: v.cpu().numpy() for n, v in out.items()}
        live = np.repeat(ik["ok"].astype(bool), k)
        frm = sj[idx.reshape(-1)[torch.from_numpy(live).cuda()].long()].contiguous()
        to = torch.from_numpy(np.repeat(ik["q"], k, axis=0)[live]).cuda()
        w = [t.cpu().numpy() for t in c.discrete_geodesic_scene_batch(frm, to, scene, margin, ms, check_target=False, want_carry=True)]
        want = {"states": w[0], "n_states": w[1], "ok": w[2], "newton_iters": w[3], "blocked": w[4], "carry": w[5]}
        for i, e in enumerate(np.flatnonzero(live)):
            for name in names:
                assert np.array_equal(_bytes(got[name][e]), _bytes(want[name][i])), (name, e)
            m = min(int(want["n_states"][i]), ms)
            assert m >= 1 and np.array_equal(_bytes(got["states"][e, :m]), _bytes(want["states"][i, :m])), ("states", e)
        for name in names:  # an empty slot never ran: zeros
            assert not got[name][~live].any(), name
        assert not live[(Q - 1) * k:].any() and torch.isnan(out["q_new"][Q - 1]).all()
        rm.close()
        scene.close()
