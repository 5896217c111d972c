"""Roadmap.grow(vet=True) (ccmp_roadmap_grow_vetted) against the composition of its parts on the store of tests/test_gpu_pose_ik.py — the
object-metric k-NN, the store's joint rows as seeds, ccmp_pose_ik_vetted_ref on the host, and the masked traversal through
ccmp_geodesic_scene_batch — bit for bit, in FD and in analytic mode.

The scene is the default skeleton scene at -0.03 with one more world sphere: 0.1 m around the left hand's target of the LAST of nine
poses.  Every solution of that arm overlaps it by 0.135 m, so the plain rule solves the pose and the vetted rule does not: its slots
must be empty (zeros, no NaN into a traversal).  Pose 0's nearest vertex is a pose-only one (a skipped slot)."""
import numpy as np
import pytest

import ik_vet_cases as V
from arm_model_cases import default_scene_host
from pose_ik_cases import hand_target, sampled_case
from test_gpu_pose_ik import OBJ, RNG_SEED, _constraint

pytestmark = pytest.mark.gpu
K, MS, MARGIN = 5, 16, V.DEFAULT_MARGIN
EDGE_NAMES = ("n_states", "ok", "newton_iters", "blocked", "carry")


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """the 1 300 vertices of test_gpu_pose_ik's store and one pose-only vertex 1e-4 from pose 0; the nine poses; the scene's proxies"""
    import torch

    c = _constraint(gpu_ctx, False)
    valid, _, targets = sampled_case(OBJ)[2:5]
    q, ok = c.sample_project_batch(0xB0B, 0, 12288, want_iters=False)[:2]
    jv = c.joint_valid_batch(q)
    more = q[(ok.bool() & jv.bool())][:1300 - len(valid[40:])]
    joints = torch.cat([torch.from_numpy(np.array(valid[40:])).cuda(), more]).contiguous()
    assert joints.shape[0] == 1300
    poses = np.array(targets[:9])
    near = poses[:1].copy()
    near[0, 0] += 1e-4
    sc = default_scene_host(c.problem)
    sc.spheres.append((-1, 19, tuple(float(v) for v in hand_target(c.problem, poses[8], 0)[1]), 0.1))
    torch.cuda.synchronize()
    return joints, poses, near, sc


def _store(gpu_ctx, world, mode):
    import torch
    from closed_chain_motion_planner_amd import ProxyScene, Roadmap

    joints, _, near, sc = world
    c = _constraint(gpu_ctx, False)
    c.setJacobianMode(mode)
    rm = Roadmap(c, capacity_hint=1301)
    rm.append(joints=joints)
    rm.append(None, torch.from_numpy(near).cuda())
    return c, rm, ProxyScene(c, sc.spheres, sc.boxes, sc.allowed)


@pytest.mark.parametrize("mode", [0, 1], ids=["fd", "analytic"])
@pytest.mark.parametrize("Q", [1, 9])
def test_grow_vetted_equals_the_composition(gpu_ctx, world, Q, mode):
    import torch
    from closed_chain_motion_planner_amd import pose_ik_ref, pose_ik_vetted_ref

    joints, poses, _, sc = world
    c, rm, scene = _store(gpu_ctx, world, mode)
    qp = poses[:Q]
    qpd = torch.from_numpy(qp).cuda()
    out = rm.grow(qpd, K, rng_seed=RNG_SEED, first_index=5, max_states=MS, scene=scene, margin=MARGIN, vet=True)
    torch.cuda.synchronize()
    # the composition
    idx, dist = rm.nearest_k(qpd, K)
    sj, _ = rm.read()
    seeds = sj[idx.long()].contiguous().cpu().numpy()
    assert (idx >= 0).all() and idx[0, 0].item() == 1300 and np.isnan(seeds[0, 0]).all() and np.isfinite(seeds[:, 1:]).all()
    ik = pose_ik_vetted_ref(c.problem, qp, seeds, sc.spheres, sc.boxes, sc.allowed, MARGIN, rng_seed=RNG_SEED, first_index=5)
    assert torch.equal(out["nbr_idx"], idx) and torch.equal(out["nbr_dist"], dist)
    assert np.array_equal(out["ik_ok"].cpu().numpy(), ik["ok"]) and np.array_equal(out["ik_which"].cpu().numpy(), ik["which"])
    assert np.array_equal(_bits(out["q_new"]), _bits(ik["q"])) and np.array_equal(_bits(out["ik_clearance"]), _bits(ik["clearance"]))
    assert ik["ok"][0] and ik["which"][0] >= 1  # the pose-only slot was skipped
    if Q == 9:  # the vetting, not the solver, fails the last pose
        assert not ik["ok"][8] and np.isnan(ik["clearance"][8]) and pose_ik_ref(c.problem, qp[8:], seeds[8:], rng_seed=RNG_SEED, first_index=13)["ok"][0]
    got = {k: v.cpu().numpy() for k, v in out.items()}
    masked = np.where(ik["ok"][:, None].astype(bool) & np.isfinite(seeds).all(axis=2), idx.cpu().numpy(), -1).reshape(-1)
    live = masked >= 0
    frm = sj[torch.from_numpy(masked[live]).cuda().long()].contiguous()
    to = torch.from_numpy(np.repeat(ik["q"], K, axis=0)[live]).cuda()
    w = [t.cpu().numpy() for t in c.discrete_geodesic_scene_batch(frm, to, scene, MARGIN, MS, check_target=False, want_carry=True)]
    want = {"states": w[0], "n_states": w[1], "ok": w[2], "newton_iters": w[3], "blocked": w[4], "carry": w[5]}
    for i, e in enumerate(np.flatnonzero(live)):
        for name in EDGE_NAMES:
            assert np.array_equal(_bits(got[name][e]), _bits(want[name][i])), (name, e)
        m = min(int(want["n_states"][i]), MS)
        assert m >= 1 and np.array_equal(_bits(got["states"][e, :m]), _bits(want["states"][i, :m])), ("states", e)
    for name in EDGE_NAMES:  # an empty slot never ran: zeros
        assert not got[name][~live].any(), name
    assert not live[0] and live[1:K].all() and (Q == 1 or not live[8 * K:].any())
    # the plain call on the same store answers the last pose; with vet=False the mirror makes today's call
    plain = rm.grow(qpd, K, rng_seed=RNG_SEED, first_index=5, max_states=MS, scene=scene, margin=MARGIN)
    torch.cuda.synchronize()
    assert "ik_clearance" not in plain and (Q == 1 or plain["ik_ok"][8].item() == 1)
    if Q == 1:
        host = rm.grow(qp, K, rng_seed=RNG_SEED, first_index=5, max_states=MS, scene=scene, margin=MARGIN, vet=True)  # the host form
        for name in got:
            if name != "states":
                assert np.array_equal(_bits(host[name]), _bits(got[name])), name
    rm.close()
    scene.close()
