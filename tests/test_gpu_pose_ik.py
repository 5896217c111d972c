"""Pose-targeted IK on the device (ik_solve_kernel, ik_select_kernel; ccmp_roadmap_grow) against the same text on the host.

ccmp_pose_ik_ref is the checker: one text (csrc/ccmp_ik.h) in one rounding model, so every output is compared BIT FOR BIT — q as
uint64 views, ok, which, every candidate's last iterate and round count.  Shapes: 1, 3 and 70 targets x 1 and 5 seed slots x 0, 14
and 31 restarts — two lanes, ragged last wavefronts, several blocks per arm — on the stock arms and on calibrated ones (the general
instantiation).  A call over 70 targets equals 70 calls over one.  Roadmap.grow equals the composition of the existing entry points."""
import ctypes as C

import numpy as np
import pytest

from conftest import config_path
from pose_ik_cases import sampled_case

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
RNG_SEED = 0x51CA


def _constraint(ctx, calibrated):
    from closed_chain_motion_planner_amd import KinematicChainConstraint, _lib

    c = KinematicChainConstraint.from_yaml(config_path(OBJ), ctx=ctx)
    if calibrated:
        for arm in (0, 1):
            dh = (C.c_double * 28)(*[1e-3 * ((5 * i + 2 * arm) % 7 - 3) for i in range(28)])
            assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
        c.setInitialPosition(np.array(c.problem.start_joint[:]))
    return c


def _inputs(T, S):
    """T targets (the 40 sample-derived ones, then further valid states' poses) and their S nearest seeds; one slot of the last target
    is NaN when there is more than one, so a skipped slot is part of every comparison"""
    _, _, valid, poses, targets, seeds = sampled_case(OBJ)
    tp = np.array(poses[:T])  # (a writable copy: the shared arrays are read-only)
    sd = np.empty((T, S, 14))
    sd[:min(T, 40)] = seeds[:T, :S]
    for t in range(40, T):
        sd[t] = valid[[(7 * t + 13 * s) % len(valid) for s in range(S)]]  # arbitrary valid states: mostly far seeds, the restarts' work
    if S > 1:
        sd[T - 1, 0, 5] = np.nan
    return tp, sd


def _same(dev, ref):
    import torch

    for name in ("q", "cand_q"):
        assert np.array_equal(dev[name].cpu().numpy().view(np.uint64), ref[name].view(np.uint64)), name
    for name in ("ok", "which", "cand_rounds"):
        assert np.array_equal(dev[name].cpu().numpy(), ref[name]), name
    assert torch.cuda.is_available()


@pytest.mark.parametrize("calibrated", [False, True], ids=["stock", "calibrated"])
@pytest.mark.parametrize("R", [0, 14, 31])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("T", [1, 3, 70])
def test_bit_for_bit_against_the_host_form(gpu_ctx, T, S, R, calibrated):
    import torch
    from closed_chain_motion_planner_amd import ik_options, pose_ik_ref

    c = _constraint(gpu_ctx, calibrated)
    tp, sd = _inputs(T, S)
    opts = ik_options(restarts=R)
    ref = pose_ik_ref(c.problem, tp, sd, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True)
    dev = c.pose_ik_batch(torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda(), rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True)
    torch.cuda.synchronize()
    _same(dev, ref)
    if T == 70 and S == 5 and R == 14 and not calibrated:
        assert ref["ok"].sum() >= 40 and (ref["cand_rounds"] == -1).any() and (ref["cand_rounds"] == -2).any() and (ref["cand_rounds"] > 0).any()
    host = c.pose_ik_batch(tp, sd, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=(T == 3))  # the host form: the same launches
    for name in host:
        assert np.array_equal(host[name].view(np.uint8), ref[name].view(np.uint8)), name


def test_batch_invariance(gpu_ctx):
    """70 calls over one target with the matching first_index give the rows of one call over 70"""
    import torch

    c = _constraint(gpu_ctx, False)
    tp, sd = _inputs(70, 5)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    whole = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=1000, want_candidates=True)
    parts = [c.pose_ik_batch(tpd[t:t + 1], sdd[t:t + 1], rng_seed=RNG_SEED, first_index=1000 + t, want_candidates=True) for t in range(70)]
    torch.cuda.synchronize()
    for name in whole:
        a = whole[name].cpu().numpy()
        b = np.concatenate([p[name].cpu().numpy() for p in parts])
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    other = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=0, want_candidates=True)  # the restarts do follow first_index
    assert not np.array_equal(other["cand_q"][:, :, :, 1:].cpu().numpy(), whole["cand_q"][:, :, :, 1:].cpu().numpy())
    assert np.array_equal(other["cand_q"][:, :, :, 0].cpu().numpy().view(np.uint64), whole["cand_q"][:, :, :, 0].cpu().numpy().view(np.uint64))


def test_argument_checks_come_before_any_launch(gpu_ctx):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, ik_options

    c = _constraint(gpu_ctx, False)
    tp, sd = _inputs(1, 1)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    for bad in (dict(restarts=32), dict(max_rounds=0), dict(eps=-1.0)):
        with pytest.raises(CcmpError) as e:
            c.pose_ik_batch(tpd, sdd, opts=ik_options(**bad))
        assert e.value.code == -1
    with pytest.raises(CcmpError) as e:
        c.pose_ik_batch(torch.zeros((1, 8), dtype=torch.float64).cuda(), torch.zeros((1, 17, 14), dtype=torch.float64).cuda())
    assert e.value.code == -1
    far = tp.copy()
    far[0, 2] += 10.0  # a target out of reach: a defined value, within max_rounds
    out = c.pose_ik_batch(torch.from_numpy(far).cuda(), sdd, want_candidates=True)
    assert out["ok"].item() == 0 and out["which"].item() == -1 and torch.isnan(out["q"]).all() and (out["cand_rounds"] == -1).all()


@pytest.fixture(scope="module")
def store(gpu_ctx):
    """1 300 vertices: the object's valid sampled states, then states the projector samples on the device"""
    import torch
    from closed_chain_motion_planner_amd import Roadmap

    c = _constraint(gpu_ctx, False)
    valid = sampled_case(OBJ)[2]
    q, ok = c.sample_project_batch(0xB0B, 0, 12288, want_iters=False)[:2]
    jv = c.joint_valid_batch(q)
    more = q[(ok.bool() & jv.bool())][:1300 - len(valid[40:])]
    joints = torch.cat([torch.from_numpy(np.array(valid[40:])).cuda(), more])
    assert joints.shape[0] == 1300
    rm = Roadmap(c, capacity_hint=1300)
    rm.append(joints=joints)
    torch.cuda.synchronize()
    return c, rm


@pytest.mark.parametrize("Q", [1, 9])
def test_grow_equals_the_composition(store, Q):
    import torch

    c, rm = store
    k, ms = 5, 16
    targets = sampled_case(OBJ)[4]
    qp = np.array(targets[:Q])
    if Q > 1:
        qp[Q - 1, 0] += 10.0  # a pose without a solution: empty slots
    qpd = torch.from_numpy(qp).cuda()
    out = rm.grow(qpd, k, rng_seed=RNG_SEED, first_index=5, max_states=ms)
    torch.cuda.synchronize()
    # the composition of the existing entry points
    idx, dist = rm.nearest_k(qpd, k)
    joints, _ = rm.read()
    seeds = joints[idx.long().clamp(min=0)].contiguous()
    ik = c.pose_ik_batch(qpd, seeds, rng_seed=RNG_SEED, first_index=5)
    torch.cuda.synchronize()
    assert torch.equal(out["nbr_idx"], idx) and torch.equal(out["nbr_dist"], dist)
    assert torch.equal(out["ik_ok"], ik["ok"]) and torch.equal(out["ik_which"], ik["which"])
    assert np.array_equal(out["q_new"].cpu().numpy().view(np.uint64), ik["q"].cpu().numpy().view(np.uint64))
    okq = ik["ok"].bool().cpu().numpy()
    assert okq[0] and (Q == 1 or not okq[Q - 1])
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
