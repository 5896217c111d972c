"""The vetted IK on the device (ik_vet_kernel, ik_assemble_kernel, ik_pick_kernel) against the same text on the host.

ccmp_arm_clearance_ref and ccmp_pose_ik_vetted_ref are the checkers — one text (csrc/ccmp_ik_vet.h) in one rounding model, so every
output is compared BIT FOR BIT — and the arm clearance is also compared with ccmp_clearance_batch on the sub-scene without the other
arm's moving spheres.  Batches are ragged against ik_vet_kernel's four rows per wavefront; the scenes are those of
tests/test_ik_vet_ref.py: per-arm pair counts around the sixteen-lane stride, the largest scene the pair rule admits, the default
skeleton scene and the scenes built from the plain run's records.  The arm clearance runs on every arm model of
tests/arm_model_cases.py; the vetted rule on the tilted ones is in tests/test_gpu_pose_ik_models.py."""
import ctypes as C

import numpy as np
import pytest

import ik_vet_cases as V
from arm_model_cases import default_scene_host, tilt
from test_gpu_pose_ik import _constraint, _inputs

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
RNG_SEED = 0x51CA
BATCHES = (1, 3, 4, 5, 63, 64, 65, 257)
VET_KEYS = ("q", "ok", "which", "clearance", "cand_q", "cand_rounds", "cand_clear", "slot_clear")


def _scene(c, sc):
    from closed_chain_motion_planner_amd import ProxyScene

    return ProxyScene(c, sc.spheres, sc.boxes, sc.allowed)


def _bytes(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint8)


def _same(dev, ref, keys=VET_KEYS):
    for k in keys:
        assert np.array_equal(_bytes(dev[k]), _bytes(ref[k])), k


@pytest.mark.parametrize("model", ["stock", "calibrated", "tilted", "calibrated_tilted"])
def test_arm_clearance_bit_for_bit(gpu_ctx, oracle_det, model):
    import torch
    from closed_chain_motion_planner_amd import ProxyScene
    from closed_chain_motion_planner_amd.scene import arm_clearance_ref

    c = _constraint(gpu_ctx, model in ("calibrated", "calibrated_tilted"))
    if model in ("tilted", "calibrated_tilted"):
        tilt(c)  # arm 1 on a rotated base: the world transform of its frames is the general one
    OP = oracle_det.problem_from_bytes(bytes(c.problem))
    n = max(BATCHES)
    q7 = V.candidates(oracle_det, OP, n)
    q7[2, 4] = np.nan  # a row that is not finite: NaN, never free
    q7d = torch.from_numpy(q7).cuda()
    for name in V.ARM_SCENES:
        spheres, boxes, allowed = V.arm_scene(name)
        full = ProxyScene(c, spheres, boxes, allowed)
        for arm in (0, 1):
            want, want_free = arm_clearance_ref(c.problem, spheres, boxes, allowed, arm, q7, margin=0.02)
            sub = ProxyScene(c, V.sub_scene(spheres, arm), boxes, allowed)
            assert sub.num_pairs == V.arm_pairs(spheres, boxes, allowed, arm)
            by_state = sub.clearance_batch(torch.from_numpy(V.state_of(c.problem, arm, q7)).cuda(), want_pair=False)[0]
            assert np.array_equal(_bytes(by_state), _bytes(want)), (name, arm)
            for B in BATCHES:
                clr, free = full.arm_clearance_batch(arm, q7d[:B].contiguous(), margin=0.02)
                torch.cuda.synchronize()
                assert np.array_equal(_bytes(clr), _bytes(want[:B])), (name, arm, B)
                assert np.array_equal(free.cpu().numpy(), want_free[:B]), (name, arm, B)
            sub.close()
        host = full.arm_clearance_batch(1, q7[:5], margin=0.02)  # the host form: the same launch
        assert np.array_equal(_bytes(host[0]), _bytes(want[:5])) and np.array_equal(host[1], want_free[:5])
        full.close()


@pytest.mark.parametrize("calibrated", [False, True], ids=["stock", "calibrated"])
@pytest.mark.parametrize("R", [0, 14])
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("T", [1, 3, 70])
def test_vetted_bit_for_bit_against_the_host_form(gpu_ctx, T, S, R, calibrated):
    import torch
    from closed_chain_motion_planner_amd import ik_options, pose_ik_vetted_ref

    c = _constraint(gpu_ctx, calibrated)
    tp, sd = _inputs(T, S)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    opts = ik_options(restarts=R)
    scenes = {"default": (default_scene_host(c.problem), V.DEFAULT_MARGIN)}
    scenes.update({k: (sc, 0.0) for k, (sc, _) in V.branch_scenes(OBJ).items()})
    solved = 0
    for name, (sc, margin) in scenes.items():
        ref = pose_ik_vetted_ref(c.problem, tp, sd, sc.spheres, sc.boxes, sc.allowed, margin, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True)
        scene = _scene(c, sc)
        dev = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True, scene=scene, margin=margin)
        torch.cuda.synchronize()
        _same(dev, ref)
        lean = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=11, opts=opts, scene=scene, margin=margin)  # without the nullable outputs
        torch.cuda.synchronize()
        _same(lean, ref, ("q", "ok", "which", "clearance"))
        if T == 3:
            host = c.pose_ik_batch(tp, sd, rng_seed=RNG_SEED, first_index=11, opts=opts, want_candidates=True, scene=scene, margin=margin)
            _same(host, ref)
        solved += int(ref["ok"].sum())
        scene.close()
    if T == 70 and S == 5 and R == 14:
        assert solved > 0


def test_the_constructed_scenes_reach_every_branch_on_the_device(gpu_ctx):
    """the 40-target inputs the scenes (a), (b), (c) were built from, on the device: the host form's bits, hence its branches"""
    import torch

    c = _constraint(gpu_ctx, False)
    P, targets, seeds, plain = V.plain_run(OBJ)
    assert bytes(P) == bytes(c.problem)
    tpd, sdd = torch.from_numpy(np.array(targets)).cuda(), torch.from_numpy(np.array(seeds)).cuda()
    counts = dict.fromkeys("abcd", 0)
    for name, (sc, _) in V.branch_scenes(OBJ).items():
        ref = V.vetted_ref(OBJ, sc, 0.0)
        scene = _scene(c, sc)
        dev = c.pose_ik_batch(tpd, sdd, rng_seed=V.RNG_SEED, want_candidates=True, scene=scene, margin=0.0)
        torch.cuda.synchronize()
        _same(dev, ref)
        for k in V.kinds(plain, {n: dev[n].cpu().numpy() for n in VET_KEYS}, 0.0):
            for x in k:
                counts[x] += 1
        scene.close()
    assert all(counts[x] > 0 for x in "abcd"), counts


def test_margin_minus_infinity_is_the_plain_call(gpu_ctx):
    import torch

    c = _constraint(gpu_ctx, False)
    tp, sd = _inputs(70, 5)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    scene = _scene(c, default_scene_host(c.problem))
    plain = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=3, want_candidates=True)
    low = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=3, want_candidates=True, scene=scene, margin=-np.inf)
    high = c.pose_ik_batch(tpd, sdd, rng_seed=RNG_SEED, first_index=3, scene=scene, margin=np.inf)
    torch.cuda.synchronize()
    _same(low, plain, ("q", "ok", "which", "cand_q", "cand_rounds"))
    assert plain["ok"].sum() >= 40
    assert not high["ok"].any() and (high["which"] == -1).all() and torch.isnan(high["q"]).all() and torch.isnan(high["clearance"]).all()


def test_batch_invariance(gpu_ctx):
    """70 calls over one target with the matching first_index give the rows of one call over 70"""
    import torch

    c = _constraint(gpu_ctx, False)
    tp, sd = _inputs(70, 5)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    scene = _scene(c, default_scene_host(c.problem))
    kw = dict(rng_seed=RNG_SEED, want_candidates=True, scene=scene, margin=V.DEFAULT_MARGIN)
    whole = c.pose_ik_batch(tpd, sdd, first_index=1000, **kw)
    parts = [c.pose_ik_batch(tpd[t:t + 1], sdd[t:t + 1], first_index=1000 + t, **kw) for t in range(70)]
    torch.cuda.synchronize()
    for name in whole:
        assert np.array_equal(_bytes(whole[name]), np.concatenate([_bytes(p[name]) for p in parts])), name
    assert 0 < int(whole["ok"].sum()) and (whole["cand_clear"] == -np.inf).any()


def test_argument_checks_come_before_any_launch(gpu_ctx):
    import torch
    from closed_chain_motion_planner_amd import CcmpError, _lib, ik_options

    c = _constraint(gpu_ctx, False)
    tp, sd = _inputs(1, 1)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    scene = _scene(c, default_scene_host(c.problem))
    for bad in (dict(opts=ik_options(restarts=32)), dict(opts=ik_options(max_rounds=0)), dict(margin=float("nan"))):
        with pytest.raises(CcmpError) as e:
            c.pose_ik_batch(tpd, sdd, scene=scene, **bad)
        assert e.value.code == -1
    with pytest.raises(CcmpError) as e:
        scene.arm_clearance_batch(2, torch.zeros((1, 7), dtype=torch.float64).cuda())
    assert e.value.code == -1
    with pytest.raises(CcmpError) as e:
        scene.arm_clearance_batch(0, torch.zeros((1, 7), dtype=torch.float64).cuda(), margin=float("nan"))
    assert e.value.code == -1
    # a NULL scene (the mirror would take the plain call): the C entry points, outputs prefilled — nothing may have been written
    L = _lib.lib()
    q = torch.full((1, 14), 7.0, dtype=torch.float64).cuda()
    ok = torch.full((1,), 9, dtype=torch.uint8).cuda()
    which = torch.full((1,), 9, dtype=torch.int32).cuda()
    clr = torch.full((1,), 7.0, dtype=torch.float64).cuda()
    h, P = c.ctx.handle, C.byref(c.problem)
    assert L.ccmp_pose_ik_vetted_batch(h, P, None, tpd.data_ptr(), sdd.data_ptr(), 1, 1, 0, 0, None, 0.0, q.data_ptr(), ok.data_ptr(), which.data_ptr(), None,
                                       None, None, None, clr.data_ptr(), None) == -1
    assert L.ccmp_pose_ik_vetted_batch(h, P, None, tpd.data_ptr(), sdd.data_ptr(), 1, 1, 0, 0, scene._h, float("nan"), q.data_ptr(), ok.data_ptr(),
                                       which.data_ptr(), None, None, None, None, clr.data_ptr(), None) == -1
    assert L.ccmp_pose_ik_vetted_batch(h, P, None, tpd.data_ptr(), sdd.data_ptr(), 1, 17, 0, 0, scene._h, 0.0, q.data_ptr(), ok.data_ptr(), which.data_ptr(),
                                       None, None, None, None, clr.data_ptr(), None) == -1
    assert L.ccmp_arm_clearance_batch(h, P, None, 0, q.data_ptr(), 1, 0.0, clr.data_ptr(), None, None) == -1
    assert L.ccmp_arm_clearance_batch(h, P, scene._h, 0, None, 1, 0.0, clr.data_ptr(), None, None) == -1
    assert L.ccmp_arm_clearance_batch(h, P, scene._h, 0, None, 0, 0.0, None, None, None) == 0  # B = 0 touches nothing
    torch.cuda.synchronize()
    assert (q == 7.0).all() and ok.item() == 9 and which.item() == 9 and clr.item() == 7.0


def test_capture_into_a_graph(gpu_ctx):
    """after one eager call at that size the call is capturable: the workspaces have their size, nothing allocates or synchronises"""
    import torch

    c = _constraint(gpu_ctx, False)
    tp, sd = _inputs(70, 5)
    tpd, sdd = torch.from_numpy(tp).cuda(), torch.from_numpy(sd).cuda()
    scene = _scene(c, default_scene_host(c.problem))
    kw = dict(rng_seed=RNG_SEED, first_index=4, want_candidates=True, scene=scene, margin=V.DEFAULT_MARGIN)
    eager = c.pose_ik_batch(tpd, sdd, **kw)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the eager call on the capture's side, outside the capture
        c.pose_ik_batch(tpd, sdd, **kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = c.pose_ik_batch(tpd, sdd, **kw)
    for t in cap.values():
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    _same(cap, eager)
    assert int(eager["ok"].sum()) > 0
