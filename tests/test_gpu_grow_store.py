"""Roadmap.grow (ccmp_roadmap_grow) on stores that hold pose-only vertices, -1 slots and non-finite joint rows, against the host
reference chain of tests/grow_store_cases.py, bit for bit: indices equal, float64 compared as bytes with every NaN canonical.

What the chain does not give — the traversal of an edge — is the existing entry point on the gathered pairs (discrete_geodesic_batch /
discrete_geodesic_scene_batch with the same max_states, check_target and round_budget), for the slots the masking rule keeps
(masked >= 0).  Every other slot must report n_states = ok = newton_iters = blocked = 0 and a zero carry, also where nbr_idx >= 0: the
caller's nbr_idx / nbr_dist stay the unmasked k-NN result.  This is the test of DESIGN.md §5.10's "no NaN reaches a traversal kernel":
ik_gather_seeds_kernel hands NaN rows to the solver, ik_grow_prepare_kernel's `finite` branch and its zero row in q_trav are taken, and
connect_gather_kernel / connect_fix_kernel run on the masked copy.  tests/test_grow_store_host.py shows that the inputs reach all of
that."""
import numpy as np
import pytest

from grow_store_cases import FIRST_INDEX, K, N_QUERIES, OBJ, RNG_SEED, bits, chain, leading_empty, mixed_store
from knn_reference import KNN_ALL, KNN_EARLIER, KNN_NOT_SELF
from test_gpu_parity import _constraint

pytestmark = pytest.mark.gpu
MS = 16
EDGE_NAMES = ("n_states", "ok", "newton_iters", "blocked", "carry")


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _store(c, parts):
    """a store filled in order from parts: ("j", joints (n,14)) or ("p", poses (n,8)) — the latter pose-only vertices"""
    from closed_chain_motion_planner_amd import Roadmap

    rm = Roadmap(c, capacity_hint=sum(len(a) for _, a in parts))
    for kind, a in parts:
        if len(a) and kind == "j":
            rm.append(joints=_dev(a))
        elif len(a):
            rm.append(None, _dev(a))
    return rm


def _arrays(rm):
    j, p = rm.read()
    return j.cpu().numpy(), p.cpu().numpy()


def _numpy(out):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}


def _same_outputs(a, b, ms=MS):
    """two results of grow: every array as bytes; the state lists up to what each edge stored (rows beyond n_states are not written)"""
    a, b = _numpy(a), _numpy(b)
    for name in a:
        if name == "states":
            for e, n in enumerate(a["n_states"]):
                m = min(int(n), ms)
                assert np.array_equal(bits(a[name][e, :m]), bits(b[name][e, :m])), (name, e)
        else:
            assert np.array_equal(bits(a[name]), bits(b[name])), name


def _check(c, rm, out, queries, k=K, mode=KNN_ALL, self_base=0, first_index=FIRST_INDEX, ms=MS, check_target=False, round_budget=0, scene=None,
           margin=None, rng_seed=RNG_SEED):
    """`out` = rm.grow(queries, ...) against the chain on the store's arrays as they stand; returns the chain's dict"""
    sj, sp = _arrays(rm)
    ref = chain(c.problem, sj, sp, queries, k, mode, self_base, rng_seed, first_index)
    got = _numpy(out)
    assert np.array_equal(got["nbr_idx"], ref["nbr_idx"]) and np.array_equal(bits(got["nbr_dist"]), bits(ref["nbr_dist"]))  # the unmasked k-NN
    assert np.array_equal(got["ik_ok"], ref["ik_ok"]) and np.array_equal(got["ik_which"], ref["ik_which"])
    assert np.array_equal(bits(got["q_new"]), bits(ref["q_new"]))
    masked = ref["masked"].reshape(-1)
    live = masked >= 0
    if live.any():
        frm = _dev(sj[masked[live]])
        to = _dev(np.repeat(ref["q_new"], k, axis=0)[live])
        assert bool(np.isfinite(sj[masked[live]]).all()) and bool(np.isfinite(np.repeat(ref["q_new"], k, axis=0)[live]).all())
        if scene is not None:
            w = [t.cpu().numpy() for t in c.discrete_geodesic_scene_batch(frm, to, scene, margin, ms, check_target=check_target, want_carry=True,
                                                                          round_budget=round_budget)]
            want = {"states": w[0], "n_states": w[1], "ok": w[2], "newton_iters": w[3], "blocked": w[4], "carry": w[5]}
        else:
            w = [t.cpu().numpy() for t in c.discrete_geodesic_batch(frm, to, ms, check_target=check_target, want_carry=True, round_budget=round_budget)]
            want = {"states": w[0], "n_states": w[1], "ok": w[2], "newton_iters": w[3], "blocked": np.zeros(len(w[1]), np.uint8), "carry": w[4]}
        for i, e in enumerate(np.flatnonzero(live)):
            for name in EDGE_NAMES:
                assert np.array_equal(bits(got[name][e]), bits(want[name][i])), (name, e)
            m = min(int(want["n_states"][i]), ms)
            assert m >= 1 and np.array_equal(bits(got["states"][e, :m]), bits(want["states"][i, :m])), ("states", e)
    for name in EDGE_NAMES:  # a masked slot never ran, whatever nbr_idx says
        assert not got[name][~live].any(), name
    return ref


@pytest.fixture(scope="module")
def world(gpu_ctx):
    c = _constraint(OBJ, gpu_ctx)
    joints, _, queries, extra, owner = mixed_store()
    return c, np.array(joints), np.array(queries), np.array(extra), owner


def _mixed(c, world):
    _, joints, _, extra, _ = world
    return _store(c, [("j", joints), ("p", extra)])


@pytest.mark.parametrize("form", ["device", "numpy"])
@pytest.mark.parametrize("Q", [N_QUERIES, 1])
def test_mixed_store(world, Q, form):
    """FD mode, no scene: 12 targets (0..5 leading pose-only slots each, two targets without a state), and target 3 alone (three
    pose-only slots ahead of the seed that solves it); the numpy form gives the device form's bytes"""
    c, joints, queries, extra, owner = world
    rm = _mixed(c, world)
    qs, first = (queries, FIRST_INDEX) if Q == N_QUERIES else (queries[3:4].copy(), FIRST_INDEX + 3)
    out = rm.grow(_dev(qs), K, rng_seed=RNG_SEED, first_index=first, max_states=MS)
    if form == "numpy":
        host = rm.grow(qs, K, rng_seed=RNG_SEED, first_index=first, max_states=MS)
        assert all(isinstance(v, np.ndarray) for v in host.values())
        _same_outputs(host, out)
        out = host
    ref = _check(c, rm, out, qs, first_index=first)
    lead = leading_empty(ref)
    assert np.array_equal(ref["ik_which"], np.where(lead < K, lead, -1))
    got = _numpy(out)
    pose_only = ref["nbr_idx"] >= len(joints)
    if Q == 1:
        assert lead[0] == 3 and list(pose_only[0]) == [True, True, True, False, False] and list(ref["masked"][0] >= 0) == [False, False, False, True, True]
    else:
        empty = (ref["masked"] < 0).sum(axis=1)
        assert (empty == K).any() and (empty == 0).any() and pose_only.any(axis=1).sum() >= 10
        assert np.isnan(got["q_new"][empty == K]).all()
        ran = got["n_states"].reshape(Q, K) > 0
        assert np.array_equal(ran, ref["masked"] >= 0)  # every kept slot stored at least its start; no other slot did
    rm.close()


@pytest.mark.parametrize("variant", ["analytic", "scene", "budget"])
def test_mixed_store_variants(world, gpu_ctx, variant):
    """once each on the 12 targets: the analytic Jacobian, a proxy scene (blocked is an output), a round budget with carries"""
    from closed_chain_motion_planner_amd.scene import ProxyScene, default_allowed, skeleton_spheres

    c = _constraint(OBJ, gpu_ctx, mode=1) if variant == "analytic" else world[0]
    queries = world[2]
    rm = _mixed(c, world)
    kw = {}
    if variant == "scene":
        kw = dict(scene=ProxyScene(c, skeleton_spheres(c.problem), (), default_allowed()), margin=0.02)
    elif variant == "budget":
        kw = dict(round_budget=32)
    out = rm.grow(_dev(queries), K, rng_seed=RNG_SEED, first_index=FIRST_INDEX, max_states=MS, **kw)
    ref = _check(c, rm, out, queries, **kw)
    got = _numpy(out)
    ran = ref["masked"].reshape(-1) >= 0
    print("%s: %d of %d slots ran, ok %s, blocked %d" % (variant, int(ran.sum()), ran.size, np.bincount(got["ok"][ran], minlength=3), int(got["blocked"].sum())))
    # the variant is exercised: edges the scene stopped; edges the budget suspended (ok = 2, to be continued from their carry)
    assert variant != "scene" or got["blocked"][ran].any()
    assert variant != "budget" or (got["ok"][ran] == 2).any()
    rm.close()


def test_short_store_and_earlier(world):
    """fewer vertices than k (a -1 slot on every target), and KNN_EARLIER from self_base = 1 (target q sees vertices 0 .. q): -1 slots
    next to pose-only ones, the pose-only vertex of targets 2 and 3 in their first slot"""
    c, joints, queries, _, _ = world
    rm = _store(c, [("j", joints[:1]), ("p", queries[2:3]), ("j", joints[1:2]), ("p", queries[3:4])])
    assert len(rm) == 4 < K
    for mode, base in ((KNN_ALL, 0), (KNN_EARLIER, 1)):
        out = rm.grow(_dev(queries[:4]), K, mode, base, rng_seed=RNG_SEED, first_index=FIRST_INDEX, max_states=MS)
        ref = _check(c, rm, out, queries[:4], mode=mode, self_base=base)
        idx = ref["nbr_idx"]
        if mode == KNN_ALL:
            assert ((idx >= 0).sum(axis=1) == 4).all() and idx[2, 0] == 1 and idx[3, 0] == 3
        else:
            assert list((idx >= 0).sum(axis=1)) == [1, 2, 3, 4] and idx[2, 0] == 1 and idx[3, 0] == 3
        assert (ref["masked"][np.isin(idx, (1, 3))] == -1).all() and (ref["masked"] >= 0).any()
    rm.close()


def test_set_joints_and_a_non_finite_row(world):
    """a pose-only vertex given joints by set_joints is an ordinary neighbour again (its slot runs); a joint row with one +inf is
    masked exactly like a NaN row"""
    from pose_ik_cases import sampled_case

    c, joints, queries, extra, owner = world
    rm = _mixed(c, world)
    n_joint = len(joints)
    v = n_joint + int(np.flatnonzero(owner == 1)[0])  # target 1's only pose-only vertex, 1e-4 from it
    state = np.array(sampled_case(OBJ)[2][1])         # the valid state whose pose target 1 is
    rm.set_joints(v, _dev(state))
    out = rm.grow(_dev(queries), K, rng_seed=RNG_SEED, first_index=FIRST_INDEX, max_states=MS)
    ref = _check(c, rm, out, queries)
    assert ref["nbr_idx"][1, 0] == v and ref["masked"][1, 0] == v and ref["ik_which"][1] == 0
    assert _numpy(out)["n_states"][1 * K + 0] >= 1
    j = int(ref["nbr_idx"][0, 0])  # target 0 has no pose-only vertex: its nearest neighbour has joints and seeded its state
    assert j < n_joint and ref["ik_which"][0] == 0 and (ref["masked"] == j).any()
    row = joints[j].copy()
    row[9] = np.inf
    rm.set_joints(j, row)  # the host form
    out = rm.grow(_dev(queries), K, rng_seed=RNG_SEED, first_index=FIRST_INDEX, max_states=MS)
    ref2 = _check(c, rm, out, queries)
    assert np.array_equal(ref2["nbr_idx"], ref["nbr_idx"]) and not (ref2["masked"] == j).any() and ref2["ik_which"][0] != 0
    rm.close()


def test_append_first_equals_query_first(world):
    """INTEGRATION.md, "A planner that would rather append first": the targets appended as pose-only vertices t .. t + 11 and
    grow(KNN_NOT_SELF, self_base = t); for one target that is grow(KNN_ALL) on the store without the vertex"""
    c, joints, queries, extra, _ = world
    rm = _mixed(c, world)
    t = len(rm)
    assert rm.append(None, _dev(queries)) == t
    out = rm.grow(_dev(queries), K, KNN_NOT_SELF, t, rng_seed=RNG_SEED, first_index=FIRST_INDEX, max_states=MS)
    ref = _check(c, rm, out, queries, mode=KNN_NOT_SELF, self_base=t)
    assert not (ref["nbr_idx"] == (t + np.arange(N_QUERIES))[:, None]).any()
    for q in (0, 3, 5):
        rm.truncate(t)
        one = _dev(queries[q:q + 1].copy())
        before = rm.grow(one, K, KNN_ALL, 0, rng_seed=RNG_SEED, first_index=FIRST_INDEX + q, max_states=MS)
        assert rm.append(None, one) == t
        after = rm.grow(one, K, KNN_NOT_SELF, t, rng_seed=RNG_SEED, first_index=FIRST_INDEX + q, max_states=MS)
        _check(c, rm, after, queries[q:q + 1], mode=KNN_NOT_SELF, self_base=t, first_index=FIRST_INDEX + q)
        _same_outputs(after, before)
    rm.close()


def test_grow_toward_on_the_mixed_store(world):
    """Roadmap.grow_toward from the poses of joint and pose-only vertices alike: its rows are propose + grow by hand"""
    import torch
    from closed_chain_motion_planner_amd import ObjectChecker
    from object_cases import box_mesh, workspace

    c, joints, queries, extra, _ = world
    rm = _mixed(c, world)
    n_joint = len(joints)
    _, poses = rm.read()
    frm = torch.cat([poses[n_joint - 6: n_joint + 10], torch.full((1, 8), float("nan"), dtype=torch.float64, device=poses.device)]).contiguous()
    goal = poses[:1].contiguous()
    chk = ObjectChecker(c, box_mesh(0.01, 0.01, 0.01), workspace())
    kw = dict(t=0.3, sigma=0.2, lo=(0.1, -0.5, 1.25), hi=(1.2, 0.5, 1.8), attempts=2, rng_seed=0x6A0, first_index=40)
    out = rm.grow_toward(chk, frm, goal, 3, max_states=8, **kw)
    prop = chk.propose(frm, goal, **kw)
    which = prop["which"].cpu().numpy()
    assert np.array_equal(out["which"].cpu().numpy(), which) and which[-1] == -1 and (which >= 0).any()
    rows = np.flatnonzero(which >= 0)
    assert np.array_equal(out["rows"], rows)
    kept = prop["pose"][torch.from_numpy(rows).cuda()].contiguous()
    assert torch.equal(out["poses"], kept)
    by_hand = rm.grow(kept, 3, rng_seed=0x6A0, first_index=40, max_states=8)
    _same_outputs(by_hand, {k: out[k] for k in by_hand}, ms=8)
    _check(c, rm, by_hand, kept.cpu().numpy(), k=3, first_index=40, ms=8, rng_seed=0x6A0)
    print("grow_toward: %d poses kept, %d pose-only neighbours" % (len(rows), int((by_hand["nbr_idx"] >= n_joint).sum())))
    chk.close()
    rm.close()
