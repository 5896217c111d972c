"""The planner's loop on the device (Roadmap.plan / ccmp_plan_*) on Wine_Bottle and the other shipped configs: a box mesh against the
fixture workspace, k = 5, lists of 16 states.

What the GPU showed first: on all three shipped configs checkMotion reaches the goal state from the start state, so open connects them
and no cycle ever runs (SOLVED, pair (0, 1), cycle 0).  Pre-filling the store cannot take that edge away, so the tests that need cycles
run Wine_Bottle towards another goal: tests/plan_cases.py: far_goal_state picks, from sampled states, the nearest one that one motion
does NOT reach, and makes its object pose the problem's goal pose.  On that problem six cycles give (every width, both modes, with and
without the scene alike): width 1 no check; width 5 two checks and a mid-stone; width 64 / 65 a check, a goal push, the whole ladder and
SOLVED after one cycle.  No single width reaches every branch within six cycles; test_the_runs_cover_every_branch asserts the union
from the reports of widths 5 and 64.

1. Plan equals its parts: `Plan.run(1)` six times, `Plan.run(6)` once and the by-hand driver of tests/plan_cases.py (the mirror's calls
   that exist without the unit, every decision on the host) leave the same bits — the store's joints and poses, the edge list and its
   weights, the labels and the state block — after every cycle.
2. Every check equals the mirror: on the store as the check saw it, `Roadmap.closest_from_goal` gives the state's nearest and
   prev_from_goal.
3. A goal one motion away is solved at open.
4. The shipped problems within a budget of 64 cycles at width 32: the invariants of the roadmap, never an error; SOLVED is not asserted.
5. Resume and caps: FULL one row short of a cycle's worst case, a run after SOLVED, two planners on two stores of one context."""
import numpy as np
import pytest

import plan_cases as P
from arm_model_cases import default_scene_host
from conftest import OBJECTS, config_path
from object_cases import box_mesh, workspace

pytestmark = pytest.mark.gpu
K, MS, SEED, MARGIN = 5, 16, 0x91A, -0.03
MESH = (0.04, 0.04, 0.1)


def _world(gpu_ctx, obj="Wine_Bottle", mode=0, scene=False):
    from closed_chain_motion_planner_amd import KinematicChainConstraint, ObjectChecker, ProxyScene

    c = KinematicChainConstraint.from_yaml(config_path(obj), ctx=gpu_ctx)
    c.setJacobianMode(mode)
    chk = ObjectChecker(c, box_mesh(*MESH), workspace())
    sc = None
    if scene:
        hs = default_scene_host(c.problem)
        sc = ProxyScene(c, hs.spheres, hs.boxes, hs.allowed)
    return c, chk, sc


def _store_bits(rm):
    j, p = rm.read(host=True)
    uv, w = rm.edges(host=True)
    return j.tobytes(), p.tobytes(), uv.tobytes(), w.tobytes(), rm.labels(host=True).tobytes()


def _same(a, b, what):
    for name, x, y in zip(("joints", "poses", "uv", "w", "labels"), a, b):
        assert x == y, (what, name)


@pytest.mark.parametrize("mode", [0, 1], ids=["fd", "analytic"])
@pytest.mark.parametrize("scene", [False, True], ids=["plain", "scene"])
@pytest.mark.parametrize("width", [1, 5, 64, 65])
def test_plan_equals_its_parts(gpu_ctx, width, scene, mode):
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, sc = _world(gpu_ctx, mode=mode, scene=scene)
    kw = dict(goal_joints=P.far_goal_state(c, chk, MS), scene=sc, margin=MARGIN, width=width, k=K, rng_seed=SEED, max_states=MS)
    rm_a, rm_b, rm_h = Roadmap(c), Roadmap(c), Roadmap(c)
    pa, pb = rm_a.plan(c, chk, **kw), rm_b.plan(c, chk, **kw)
    hp = P.HandPlan(rm_h, c, chk, **kw)
    assert P.state_bits(pa.state()) == P.state_bits(hp.state), (pa.state(), hp.state)
    _same(_store_bits(rm_a), _store_bits(rm_h), "open")
    ran = 0
    for cyc in range(6):
        ra = pa.run(1)
        hp.run(1)
        sa = pa.state()
        assert P.state_bits(sa) == P.state_bits(hp.state), (cyc, sa, hp.state)
        _same(_store_bits(rm_a), _store_bits(rm_h), "cycle %d" % cyc)
        ran += ra["cycles_run"]
    rb = pb.run(6)
    print("width %d scene %s mode %d: %s" % (width, scene, mode, rb))
    assert rb["cycles_run"] == ran == rb["cycles_total"]
    sb = pb.state()
    if rb["status"] == P.BUDGET:  # six single runs and one run of six end on the same verdict
        assert ra["status"] == P.BUDGET
    assert P.state_bits(sb) == P.state_bits(pa.state())
    _same(_store_bits(rm_a), _store_bits(rm_b), "run(6)")
    cnt = rb["counters"]
    assert cnt["proposals"] == width * ran and rb["size"] == len(rm_b) and rb["edges"] == rm_b.num_edges
    assert cnt["vertices_kept"] >= 1 and rb["size"] > 2  # the loop grew the store
    for h in (pa, pb, rm_a, rm_b, rm_h, chk) + ((sc,) if sc is not None else ()):
        h.close()


def test_the_runs_cover_every_branch(gpu_ctx):
    """from the reports: among the runs of test_plan_equals_its_parts (widths 5 and 64, six cycles) are a check, a goal push, a
    non-empty ladder prefix and a mid-stone"""
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, _ = _world(gpu_ctx)
    gj = P.far_goal_state(c, chk, MS)
    total = {}
    for width in (5, 64):
        rm = Roadmap(c)
        pl = rm.plan(c, chk, goal_joints=gj, width=width, k=K, rng_seed=SEED, max_states=MS, max_cycles=6)
        print(width, pl.report)
        for n, v in pl.report["counters"].items():
            total[n] = total.get(n, 0) + v
        pl.close()
        rm.close()
    # open pushes one start and one goal per run: a push made by a check is one more
    assert total["checks"] >= 1 and total["goal_pushes"] >= 2 + 1 and total["ladder_vertices"] >= 1 and total["mid_stones"] >= 1, total


def test_every_check_equals_the_mirror(gpu_ctx):
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, _ = _world(gpu_ctx)
    rm = Roadmap(c)
    pl = rm.plan(c, chk, goal_joints=P.far_goal_state(c, chk, MS), width=8, k=K, rng_seed=SEED, max_states=MS)
    checked = fired = 0
    for _ in range(8):
        before = pl.state()
        if before["status"] == P.SOLVED:
            break
        pl.run(1)
        s = pl.state()
        if s["counters"]["checks"] == before["counters"]["checks"]:
            assert (s["nearest"], s["prev_from_goal"]) == (before["nearest"], before["prev_from_goal"])
            continue
        # the store as the check saw it: the first size_at_check vertices and the edges among them
        n = s["size_at_check"]
        j, p = rm.read(host=True)
        uv, _ = rm.edges(host=True)
        old = Roadmap(c)
        old.append(joints=j[:n], poses=p[:n])
        keep = uv[(uv < n).all(axis=1)]
        if len(keep):
            old.add_edges(np.ascontiguousarray(keep))
        want_c, want_d = old.closest_from_goal(before["starts"], before["goals"][0])
        old.close()
        if want_d < before["prev_from_goal"] - 0.1:
            assert (s["nearest"], s["prev_from_goal"]) == (want_c, want_d), (s, want_c, want_d)
            fired += 1
        else:
            assert (s["nearest"], s["prev_from_goal"]) == (before["nearest"], before["prev_from_goal"])
        checked += 1
    assert checked >= 1 and fired >= 1, (checked, fired)
    pl.close()
    rm.close()


def _one_motion_world(gpu_ctx):
    """the first recorded edge that checkMotion passes in both directions, as (constraint with that start state, checker, u row, v row)"""
    import torch
    from dense_path_cases import recorded_roadmap

    c, chk, _ = _world(gpu_ctx)
    nodes, uv = recorded_roadmap()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    fwd = c.discrete_geodesic_batch(dev(nodes[uv[:, 0]]), dev(nodes[uv[:, 1]]), max_states=MS, check_target=True)[2].cpu().numpy()
    bwd = c.discrete_geodesic_batch(dev(nodes[uv[:, 1]]), dev(nodes[uv[:, 0]]), max_states=MS, check_target=True)[2].cpu().numpy()
    both = np.flatnonzero((fwd == 1) & (bwd == 1))
    assert len(both) >= 1  # a condition on the fixture, not on the code under test
    u, v = uv[both[0]]
    c.problem.start_joint[:] = nodes[u].tolist()
    return c, chk, nodes[u], nodes[v]


def test_a_goal_one_motion_away_is_solved_at_open(gpu_ctx):
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, qu, qv = _one_motion_world(gpu_ctx)
    rm = Roadmap(c)
    pl = rm.plan(c, chk, goal_joints=qv, width=5, k=K, rng_seed=SEED, max_states=MS)
    r = pl.report
    assert r["status"] == P.SOLVED and r["solved"] == (0, 1) and r["cycles_total"] == 0 and r["size"] == 2 and r["edges"] == 1
    out = rm.shortest_paths(np.array([0], dtype=np.int32), np.array([1], dtype=np.int32), host=True)
    assert int(out["path_len"][0]) == 2 and out["path"][0, :2].tolist() == [0, 1]
    assert out["joints"][0, 0].tobytes() == qu.tobytes() and out["joints"][0, 1].tobytes() == qv.tobytes()
    # a run after SOLVED returns at once with the same report
    again = pl.run(5)
    assert again == r and len(rm) == 2
    pl.close()
    rm.close()


@pytest.mark.parametrize("obj", OBJECTS)
def test_shipped_problems_within_a_budget(gpu_ctx, obj):
    import torch
    from closed_chain_motion_planner_amd import Roadmap, graph_labels_ref

    c, chk, _ = _world(gpu_ctx, obj)
    rm = Roadmap(c)
    pl = rm.plan(c, chk, width=32, k=K, rng_seed=SEED, max_states=MS)  # an error would raise here or in run
    prev = [pl.report["prev_from_goal"]]
    for _ in range(8):
        r = pl.run(8)
        prev.append(r["prev_from_goal"])
        if r["status"] != P.BUDGET:
            break
    print(obj, r)
    assert r["status"] in (P.SOLVED, P.BUDGET) and r["cycles_total"] <= 64
    assert all(b <= a for a, b in zip(prev, prev[1:])), prev  # prev_from_goal never rose
    j, p = rm.read(host=True)
    uv, w = rm.edges(host=True)
    assert np.array_equal(rm.labels(host=True), graph_labels_ref(uv, len(rm)))
    has = np.isfinite(j).all(axis=1)
    assert has.all() and c.is_satisfied_batch(torch.from_numpy(j[has]).cuda()).cpu().numpy().all()
    if r["status"] == P.SOLVED:
        s, g = r["solved"]
        out = rm.shortest_paths(np.array([s], dtype=np.int32), np.array([g], dtype=np.int32), host=True)
        n = int(out["path_len"][0])
        rows, _, goal = out["joints"][0, :n], *P.problem_poses(c.problem)
        assert n >= 2 and rows[0].tobytes() == np.array(c.problem.start_joint[:]).tobytes()
        assert out["poses"][0, n - 1, :7].tobytes() == goal[:7].tobytes()
        ok = c.discrete_geodesic_batch(torch.from_numpy(rows[:-1].copy()).cuda(), torch.from_numpy(rows[1:].copy()).cuda(), max_states=64, check_target=True)[2]
        print(obj, "path rows", n, "check_motion", ok.cpu().numpy().tolist())
        assert (ok.cpu().numpy() == 1).all()
    pl.close()
    rm.close()


def test_full_one_row_short_of_a_cycle(gpu_ctx):
    from closed_chain_motion_planner_amd import CcmpError, Roadmap

    c, chk, _ = _world(gpu_ctx)
    gj = P.far_goal_state(c, chk, MS)
    W = 5
    worst = W * (1 + K) + 9 + 2
    rm = Roadmap(c)
    pl = rm.plan(c, chk, goal_joints=gj, width=W, k=K, rng_seed=SEED, max_states=MS, max_vertices=2 + worst - 1)
    assert len(rm) == 2
    before = _store_bits(rm)
    r = pl.run(3)
    assert r["status"] == P.FULL and r["cycles_run"] == 0 and r["cycles_total"] == 0 and r["counters"]["proposals"] == 0
    _same(before, _store_bits(rm), "the refused cycle")
    pl.close()
    rm2 = Roadmap(c)
    p2 = rm2.plan(c, chk, goal_joints=gj, width=W, k=K, rng_seed=SEED, max_states=MS, max_vertices=2 + worst)  # exactly the worst case fits: one cycle runs
    assert p2.run(1)["cycles_run"] == 1
    p2.close()
    with pytest.raises(CcmpError):
        rm2.plan(c, chk, width=W, k=K, max_vertices=len(rm2) + 1)  # no room for the start and the goal vertex
    with pytest.raises(CcmpError):
        rm2.plan(c, chk, width=257, k=K)
    with pytest.raises(CcmpError):
        rm2.plan(c, chk, width=W, k=17)
    with pytest.raises(CcmpError):
        rm2.plan(c, chk, width=W, k=K, sigma=float("nan"))
    rm.close()
    rm2.close()


def test_two_planners_on_two_stores_do_not_disturb_each_other(gpu_ctx):
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, _ = _world(gpu_ctx)
    gj = P.far_goal_state(c, chk, MS)
    alone = Roadmap(c)
    pa = alone.plan(c, chk, goal_joints=gj, width=5, k=K, rng_seed=SEED, max_states=MS, max_cycles=3)
    want_state, want_store = P.state_bits(pa.state()), _store_bits(alone)
    r1, r2 = Roadmap(c), Roadmap(c)
    p1 = r1.plan(c, chk, goal_joints=gj, width=5, k=K, rng_seed=SEED, max_states=MS)
    p2 = r2.plan(c, chk, goal_joints=gj, width=8, k=K, rng_seed=SEED + 1, max_states=MS)
    for _ in range(3):
        p1.run(1)
        p2.run(1)
    assert P.state_bits(p1.state()) == want_state
    _same(_store_bits(r1), want_store, "interleaved")
    s2 = p2.state()
    assert s2["counters"]["proposals"] == 8 * s2["cycle"] and s2["cycle"] >= 1
    for h in (pa, p1, p2, alone, r1, r2):
        h.close()
