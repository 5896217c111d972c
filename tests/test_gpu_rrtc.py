"""RRT-Connect on the device (Roadmap.rrt_connect / ccmp_rrtc_*, Roadmap.nearest_in_tree) on Wine_Bottle: lists of 16 states, the
fixture scene, the far goal of tests/plan_cases.py (a goal one motion does not reach) and the shipped goal (one motion away).

1. Nearest-in-tree equals its _ref form bit for bit on stores of 1 .. 1025 rows with pose-only (NaN) and duplicated rows, for 1 .. 65
   queries and the trees "every vertex", "none", one of two components, eight of nine; with every vertex in the tree it equals
   `Roadmap.nearest_k` (joint metric, k = 1).  The sizes reach both launch shapes (one partition; partitions and the merge).
2. The pick kernel equals ccmp_rrtc_pick_ref on real traversals (both Jacobian modes, with and without the scene, lists of 2 and 16).
3. `RRTConnect` equals the loop written by hand (tests/rrtc_cases.py: HandRRTConnect) after every one of six cycles — state, store rows,
   edges and labels bit for bit — and `run(2)` three times equals `run(6)` once; then the invariants of the store it grew.
4. What occurred, from the hand loop, on the union of the runs: see test_the_runs_cover_the_outcomes.
5. A solved run on the shipped goal: the path and its dense form.  FULL at the stated size, a run after SOLVED, the argument checks.
6. The solution test's kernel, which Plan shares, at open on lists of 1 x 1, 1 x 8, 8 x 1, 8 x 8 and 3 x 5 vertices: no pair, the last
   pair alone, two pairs whose start-major and goal-major orders differ."""
import numpy as np
import pytest

import plan_cases as P
import rrtc_cases as R
from arm_model_cases import default_scene_host
from conftest import config_path
from object_cases import box_mesh, workspace

pytestmark = pytest.mark.gpu
MS, SEED, MARGIN = 16, 0x77C, -0.03
MESH = (0.04, 0.04, 0.1)
NS, QS = (1, 2, 63, 64, 65, 257, 1025), (1, 3, 64, 65)


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


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _store_bits(rm):
    j, p = rm.read(host=True)
    uv, w = rm.edges(host=True)
    return j.tobytes(), p.tobytes(), uv.tobytes(), w.tobytes(), rm.labels(host=True).tobytes()


def _same(a, b, what):
    for name, x, y in zip(("joints", "poses", "uv", "w", "labels"), a, b):
        assert x == y, (what, name)


# ---- 1. nearest vertex of a tree ---------------------------------------------------------------------------------------------------------
def test_the_sizes_reach_both_launch_shapes(gpu_ctx):
    from closed_chain_motion_planner_amd import rrtc_nearest_shape

    parts = {(N, Q): rrtc_nearest_shape(gpu_ctx.handle, Q, N)[1] for N in NS for Q in QS}
    print(parts)
    assert any(p == 1 for p in parts.values()) and any(p > 1 for p in parts.values())


def test_nearest_in_tree_merge_across_wavefronts(gpu_ctx):
    """The policy takes no option (its shape is a function of Q, N and the CU count), so the shapes are reached by sizes: the sizes above
    cut a store into at most five partitions, whose merge stays inside one wavefront.  One store large enough that a single query is cut
    into more than 64 partitions: the merge kernel's fold across its four wavefronts sees real bests."""
    from closed_chain_motion_planner_amd import KinematicChainConstraint, Roadmap, nearest_in_tree_ref, rrtc_nearest_shape

    N = 256 * 130 + 1
    c = KinematicChainConstraint.from_yaml(config_path("Wine_Bottle"), ctx=gpu_ctx)
    joints = R.tree_store(N)
    rm = Roadmap(c)
    rm.append(joints=_dev(joints), poses=_dev(np.zeros((N, 8))))
    rm.add_edges(np.array([(i % 2, i) for i in range(2, N)], dtype=np.int32))  # two stars: the even and the odd vertices
    labels = rm.labels(host=True)
    assert labels.tolist() == [i % 2 for i in range(N)]
    for Q in (1, 3):
        assert rrtc_nearest_shape(gpu_ctx.handle, Q, N)[1] > 64
        q = R.tree_queries(joints, Q)
        q[-1] = joints[N - 2]  # an answer in the last, one-row partition or next to it
        for roots in ([0], [1], [0, 1]):
            idx, dist = [x.cpu().numpy() for x in rm.nearest_in_tree(roots, _dev(q))]
            want_i, want_d = nearest_in_tree_ref(joints, labels, roots, q)
            assert idx.tolist() == want_i.tolist() and dist.tobytes() == want_d.tobytes(), (Q, roots)
    rm.close()


@pytest.mark.parametrize("N", NS)
def test_nearest_in_tree_equals_ref(gpu_ctx, N):
    from closed_chain_motion_planner_amd import KinematicChainConstraint, Roadmap, nearest_in_tree_ref
    from closed_chain_motion_planner_amd.roadmap import METRIC_JOINT

    c = KinematicChainConstraint.from_yaml(config_path("Wine_Bottle"), ctx=gpu_ctx)
    joints = R.tree_store(N)
    for stride, roots in ((1, [0]), (2, [0]), (9, [r for r in range(8) if r < N])):
        rm = Roadmap(c)
        rm.append(joints=_dev(joints), poses=_dev(np.zeros((N, 8))))
        uv = R.tree_edges(N, stride)
        if len(uv):
            rm.add_edges(uv)
        labels = rm.labels(host=True)
        for Q in QS:
            q = R.tree_queries(joints, Q)
            for rt in ([], roots):
                idx, dist = [x.cpu().numpy() for x in rm.nearest_in_tree(rt, _dev(q))]
                want_i, want_d = nearest_in_tree_ref(joints, labels, rt, q)
                assert idx.tolist() == want_i.tolist(), (N, stride, Q, rt)
                assert dist.tobytes() == want_d.tobytes(), (N, stride, Q, rt)
            if stride == 1:  # every vertex is in the tree: the joint-metric k-NN with k = 1 (idx, dist: the answer for `roots`)
                ki, kd = [x.cpu().numpy() for x in rm.nearest_k(_dev(q), 1, metric=METRIC_JOINT)]
                assert ki[:, 0].tolist() == idx.tolist() and kd[:, 0].tobytes() == dist.tobytes(), (N, Q)
        hi, hd = rm.nearest_in_tree(roots, R.tree_queries(joints, 3))  # the host form
        wi, wd = nearest_in_tree_ref(joints, labels, roots, R.tree_queries(joints, 3))
        assert hi.tolist() == wi.tolist() and hd.tobytes() == wd.tobytes()
        rm.close()


def test_nearest_in_tree_device_roots_and_bad_roots(gpu_ctx):
    from closed_chain_motion_planner_amd import CcmpError, KinematicChainConstraint, Roadmap

    c = KinematicChainConstraint.from_yaml(config_path("Wine_Bottle"), ctx=gpu_ctx)
    joints = R.tree_store(65)
    rm = Roadmap(c)
    rm.append(joints=_dev(joints), poses=_dev(np.zeros((65, 8))))
    rm.add_edges(R.tree_edges(65, 2))
    q = _dev(R.tree_queries(joints, 5))
    a = rm.nearest_in_tree([1], q)
    b = rm.nearest_in_tree(_dev(np.array([1], dtype=np.int32)), q)
    assert a[0].tolist() == b[0].tolist() and all(i % 2 == 1 for i in a[0].tolist())
    far = rm.nearest_in_tree([1, 99, -4], q)  # the device form: a root outside the store contributes no label
    assert far[0].tolist() == a[0].tolist()
    with pytest.raises(CcmpError):
        rm.nearest_in_tree([99], q.cpu().numpy())  # the host form refuses it
    with pytest.raises(CcmpError):
        rm.nearest_in_tree(list(range(9)), q)
    rm.close()


# ---- 2. the pick kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ms", [2, 16])
@pytest.mark.parametrize("scene", [False, True], ids=["plain", "scene"])
@pytest.mark.parametrize("mode", [0, 1], ids=["fd", "analytic"])
def test_pick_kernel_equals_ref_on_real_traversals(gpu_ctx, mode, scene, ms):
    from closed_chain_motion_planner_amd import rrtc_pick, rrtc_pick_ref

    c, chk, sc = _world(gpu_ctx, mode=mode, scene=scene)
    q, ok = c.sample_project_batch(SEED, 0, 2048, want_iters=False)[:2]  # (about one draw in five is a valid state)
    good = q[ok.bool() & c.joint_valid_batch(q).bool()].contiguous()
    assert good.shape[0] >= 130  # a condition on the sample
    frm, to = good[:65].contiguous(), good[65:130].contiguous()
    to[:8] = frm[:8] + 0.01  # near targets, off the manifold: short lists
    if sc is not None:
        out = c.discrete_geodesic_scene_batch(frm, to, sc, MARGIN, max_states=ms, want_carry=True, round_budget=24)
    else:
        out = c.discrete_geodesic_batch(frm, to, max_states=ms, want_carry=True, round_budget=24)
    st, ns, oks = out[0], out[1], out[2]
    d = _dev(np.array([R.dist(a, b) for a, b in zip(frm.cpu().numpy(), to.cpu().numpy())]))
    use = _dev(np.array([(i * 5 + 1) % 7 != 0 and 1 or (i % 2) * 2 for i in range(65)], dtype=np.uint8))
    seen = set()
    for E in (1, 5, 64, 65):
        for pick_mode, rng, u in ((0, 0.1, None), (0, 0.5, use), (0, 4.0, None), (1, 0.1, use), (1, 0.1, None)):
            args = (st[:E].contiguous(), ns[:E].contiguous(), oks[:E].contiguous(), to[:E].contiguous())
            kw = dict(d=d[:E].contiguous() if pick_mode == 0 else None, use=None if u is None else u[:E].contiguous(), range=rng, mode=pick_mode)
            got = {k: v.cpu().numpy() for k, v in rrtc_pick(gpu_ctx, *args, **kw).items()}
            want = rrtc_pick_ref(*[a.cpu().numpy() for a in args], d=None if kw["d"] is None else kw["d"].cpu().numpy(),
                                 use=None if kw["use"] is None else kw["use"].cpu().numpy(), range=rng, mode=pick_mode)
            for name in ("outcome", "row_index"):
                assert got[name].tolist() == want[name].tolist(), (E, pick_mode, rng, name)
            assert got["row"].tobytes() == want["row"].tobytes() and got["gap"].tobytes() == want["gap"].tobytes(), (E, pick_mode, rng)
            seen |= {(pick_mode, int(o)) for o in want["outcome"]}
    print("mode %d scene %s ms %d: outcomes %s, n_states %s" % (mode, scene, ms, sorted(seen), np.bincount(ns.cpu().numpy().clip(0, ms + 1)).tolist()))
    for h in (chk,) + ((sc,) if sc is not None else ()):
        h.close()


# ---- 3. the planner against the loop by hand -----------------------------------------------------------------------------------------------
def _far(gpu_ctx, mode, scene):
    c, chk, sc = _world(gpu_ctx, mode=mode, scene=scene)
    goal = P.far_goal_state(c, chk, MS)
    start = np.array(c.problem.start_joint[:])
    return c, chk, sc, start, goal


def _first_index(c):
    """a condition on the draws, not on the code under test: about one draw in five is a valid state, so a width-1 run of six cycles
    starts at the first draw index from which three of six draws are valid states"""
    q, ok = c.sample_project_batch(SEED, 0, 512, want_iters=False)[:2]
    flags = (ok.bool() & c.joint_valid_batch(q).bool()).cpu().numpy()
    return next(i for i in range(506) if flags[i:i + 6].sum() >= 3)


def _open(c, sc, start, goal, **kw):
    from closed_chain_motion_planner_amd import Roadmap

    rm = Roadmap(c)
    first = rm.append(joints=_dev(np.stack([start, goal])))
    assert first == 0
    return rm, rm.rrt_connect(c, starts=[0], goals=[1], scene=sc, margin=MARGIN, max_states=MS, rng_seed=SEED, **kw)


def _invariants(c, sc, rm, state, W, sizes, edge_counts, entry_labels, first_index=0):
    """the store after the cycles: sizes / edge_counts = the store's size / edge count at the entry of every cycle and at the end;
    entry_labels[k] = the labels at the entry of cycle k"""
    joints, _ = rm.read(host=True)
    uv, w = rm.edges(host=True)
    labels = rm.labels(host=True)
    cnt, cycles = state["counters"], state["cycle"]
    new = _dev(joints[2:])
    if len(joints) > 2:
        assert c.is_satisfied_batch(new).cpu().numpy().all() and c.joint_valid_batch(new).cpu().numpy().all()
        if sc is not None:
            assert (sc.clearance_batch(new, MARGIN, want_pair=False)[0].cpu().numpy() > MARGIN).all()
    for k in range(cycles):  # every edge of cycle k joins a vertex of the store at cycle entry to a new one
        e = uv[edge_counts[k]:edge_counts[k + 1]]
        assert ((e[:, 0] >= 0) & (e[:, 0] < sizes[k]) & (e[:, 1] >= sizes[k]) & (e[:, 1] < sizes[k + 1])).all(), (k, e, sizes)
        lab = entry_labels[k]  # ... and that vertex was in a tree then: its label was the label of the start root or of the goal root
        assert all(int(lab[u]) in (int(lab[0]), int(lab[1])) for u in e[:, 0]), (k, e, lab)
    roots = {int(labels[0]), int(labels[1])}
    assert all(int(l) in roots or int(l) == v for v, l in enumerate(labels))
    assert cnt["vertices"] == len(joints) - 2 and cnt["edges"] == len(uv) and cnt["samples"] == W * cycles and state["next_index"] == first_index + W * cycles
    assert cnt["projected"] == cnt["trapped"] + cnt["advanced"] + cnt["reached"] + cnt["unsettled"] <= cnt["samples"]
    assert cnt["connect_reached"] + cnt["connect_added"] + cnt["connect_nothing"] == cnt["advanced"] + cnt["reached"]
    assert cnt["vertices"] == cnt["advanced"] + cnt["reached"] + cnt["connect_added"] and cnt["edges"] == cnt["vertices"] + cnt["connect_reached"]
    assert np.array_equal(w, np.array([R.dist(joints[a], joints[b]) for a, b in uv]))


CASES = [(1, 1, False, 0.1), (5, 1, False, 0.1), (64, 1, False, 0.1), (5, 0, False, 0.1), (5, 1, True, 0.1), (5, 1, True, 3.0)]


@pytest.mark.parametrize("width,mode,scene,rng", CASES, ids=["w1", "w5", "w64", "w5-fd", "w5-scene", "w5-scene-range3"])
def test_rrt_connect_equals_the_hand_loop(gpu_ctx, width, mode, scene, rng):
    c, chk, sc, start, goal = _far(gpu_ctx, mode, scene)
    first = _first_index(c)
    kw = dict(width=width, range=rng, first_index=first)
    rm_a, pa = _open(c, sc, start, goal, **kw)
    rm_b, pb = _open(c, sc, start, goal, **kw)
    rm_c, pc = _open(c, sc, start, goal, **kw)
    from closed_chain_motion_planner_amd import Roadmap

    rm_h = Roadmap(c)
    rm_h.append(joints=_dev(np.stack([start, goal])))
    hp = R.HandRRTConnect(rm_h, c, [0], [1], scene=sc, margin=MARGIN, width=width, range=rng, rng_seed=SEED, max_states=MS, first_index=first)
    assert R.state_bits(pa.state()) == R.state_bits(hp.state), (pa.state(), hp.state)
    assert hp.state["status"] == R.OPEN  # the far goal is not connected at open
    sizes, edge_counts, entry_labels, ran = [len(rm_h)], [rm_h.num_edges], [], 0
    for cyc in range(6):
        if hp.state["status"] == R.SOLVED:
            break
        entry_labels.append(rm_a.labels(host=True))
        ra = pa.run(1)
        hp.run(1)
        sa = pa.state()
        assert R.state_bits(sa) == R.state_bits(hp.state), (cyc, sa, hp.state)
        _same(_store_bits(rm_a), _store_bits(rm_h), "cycle %d" % cyc)
        sizes.append(len(rm_h))
        edge_counts.append(rm_h.num_edges)
        ran += ra["cycles_run"]
    for _ in range(3):
        rb = pb.run(2)
    rc = pc.run(6)
    print("width %d mode %d scene %s range %g: %s seen %s" % (width, mode, scene, rng, rc, sorted(hp.seen)))
    assert rc["cycles_total"] == ran == rb["cycles_total"] and rc["status"] == rb["status"] == hp.state["status"]
    assert R.state_bits(pb.state()) == R.state_bits(pc.state()) == R.state_bits(pa.state())
    _same(_store_bits(rm_a), _store_bits(rm_b), "run(2) x 3")
    _same(_store_bits(rm_a), _store_bits(rm_c), "run(6)")
    assert rc["size"] == len(rm_c) and rc["edges"] == rm_c.num_edges and rc["counters"]["projected"] >= 1
    _invariants(c, sc, rm_c, pc.state(), width, sizes, edge_counts, entry_labels, first_index=first)
    for h in (pa, pb, pc, rm_a, rm_b, rm_c, rm_h, chk) + ((sc,) if sc is not None else ()):
        h.close()


def test_the_runs_cover_the_outcomes(gpu_ctx):
    """From the hand loop, never from the code under test: the union over widths 1, 5 and 64 at range 0.1 and width 5 at range 3 (six
    cycles each, analytic mode, lists of 16) of the (step, outcome) pairs that occurred.  What the far goal's six cycles do NOT reach, at
    any of these widths: REACHED — on this config two valid states are 6.8 apart in the median and never closer than 2.7 in 1 024 pairs
    (profiles/rrtc.md, the CPU oracle's pairs: `python tools/measure.py rrtc cpu`), so no sample lies within the range of a tree vertex —
    and JOINED, the trees being far apart by construction of the goal.  profiles/rrtc.md names both.  JOINED is asserted where it must occur, in the solved run below; REACHED on real traversals in the pick test above."""
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, _, start, goal = _far(gpu_ctx, 1, False)
    seen = set()
    for width, rng in ((1, 0.1), (5, 0.1), (64, 0.1), (5, 3.0)):
        rm = Roadmap(c)
        rm.append(joints=_dev(np.stack([start, goal])))
        hp = R.HandRRTConnect(rm, c, [0], [1], width=width, range=rng, rng_seed=SEED, max_states=MS, first_index=_first_index(c))
        hp.run(6)
        print(width, rng, hp.state, sorted(hp.seen))
        seen |= hp.seen
        rm.close()
    chk.close()
    want = {("extend", R.NONE), ("extend", R.TRAPPED), ("extend", R.ADVANCED), ("extend", R.UNSETTLED), ("connect", R.C_NOTHING), ("connect", R.C_ADDED)}
    assert want <= seen, sorted(seen)


# ---- 5. a solved run, limits ---------------------------------------------------------------------------------------------------------------
def test_a_solved_run_on_the_shipped_goal(gpu_ctx):
    """the shipped goal is one motion from the start: the trees join early.  The condition of the test is that the hand loop solves
    within 8 cycles at width 32; then RRTConnect does so in the same cycle and its solution is a path from the start to the goal.  The
    dense form's seg_ok is printed, not asserted: an edge was validated as a prefix of a traversal towards something else."""
    from closed_chain_motion_planner_amd import Roadmap

    c, chk, _ = _world(gpu_ctx, mode=1)
    start = np.array(c.problem.start_joint[:])
    _, goal_pose = P.problem_poses(c.problem)
    ik = c.pose_ik_batch(_dev(goal_pose.reshape(1, 8)), _dev(start.reshape(1, 1, 14)), rng_seed=SEED)
    assert int(ik["ok"][0]) == 1  # a condition on the shipped problem
    goal = ik["q"][0].cpu().numpy()
    rm_h = Roadmap(c)
    rm_h.append(joints=_dev(np.stack([start, goal])))
    hp = R.HandRRTConnect(rm_h, c, [0], [1], width=32, rng_seed=SEED, max_states=64)
    hp.run(8)
    assert hp.state["status"] == R.SOLVED, hp.state  # the test's condition
    assert ("connect", R.C_JOINED) in hp.seen and hp.state["counters"]["connect_reached"] >= 1  # a joined pair, from the hand loop
    rm = Roadmap(c)
    pl = rm.rrt_connect(c, start_joints=start, goal_joints=goal, width=32, rng_seed=SEED, max_cycles=8)
    r = pl.report
    assert r["status"] == R.SOLVED and r["solved"] == (0, 1) and r["cycles_total"] == hp.state["cycle"]
    assert R.state_bits(pl.state()) == R.state_bits(hp.state)
    sol = pl.solution(host=True)
    n = int(sol["path_len"][0])
    assert np.isfinite(sol["cost"][0]) and n >= 2
    assert sol["joints"][0, 0].tobytes() == start.tobytes() and sol["joints"][0, n - 1].tobytes() == goal.tobytes()
    dense = rm.dense_solution(c, [0], [1])
    assert dense is not None and np.isfinite(dense[0])
    print("solved in cycle %d, path of %d vertices, cost %g, seg_ok %s" % (r["cycles_total"], n, dense[0], dense[2]["seg_ok"].cpu().numpy().tolist()))
    again = pl.run(5)  # a run after SOLVED returns at once with the same report
    assert again == dict(r, cycles_run=0) and len(rm) == r["size"]
    for h in (pl, rm, rm_h, chk):
        h.close()


# ---- 6. the solution test's kernel (one text for Plan and RRTConnect) at the list shapes where its lane arithmetic can go wrong --------------
def _pair_lists(S, G, case):
    """starts [S], goals [G] on a store of 12 vertices in four components (vertex v in component v % 4; a list may repeat a vertex):
    "none": no pair is connected; "last": only pair (S - 1, G - 1), at 8 x 8 lane 63; "two": pairs (lo, G - 1) and (hi, 0) with lo < hi —
    start-major order takes the first, goal-major order would take the second wherever S >= 2 and G >= 2"""
    comp = lambda c, n: [c + 4 * (i % 3) for i in range(n)]
    if case == "none":
        return comp(0, S), comp(2, G)
    if case == "last":
        return comp(0, S - 1) + [1], comp(2, G - 1) + [5]
    starts, goals = comp(2, S), comp(3, G)
    hi = min(2, S - 1)
    lo = max(hi - 1, 0)
    if S == 1 or G == 1:  # one list has a single entry: both pairs share it, all four ends in component 0
        starts[hi], starts[lo], goals[0], goals[G - 1] = 4, 0, 8, 8
    else:
        starts[lo], goals[G - 1], starts[hi], goals[0] = 0, 4, 1, 5
    return starts, goals


@pytest.mark.parametrize("S,G", [(1, 1), (1, 8), (8, 1), (8, 8), (3, 5)])
def test_the_solution_test_at_every_list_shape(gpu_ctx, S, G):
    """open runs the solution test once (max_cycles = 0).  The expected state is the restatement's (rrtc_cases.new_state + connected) on
    the labels of graph_labels_ref over the same edges — never the library's _ref form of the test itself."""
    from closed_chain_motion_planner_amd import KinematicChainConstraint, Roadmap, graph_labels_ref

    c = KinematicChainConstraint.from_yaml(config_path("Wine_Bottle"), ctx=gpu_ctx)
    rm = Roadmap(c)
    rm.append(joints=np.random.default_rng(12).uniform(-2.0, 2.0, size=(12, 14)))  # the host forms, both: synchronous on one stream
    uv = R.tree_edges(12, 4)
    rm.add_edges(uv)
    labels = graph_labels_ref(uv, 12)
    assert labels.tolist() == [v % 4 for v in range(12)]
    for case in ("none", "last", "two"):
        starts, goals = _pair_lists(S, G, case)
        want = R.connected(labels, R.new_state(starts, goals))
        if case == "none":
            assert want["status"] == R.OPEN
        elif case == "last":
            assert (want["solved_start"], want["solved_goal"]) == (1, 5)
            assert [(s, g) for s in range(S) for g in range(G) if labels[starts[s]] == labels[goals[g]]] == [(S - 1, G - 1)]
        elif S >= 2 and G >= 2:  # the orders differ: goal-major would take (starts[hi], goals[0]) = (1, 5)
            assert (want["solved_start"], want["solved_goal"]) == (0, 4)
        pl = rm.rrt_connect(c, starts=starts, goals=goals, max_cycles=0)
        got = pl.state()
        assert R.state_bits(got) == R.state_bits(want), (case, got, want)
        assert pl.report["cycles_total"] == 0
        assert pl.report["solved"] == ((want["solved_start"], want["solved_goal"]) if want["status"] == R.SOLVED else None), (case, pl.report)
        pl.close()
    rm.close()


def test_full_at_the_stated_size_and_the_argument_checks(gpu_ctx):
    from closed_chain_motion_planner_amd import CcmpError

    c, chk, _, start, goal = _far(gpu_ctx, 1, False)
    W = 5
    rm, pl = _open(c, None, start, goal, width=W, max_vertices=2 + 2 * W - 1)
    before = _store_bits(rm)
    r = pl.run(3)
    assert r["status"] == R.FULL and r["cycles_run"] == 0 and r["cycles_total"] == 0 and r["counters"]["samples"] == 0
    _same(before, _store_bits(rm), "the refused cycle")
    pl.close()
    rm2, p2 = _open(c, None, start, goal, width=W, max_vertices=2 + 2 * W)  # exactly the worst case fits: one cycle runs
    assert p2.run(1)["cycles_run"] == 1
    p2.close()
    nan = float("nan")
    for bad in (dict(starts=[len(rm2)]), dict(goals=[-1]), dict(starts=[]), dict(goals=[0] * 9), dict(width=0), dict(width=257), dict(range=0.0), dict(range=nan),
                dict(range=float("inf")), dict(max_states=1), dict(round_budget=-1), dict(max_vertices=2**31)):
        kw = dict(starts=[0], goals=[1], width=W)
        kw.update(bad)
        with pytest.raises(CcmpError):
            rm2.rrt_connect(c, **kw)
    with pytest.raises(CcmpError):
        rm2.rrt_connect(c, starts=[0], goals=[1], margin=nan)
    with pytest.raises(ValueError):
        rm2.rrt_connect(c, starts=[0])
    for h in (rm, rm2, chk):
        h.close()
