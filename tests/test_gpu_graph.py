"""The roadmap graph on the device (ccmp_roadmap_commit, _add_edges, _closest, the labels) against the host forms and the numpy
union-find, bit for bit: integers equal, float64 compared as bytes.  The kernels and the *_ref forms compile one text
(csrc/ccmp_graph.h); tests/test_graph_ref.py checks that text against restatements that share nothing with it."""
import numpy as np
import pytest

from graph_cases import (BATCH_SHAPES, MS, ROOTS, base_store, batch_case, bits, commit_args, initial_edges, make_case, same_commit, union_find_labels)
from test_gpu_parity import _constraint

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"


def _dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C", copy=True)).cuda()


@pytest.fixture(scope="module")
def c(gpu_ctx):
    return _constraint(OBJ, gpu_ctx)


def _pose_store(c, n, capacity_hint=None, seed=0):
    """n pose-only vertices (the labels and closest read no joints)"""
    from closed_chain_motion_planner_amd import Roadmap

    rng = np.random.default_rng(seed)
    poses = np.zeros((n, 8))
    poses[:, :3] = rng.uniform(-1, 1, (n, 3))
    q = rng.normal(size=(n, 4))
    poses[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    rm = Roadmap(c, capacity_hint=n if capacity_hint is None else capacity_hint)
    rm.append(None, _dev(poses))
    import torch

    torch.cuda.current_stream().synchronize()  # the append is asynchronous on this stream; the tests' host forms run on the context's own
    return rm, poses


def _edges_check(rm, uv_all, n):
    """the store's labels and edge list against the numpy union-find over every edge added so far"""
    assert rm.num_edges == len(uv_all)
    assert np.array_equal(rm.labels(host=True), union_find_labels(uv_all, n))
    uv, _ = rm.edges(host=True)
    assert np.array_equal(uv, uv_all)
    assert np.array_equal(rm.labels().cpu().numpy(), rm.labels(host=True))


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 65, 1025, 4099])
def test_a_whole_chain_in_one_call(c, N):
    """0-1-...-(N-1) reversed and shuffled: every hook of a round collides with its neighbours'"""
    chain = np.stack([np.arange(N - 1), np.arange(1, N)], axis=1).astype(np.int32)
    rng = np.random.default_rng(N)
    for order in (chain[::-1], rng.permutation(chain), chain[:, ::-1]):
        rm, _ = _pose_store(c, N)
        assert np.array_equal(rm.labels(host=True), np.arange(N))
        order = np.ascontiguousarray(order)
        assert rm.add_edges(_dev(order)) == 0
        _edges_check(rm, order, N)
        assert not rm.labels(host=True).any()
        rm.close()


@pytest.mark.parametrize("E", [1, 63, 64, 65, 4098])
def test_random_edges_stars_duplicates_and_three_calls_in_a_row(c, E):
    N = 1025
    rng = np.random.default_rng(E)
    rm, _ = _pose_store(c, N)
    star = np.stack([np.full(40, 700), rng.choice(700, 40, replace=False)], axis=1)
    # pairs of edges that hook ONE root (900 / 901) from two components in the same round, both ways round
    two = np.array([[900, 3], [900, 2], [5, 901], [901, 4], [900, 901]])
    rand = rng.integers(0, N, size=(E, 2))
    rand = rand[rand[:, 0] != rand[:, 1]]
    calls = [np.concatenate([rand, rand[: len(rand) // 2]]), np.concatenate([star, two, star[:7, ::-1]]), rng.integers(0, N // 2, size=(E, 2)) * 2 + np.array([0, 1])]
    done = np.zeros((0, 2), np.int32)
    for i, uv in enumerate(calls):
        uv = np.ascontiguousarray(uv.astype(np.int32))
        if len(uv) == 0:
            continue
        if i == 1:
            rm.add_edges(uv)  # the host form
        else:
            assert rm.add_edges(_dev(uv)) == 0
        done = np.concatenate([done, uv])
        _edges_check(rm, done, N)
    rm.close()


def test_the_device_form_skips_bad_edges_and_the_host_form_refuses_them(c):
    from closed_chain_motion_planner_amd import CcmpError

    rm, _ = _pose_store(c, 65)
    uv = np.array([[0, 1], [3, 3], [64, 2], [65, 2], [-1, 4], [7, 8], [2, 1 << 30]], dtype=np.int32)
    assert rm.add_edges(_dev(uv)) == 4
    _edges_check(rm, uv[[0, 2, 5]], 65)
    for bad in ([[3, 3]], [[0, 65]], [[-1, 0]]):
        with pytest.raises(CcmpError) as e:
            rm.add_edges(np.array(bad, dtype=np.int32))
        assert e.value.code == -1
    assert rm.num_edges == 3
    rm.close()


def test_edge_weights_are_the_joint_distance(c):
    from closed_chain_motion_planner_amd import Roadmap, joint_distance

    joints = np.array(base_store()[0])
    rm = Roadmap(c, capacity_hint=len(joints))
    rm.append(joints=_dev(joints))
    uv = initial_edges(len(joints))
    rm.add_edges(_dev(uv))
    _, w = rm.edges(host=True)
    want = np.array([joint_distance(joints[u], joints[v]) for u, v in uv])
    assert np.array_equal(bits(w), bits(want))
    assert np.array_equal(bits(rm.edges()[1]), bits(want))
    rm.close()


def test_growth_of_rows_and_edges_in_mid_sequence_and_truncate(c):
    """from capacity 4: the rows (with their labels) and the edge block move while the graph is live; truncate stops at the edge floor"""
    from closed_chain_motion_planner_amd import CcmpError, Roadmap

    joints = np.array(base_store()[0])
    rm = Roadmap(c, capacity_hint=4)
    done = np.zeros((0, 2), np.int32)
    n = 0
    rng = np.random.default_rng(4)
    for step, grow in enumerate((3, 2, 30, 100, 59)):
        rm.append(joints=_dev(joints[n:n + grow]))
        n += grow
        uv = rng.integers(0, n, size=(3 + 400 * step, 2)).astype(np.int32)  # 1 203 edges in the fourth call: beyond the first edge block
        uv = np.ascontiguousarray(uv[uv[:, 0] != uv[:, 1]])
        rm.add_edges(_dev(uv))
        done = np.concatenate([done, uv])
        _edges_check(rm, done, n)
    floor = int(done.max()) + 1
    rm.append(joints=_dev(joints[:5]))  # five vertices without an edge
    assert len(rm) == n + 5 and np.array_equal(rm.labels(n, 5, host=True), np.arange(n, n + 5))
    rm.truncate(n + 2)
    if floor > 0:
        with pytest.raises(CcmpError) as e:
            rm.truncate(floor - 1)
        assert e.value.code == -1 and len(rm) == n + 2
    rm.truncate(floor)
    assert len(rm) == floor
    _edges_check(rm, done, floor)
    rm.close()
    rm, _ = _pose_store(c, 10)  # a store without edges truncates as before
    rm.truncate(3)
    rm.truncate(0)
    assert len(rm) == 0
    rm.close()


# ---- commit ---------------------------------------------------------------------------------------------------------------------------
def _graph_store(c, g):
    """a store holding the Graph g: its vertices and its edges, in order"""
    from closed_chain_motion_planner_amd import Roadmap

    sj, sp = g.arrays()
    rm = Roadmap(c, capacity_hint=4)
    rm.append(_dev(sj), _dev(sp))
    if g.edges:
        rm.add_edges(_dev(np.array([(u, v) for u, v, _ in g.edges], dtype=np.int32)))
    return rm, sj, sp


def _commit_and_compare(c, rm, sj, sp, case, form):
    """Roadmap.commit against commit_ref on the store's arrays at entry; rows, edges and labels read back from the store"""
    from closed_chain_motion_planner_amd import commit_ref, graph_labels_ref

    n0, e0 = len(rm), rm.num_edges
    labels0 = rm.labels(host=True)
    uv0, _ = rm.edges(host=True)
    want = commit_ref(c.problem, sj, sp, labels0, **commit_args(case))
    kw = commit_args(case)
    if form == "device":
        for name in ("nbr_idx", "edge_ok", "n_states", "new_joints", "new_poses", "states", "vertex_ok"):
            kw[name] = None if kw[name] is None else _dev(kw[name])
    out = rm.commit(**kw)
    rows_j, rows_p = rm.read(n0, host=True)
    uv, w = rm.edges(e0, host=True)
    got = {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in out.items()}
    got.update(rows_joints=rows_j, rows_poses=rows_p, edges_uv=uv, edges_w=w)
    same_commit(got, want)
    assert got["vertices_added"] == len(want["rows_joints"]) and got["edges_added"] == len(want["edges_uv"])
    assert len(rm) == n0 + got["vertices_added"] and rm.num_edges == e0 + got["edges_added"]
    assert np.array_equal(rm.labels(host=True), graph_labels_ref(np.concatenate([uv0, uv]), len(rm)))
    assert np.array_equal(rm.labels(host=True), union_find_labels(np.concatenate([uv0, uv]), len(rm)))
    return got


@pytest.mark.parametrize("form", ["device", "numpy"])
@pytest.mark.parametrize("Q,k", BATCH_SHAPES)
def test_commit_batches(c, Q, k, form):
    g, case = batch_case(Q, k)
    rm, sj, sp = _graph_store(c, g)
    got = _commit_and_compare(c, rm, sj, sp, case, form)
    if Q * k >= 60:
        assert (got["mid_index"] >= 0).any()
    rm.close()


def test_forty_sequential_commits(c):
    """the planner's shape, Q = 1 and k = 5, on one growing store from capacity 4; every seventh keeps its isolated vertex"""
    from graph_cases import Graph

    joints, poses, fresh, fresh_poses, goal = base_store()
    rm, sj, sp = _graph_store(c, Graph(joints, poses, initial_edges(len(joints))))
    for step in range(40):
        case = make_case(sj, sp, 1, 5, 500 + step, goal, fresh[step:step + 1], fresh_poses[step:step + 1], flags=1 if step % 7 == 3 else 0)
        got = _commit_and_compare(c, rm, sj, sp, case, "device" if step % 2 else "numpy")
        sj, sp = np.concatenate([sj, got["rows_joints"]]), np.concatenate([sp, got["rows_poses"]])
    assert len(rm) > len(joints) + 20
    rm.close()


def test_commit_without_lists_goal_or_flags_and_the_empty_call(c):
    g, case = batch_case(12, 5)
    for drop in ("states", "goal_pose", "vertex_ok"):
        rm, sj, sp = _graph_store(c, g)
        less = dict(case)
        less[drop] = None
        got = _commit_and_compare(c, rm, sj, sp, less, "device")
        if drop != "vertex_ok":
            assert (got["mid_index"] < 0).all()
        rm.close()
    rm, sj, sp = _graph_store(c, g)
    empty = make_case(sj, sp, 0, 5, 1, case["goal_pose"], *base_store()[2:4])
    out = rm.commit(**commit_args(empty))
    assert out["vertices_added"] == 0 and out["edges_added"] == 0 and len(rm) == len(sj)
    rm.close()


def test_grow_then_commit_end_to_end(c):
    """Roadmap.grow on the mixed store of grow_store_cases, its outputs unchanged into commit, then commit_ref on the same arrays"""
    from grow_store_cases import FIRST_INDEX, K, RNG_SEED, mixed_store
    from closed_chain_motion_planner_amd import Roadmap

    joints, _, queries, extra, _ = mixed_store()
    rm = Roadmap(c, capacity_hint=len(joints) + len(extra))
    rm.append(joints=_dev(np.array(joints)))
    rm.append(None, _dev(np.array(extra)))
    rm.add_edges(_dev(initial_edges(len(joints))))
    out = rm.grow(_dev(np.array(queries)), K, rng_seed=RNG_SEED, first_index=FIRST_INDEX, max_states=16)
    sj, sp = (a.cpu().numpy() for a in rm.read())
    case = {"nbr_idx": out["nbr_idx"].cpu().numpy(), "edge_ok": out["ok"].cpu().numpy(), "n_states": out["n_states"].cpu().numpy(),
            "states": out["states"].cpu().numpy(), "max_states": 16, "new_joints": out["q_new"].cpu().numpy(), "new_poses": np.array(queries),
            "vertex_ok": out["ik_ok"].cpu().numpy(), "goal_pose": base_store()[4], "roots": ROOTS, "flags": 0}
    n0, e0 = len(rm), rm.num_edges
    labels0 = rm.labels(host=True)
    from closed_chain_motion_planner_amd import commit_ref

    want = commit_ref(c.problem, sj, sp, labels0, **commit_args(case))
    got = rm.commit(out["nbr_idx"], out["ok"], out["n_states"], out["q_new"], _dev(np.array(queries)), states=out["states"], vertex_ok=out["ik_ok"],
                    goal_pose=case["goal_pose"], roots=ROOTS)
    got = {name: (v.cpu().numpy() if hasattr(v, "cpu") else v) for name, v in got.items()}
    got["rows_joints"], got["rows_poses"] = rm.read(n0, host=True)
    got["edges_uv"], got["edges_w"] = rm.edges(e0, host=True)
    same_commit(got, want)
    assert got["edges_added"] > 0 and (got["new_index"] >= 0).any()
    rm.close()


# ---- closest --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 5, 64])
@pytest.mark.parametrize("N", [3, 1000, 4099, 65537])
def test_closest(c, N, F):
    """one and several partitions (2 048 vertices each); the planted best vertex in the last partition; ties across partitions: the pose
    of the planted vertex also sits at a lower index of another partition in half of the components"""
    from closed_chain_motion_planner_amd import closest_ref

    rng = np.random.default_rng(N + F)
    rm, poses = _pose_store(c, N, seed=N)
    uv = rng.integers(0, N, size=(N // 2 + 1, 2)).astype(np.int32)
    uv = np.ascontiguousarray(uv[uv[:, 0] != uv[:, 1]])
    target = np.array([0.1, -0.2, 0.3, 0.0, 0.0, 0.0, 1.0, 0.0])
    if N > 3:  # plant: the target's own pose at N - 1 (distance 0) and, again, at 1 and in the middle; a NaN pose; all in one component
        plant = np.array([[N - 1, 0], [1, N - 1], [N // 2, 1], [2, N - 1]], dtype=np.int32)
        uv = np.concatenate([uv, plant])
        fix = {N - 1: target, 1: target, N // 2: target, 2: np.full(8, np.nan)}
        for i, p in fix.items():
            poses[i] = p
        rm.close()
        from closed_chain_motion_planner_amd import Roadmap

        rm = Roadmap(c, capacity_hint=N)
        rm.append(None, _dev(poses))
    if len(uv):
        rm.add_edges(_dev(uv))
    labels = rm.labels(host=True)
    assert np.array_equal(labels, union_find_labels(uv, N))
    froms = rng.integers(0, N, size=F).astype(np.int32)
    froms[0] = N - 1
    for tgt in (target, poses[N // 3]):
        want = closest_ref(poses, labels, froms, tgt)
        got = rm.closest(froms, tgt)
        dev = [t.cpu().numpy() for t in rm.closest(_dev(froms), _dev(tgt))]
        for g in (got, dev):
            assert np.array_equal(g[0], want[0]) and np.array_equal(bits(g[1]), bits(want[1])) and np.array_equal(bits(g[2]), bits(want[2]))
    if N > 3:
        idx, dist, _ = rm.closest(froms[:1], target)
        assert idx[0] == 1 and dist[0] == 0.0  # the tie goes to the lowest index, whichever partition holds it
        poses2 = poses.copy()
        assert closest_ref(poses2, labels, froms[:1], target)[0][0] == 1
    rm.close()


def test_closest_with_the_best_only_in_the_last_partition(c):
    from closed_chain_motion_planner_amd import Roadmap, closest_ref

    N = 4099
    rng = np.random.default_rng(9)
    poses = np.zeros((N, 8))
    poses[:, :3] = rng.uniform(1, 2, (N, 3))
    poses[:, 6] = 1.0
    target = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0])
    poses[N - 1, :3] = 0.5
    rm = Roadmap(c, capacity_hint=N)
    rm.append(None, _dev(poses))
    chain = np.stack([np.arange(N - 1), np.arange(1, N)], axis=1).astype(np.int32)
    rm.add_edges(_dev(chain))
    idx, dist, fd = rm.closest(np.array([0, 7], np.int32), target)
    want = closest_ref(poses, np.zeros(N, np.int32), np.array([0, 7], np.int32), target)
    assert idx.tolist() == [N - 1, N - 1] and np.array_equal(bits(dist), bits(want[1])) and np.array_equal(bits(fd), bits(want[2]))
    assert rm.closest_from_goal([0], N - 1) == (N - 1, 0.0)
    assert rm.closest_from_goal([0, 7], N - 1) == (7, 0.0)  # the second from finds nothing STRICTLY better than 0: temp = from
    rm.close()


def test_closest_from_goal_is_the_references_loop(c):
    """closestVal carried across froms, temp = from unless strictly better, only the last from's vertex comes back"""
    from closed_chain_motion_planner_amd import Roadmap, pose_distance

    poses = np.zeros((8, 8))
    poses[:, 6] = 1.0
    poses[:, 0] = [5.0, 4.0, 3.0, 9.0, 6.0, 2.5, 7.0, 0.0]  # vertex 7 = `to`, alone; components {0,1,2}, {3,4}, {5,6}
    rm = Roadmap(c, capacity_hint=8)
    rm.append(None, _dev(poses))
    rm.add_edges(np.array([[0, 1], [1, 2], [3, 4], [5, 6]], dtype=np.int32))
    d = lambda i: pose_distance(poses[i], poses[7])
    assert rm.closest_from_goal([0], 7) == (2, d(2))
    assert rm.closest_from_goal([0, 3], 7) == (3, d(2))  # nothing in {3,4} beats 3.0: temp = from, the value stays
    assert rm.closest_from_goal([3, 6], 7) == (5, d(5))
    assert rm.closest_from_goal([2], 7) == (2, d(2))      # from itself is the best: not STRICTLY better
    assert rm.closest_from_goal([], 7) == (None, float("inf"))
    rm.close()
