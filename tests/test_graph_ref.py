"""The host forms of the roadmap graph (ccmp_roadmap_commit_ref, ccmp_graph_labels_ref, ccmp_roadmap_closest_ref, ccmp_joint_distance:
csrc/ccmp_graph.h compiled for the host, the same bits as the kernels) against checkers that share no text with them: the Python
restatement of growTree's tail on an edge-by-edge union-find, a numpy union-find, one ccmp_pose_distance call per pair.  Every
comparison is on integers or on bits.  No device."""
import numpy as np
import pytest

from conftest import config_path
from graph_cases import (BATCH_SHAPES, GREACHED, MS, ROOTS, SLOT_KINDS, SREACHED, TRAPPED, UNSETTLED, Graph, base_store, batch_case, bits, commit_args,
                         edge_weight, initial_edges, kind_counts, make_case, python_commit, same_commit, union_find_labels)

pytestmark = pytest.mark.usefixtures("ccmp_built")


@pytest.fixture(scope="module")
def api(ccmp_built):
    from closed_chain_motion_planner_amd import closest_ref, commit_ref, graph_labels_ref, joint_distance, load_config, pose_distance
    from graph_cases import OBJ

    class Api:
        pass

    a = Api()
    a.commit_ref, a.graph_labels_ref, a.closest_ref, a.joint_distance, a.pose_distance = commit_ref, graph_labels_ref, closest_ref, joint_distance, pose_distance
    a.P = load_config(config_path(OBJ))
    return a


def _ref(api, g, case):
    """commit_ref on the arrays of the Graph g as it stands"""
    sj, sp = g.arrays()
    return api.commit_ref(api.P, sj, sp, g.labels(), **commit_args(case))


def test_forty_sequential_commits(api):
    """Q = 1, k = 5, on one growing graph: every index, edge, weight bit, label and state equal at every step; the library's side keeps
    its own arrays (the returned rows and edges appended, the labels from graph_labels_ref on all edges so far)"""
    joints, poses, fresh, fresh_poses, goal = base_store()
    e0 = initial_edges(len(joints))
    g = Graph(joints, poses, e0)
    sj, sp, uv = np.array(joints), np.array(poses), np.array(e0)
    counts, states, mids = dict.fromkeys(SLOT_KINDS, 0), set(), 0
    for step in range(40):
        case = make_case(sj, sp, 1, 5, 500 + step, goal, fresh[step:step + 1], fresh_poses[step:step + 1], flags=1 if step % 7 == 3 else 0)
        for name, c in kind_counts(case).items():
            counts[name] += c
        labels = api.graph_labels_ref(uv, len(sj))
        assert np.array_equal(labels, g.labels()), step
        got = api.commit_ref(api.P, sj, sp, labels, **commit_args(case))
        want = python_commit(g, case)
        same_commit(got, want)
        sj, sp = np.concatenate([sj, got["rows_joints"]]), np.concatenate([sp, got["rows_poses"]])
        uv = np.concatenate([uv, got["edges_uv"]])
        states.add(int(got["grow_state"][0]))
        mids += int((got["mid_index"] >= 0).sum())
    assert np.array_equal(api.graph_labels_ref(uv, len(sj)), g.labels())
    assert all(counts[name] >= 5 for name in SLOT_KINDS), counts
    assert states == {TRAPPED, SREACHED, GREACHED, UNSETTLED} and mids >= 3, (states, mids)


def test_every_slot_kind_occurs_in_the_batches():
    total, mids = dict.fromkeys(SLOT_KINDS, 0), 0
    for Q, k in BATCH_SHAPES:
        case = batch_case(Q, k)[1]
        for name, c in kind_counts(case).items():
            total[name] += c
        if Q * k >= 60:
            assert all(c > 0 for c in kind_counts(case).values()), (Q, k, kind_counts(case))
    assert all(c >= 20 for c in total.values()), total


@pytest.mark.parametrize("Q,k", BATCH_SHAPES)
def test_batches(api, Q, k):
    g, case = batch_case(Q, k)
    got = _ref(api, g, case)
    want = python_commit(g, case)
    same_commit(got, want)
    if Q * k >= 60:
        assert (got["mid_index"] >= 0).any() and len(set(got["grow_state"].tolist())) >= 2


def test_the_batches_reach_every_state(api):
    seen = set()
    for Q, k in BATCH_SHAPES:
        g, case = batch_case(Q, k)
        seen |= set(_ref(api, g, case)["grow_state"].tolist())
    assert seen == {TRAPPED, SREACHED, GREACHED, UNSETTLED}


def _quirk_graph():
    """vertices 0 (the root) .. 9 of the base store; 0-1 and 2-3-4: the start's component and another one"""
    joints, poses, fresh, fresh_poses, goal = base_store()
    return Graph(joints[:10], poses[:10], [(0, 1), (2, 3), (3, 4)]), joints[:10], poses[:10], fresh, fresh_poses, goal


@pytest.mark.parametrize("order,expect_mid", [(("r2", "r0", "f3"), True), (("f3", "r2", "r0"), False), (("r2", "f3", "r0"), False)])
def test_the_component_quirk_both_ways(api, order, expect_mid):
    """a failed neighbour (3) in a non-start component AFTER a reached neighbour of that component (2) and a reached start neighbour (1)
    gives a mid-stone; the same slots in another order give none"""
    from closed_chain_motion_planner_amd import pose_distance

    g, joints, poses, fresh, fresh_poses, goal = _quirk_graph()
    d = np.array([pose_distance(p, goal) for p in poses])
    closer = int(np.argmin(d))
    assert closer != 3 and d[closer] < d[3]
    nbr, ok, ns = np.zeros((1, 3), np.int32), np.zeros(3, np.uint8), np.zeros(3, np.int32)
    states = np.zeros((3, MS, 14))
    for r, name in enumerate(order):
        n = {"r2": 2, "r0": 1, "f3": 3}[name]
        nbr[0, r], ok[r], ns[r] = n, name[0] == "r", 3
        states[r, :] = joints[n]
        states[r, 2] = joints[closer] if name == "f3" else fresh[0]
    case = {"nbr_idx": nbr, "edge_ok": ok, "n_states": ns, "states": states, "max_states": MS, "new_joints": np.array(fresh[:1]), "new_poses": np.array(fresh_poses[:1]),
            "vertex_ok": None, "goal_pose": np.array(goal), "roots": (0,), "flags": 0}
    got = _ref(api, g, case)
    same_commit(got, python_commit(g, case))
    assert got["grow_state"][0] == SREACHED and got["new_index"][0] == 10
    f3 = order.index("f3")
    assert (got["mid_index"][0, f3] == 11) == expect_mid and (got["mid_index"] >= 0).sum() == int(expect_mid)
    assert len(got["edges_uv"]) == 2 + int(expect_mid)
    if expect_mid:
        assert got["edges_uv"][2].tolist() == [3, 11] and np.array_equal(bits(got["rows_joints"][1]), bits(joints[closer]))


def _single(api, kinds, flags=0, vertex_ok=None, states=True, goal=True):
    joints, poses, fresh, fresh_poses, goal_pose = base_store()
    g = Graph(joints, poses, initial_edges(len(joints)))
    case = make_case(joints, poses, 1, len(kinds), 77, goal_pose, fresh, fresh_poses, kinds=[list(kinds)], flags=flags, with_vertex_ok=False)
    case["vertex_ok"] = vertex_ok
    if not states:
        case["states"] = None
    if not goal:
        case["goal_pose"] = None
    got = _ref(api, g, case)
    same_commit(got, python_commit(g, case))
    return got, len(joints)


def test_keep_isolated_vertex_ok_unsettled_and_the_lists_that_give_nothing(api):
    got, N = _single(api, ("failed_farther", "empty", "failed_zero"))
    assert got["grow_state"][0] == TRAPPED and got["new_index"][0] == -1 and len(got["rows_joints"]) == 0 and len(got["edges_uv"]) == 0
    got, N = _single(api, ("failed_farther", "empty", "failed_zero"), flags=1)  # startgoalMilestone: the vertex stays without an edge
    assert got["grow_state"][0] == TRAPPED and got["new_index"][0] == N and len(got["rows_joints"]) == 1 and len(got["edges_uv"]) == 0
    got, N = _single(api, ("reached", "failed_closer"), vertex_ok=np.zeros(1, np.uint8), flags=1)
    assert got["grow_state"][0] == TRAPPED and got["new_index"][0] == -1 and len(got["rows_joints"]) == 0
    for kind in ("unsettled_ok2", "unsettled_long"):
        got, N = _single(api, ("reached", kind, "failed_closer"))
        assert got["grow_state"][0] == UNSETTLED and got["new_index"][0] == -1 and len(got["rows_joints"]) == 0 and len(got["edges_uv"]) == 0
    for kind in ("failed_one", "failed_tie", "failed_nan", "failed_farther"):  # n_states = 1, the exact tie, a NaN last state, farther
        got, N = _single(api, ("reached", kind))
        assert (got["mid_index"] < 0).all() and len(got["edges_uv"]) == 1 and got["new_index"][0] == N, kind
    for kw in ({"states": False}, {"goal": False}):  # no lists / no goal: no mid-stones
        got, N = _single(api, ("reached", "failed_closer", "failed_closer"), **kw)
        assert (got["mid_index"] < 0).all() and len(got["edges_uv"]) == 1


def test_a_trapped_vertex_still_leaves_its_mid_stones(api):
    """no slot reached, but a failed neighbour in the start's component with a closer last state: the vertex goes, the mid-stone takes
    its index (stefanBiPRM.cpp:353-359)"""
    joints, poses, fresh, fresh_poses, goal = base_store()
    lab = union_find_labels(initial_edges(len(joints)), len(joints))
    g = Graph(joints, poses, initial_edges(len(joints)))
    case = make_case(joints, poses, 1, 2, 5, goal, fresh, fresh_poses, kinds=[["failed_closer", "failed_farther"]], with_vertex_ok=False)
    in_start = [int(i) for i in np.flatnonzero(lab == lab[ROOTS[0]])]
    from closed_chain_motion_planner_amd import pose_distance

    d = np.array([pose_distance(p, goal) for p in poses])
    n = next(i for i in in_start if d[i] > d.min())
    case["nbr_idx"][0, 0] = n
    case["states"][0, :case["n_states"][0] - 1] = joints[n]
    got = _ref(api, g, case)
    same_commit(got, python_commit(g, case))
    assert got["grow_state"][0] == TRAPPED and got["new_index"][0] == -1 and got["mid_index"][0].tolist() == [len(joints), -1]
    assert got["edges_uv"].tolist() == [[n, len(joints)]]


def test_joint_distance_is_the_knn_rule(api):
    joints = base_store()[0]
    for a, b in zip(joints[:50], joints[50:100]):
        assert api.joint_distance(a, b) == edge_weight(a, b)
    assert api.joint_distance(joints[0], joints[0]) == 0.0 and np.isnan(api.joint_distance(joints[0], np.full(14, np.nan)))


@pytest.mark.parametrize("N,E,seed", [(1, 0, 0), (2, 1, 1), (65, 40, 2), (1025, 700, 3), (4099, 4098, 4), (300, 2000, 5)])
def test_labels_ref_against_the_numpy_union_find(api, N, E, seed):
    rng = np.random.default_rng(seed)
    uv = rng.integers(0, N, size=(E, 2)).astype(np.int32)
    uv = np.ascontiguousarray(uv[uv[:, 0] != uv[:, 1]])
    assert np.array_equal(api.graph_labels_ref(uv, N), union_find_labels(uv, N))
    chain = np.stack([np.arange(N - 1), np.arange(1, N)], axis=1).astype(np.int32)[::-1]
    assert not api.graph_labels_ref(chain, N).any()


def closest_reference(pose_distance, poses, labels, froms, target):
    """one ccmp_pose_distance call per pair, masked by label, lexsort by (distance, index); NaN never a candidate"""
    d = np.array([pose_distance(p, target) for p in poses])
    idx, dist, fd = [], [], []
    for f in froms:
        cand = np.flatnonzero((labels == labels[f]) & ~np.isnan(d))
        if len(cand):
            best = cand[np.lexsort((cand, d[cand]))[0]]
            idx.append(best)
            dist.append(d[best])
        else:
            idx.append(-1)
            dist.append(np.inf)
        fd.append(d[f])
    return np.array(idx, np.int32), np.array(dist), np.array(fd)


def closest_store():
    """the base store's poses with duplicates (vertex 20 = 7, 150 = 7), NaN poses (30, 31), and labels with a singleton component"""
    joints, poses, _, _, goal = base_store()
    poses = np.array(poses)
    poses[20], poses[150] = poses[7], poses[7]
    poses[30, 4], poses[31, 0] = np.nan, np.nan
    labels = union_find_labels(initial_edges(len(poses), seed=11)[:60], len(poses))
    return poses, labels, goal


def test_closest_ref(api):
    poses, labels, goal = closest_store()
    sizes = np.bincount(labels, minlength=len(poses))
    single = int(np.flatnonzero(sizes[labels] == 1)[0])
    big = int(np.argmax(sizes))
    labels[[7, 20, 150, 30]] = big  # the duplicates and a NaN pose in the largest component
    froms = np.array([big, single, 7, 150, 31, 0, 5], dtype=np.int32)
    targets = [goal, poses[7], poses[single], poses[int(np.flatnonzero(labels == big)[3])]]  # free, the duplicated pose, vertices
    for target in targets:
        got = api.closest_ref(poses, labels, froms, target)
        want = closest_reference(api.pose_distance, poses, labels, froms, target)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(bits(got[2]), bits(want[2]))
    idx, dist, _ = api.closest_ref(poses, labels, froms, poses[7])
    assert idx[0] == 7 and dist[0] == 0.0 and idx[3] == 7  # duplicates: the lower index wins
    idx, dist, fd = api.closest_ref(poses, labels, np.array([single], np.int32), goal)
    assert idx[0] == single and dist[0] == fd[0]
    lone = np.array(labels)
    lone[31] = 31  # a component whose only pose is NaN: no candidate
    idx, dist, fd = api.closest_ref(poses, lone, np.array([31], np.int32), goal)
    assert idx[0] == -1 and dist[0] == np.inf and np.isnan(fd[0])
