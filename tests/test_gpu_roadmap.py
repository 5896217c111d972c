"""The device-resident roadmap store (ccmp_roadmap_*) and the planner's tree metric on the device, bit for bit: the object metric
against tests/pose_knn_reference.py (one ccmp_pose_distance host call per pair, NaN dropped, the mode applied, lexsort by (distance,
index): indices equal, distances equal as uint64 views), derived poses against the oracle's compute_t_wo + a numpy R_to_quat, the
joint metric against ccmp_knn_batch, the store's semantics against a store filled in one append, ccmp_roadmap_connect against the
entry points it composes.

The launch shape is ccmp_policy.cpp's plan_knn_pose: up to 8 queries run the partitioned form (knn_pose_few_kernel, one block per
partition and query), more run one query per thread over LDS tiles of 512 poses (knn_pose_many_kernel); partitions hold at least 1024
poses (two tiles), so N = 4099 is five partitions — four of two tiles and one of three poses — in both forms."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_roadmap
from knn_reference import KNN_ALL, KNN_EARLIER, KNN_NOT_SELF
from pose_knn_reference import PoseDistanceTable, pose_of_numpy, reference
from test_gpu_parity import _constraint, _oracle_problem

from closed_chain_motion_planner_amd import _lib
from closed_chain_motion_planner_amd._lib import METRIC_JOINT, METRIC_OBJECT

pytestmark = pytest.mark.gpu

TILE, MIN_PARTITION, FEW_QUERIES = 512, 1024, 8
N_MAX, Q_MAX = 4099, 300
assert N_MAX > 3 * MIN_PARTITION + TILE and N_MAX % TILE != 0 and Q_MAX > FEW_QUERIES  # several partitions, a ragged last tile, both layouts


def _rm(c, joints=None, poses=None, hint=0):
    import torch
    from closed_chain_motion_planner_amd import Roadmap

    rm = Roadmap(c, hint)
    if joints is not None or poses is not None:
        rm.append(None if joints is None else torch.as_tensor(np.ascontiguousarray(joints)).cuda(),
                  None if poses is None else torch.as_tensor(np.ascontiguousarray(poses)).cuda())
    return rm


def _poses_of(c, joints):
    """the device-derived poses of joint states"""
    j, p = _rm(c, joints).read()
    assert np.array_equal(j.cpu().numpy().view(np.uint64), np.ascontiguousarray(joints).view(np.uint64))
    return p.cpu().numpy()


@pytest.fixture(scope="module")
def world(gpu_ctx):
    """nodes: the recorded roadmap's milestones, then valid projected Wine_Bottle samples; queries: fresh projected samples; the poses
    of both as the device derives them; their distances"""
    c = _constraint("Wine_Bottle", gpu_ctx)
    q, ok, _, _ = c.sample_project_batch(0x4B4E, 0, 32768, want_iters=False)
    good = q[ok != 0].cpu().numpy()
    road = load_roadmap("Wine_Bottle")[0]
    assert len(good) >= N_MAX - len(road) + Q_MAX
    nodes_j = np.ascontiguousarray(np.concatenate([road, good])[:N_MAX])
    queries_j = np.ascontiguousarray(good[-Q_MAX:])
    nodes_p, queries_p = _poses_of(c, nodes_j), _poses_of(c, queries_j)
    return {"c": c, "nj": nodes_j, "qj": queries_j, "np": nodes_p, "qp": queries_p, "table": PoseDistanceTable(queries_p, nodes_p)}


def _knn(rm, queries, k, mode=KNN_ALL, self_base=0, metric=METRIC_OBJECT):
    import torch

    idx, dist = rm.nearest_k(torch.as_tensor(np.ascontiguousarray(queries)).cuda(), k, metric, mode, self_base)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


@pytest.mark.parametrize("N", [1, 3, 64, 1000, N_MAX])
@pytest.mark.parametrize("Q", [1, 37, Q_MAX])
def test_shape_sweep(world, N, Q):
    rm = _rm(world["c"], world["nj"][:N], world["np"][:N])
    assert len(rm) == N
    for k in (1, 5, 16):
        got = _knn(rm, world["qp"][:Q], k)
        _same(got, world["table"].rank(k, n_nodes=N, n_queries=Q))
        assert (got[0] >= 0).sum() == Q * min(k, N) and np.all(np.isinf(got[1][got[0] < 0]))  # N < k: -1 / +inf slots


@pytest.mark.parametrize("mode", [KNN_NOT_SELF, KNN_EARLIER])
@pytest.mark.parametrize("s", [0, 17])
def test_modes(world, mode, s):
    """the queries are rows [s, s + Q) of the nodes"""
    nd = world["np"][:1300]  # two partitions
    rm = _rm(world["c"], world["nj"][:1300], nd)
    for Q in (5, 40):
        got = _knn(rm, nd[s: s + Q], 5, mode, s)
        _same(got, reference(nd, nd[s: s + Q], 5, mode, s))
        if mode == KNN_NOT_SELF:
            assert not np.any(got[0] == (s + np.arange(Q))[:, None])
        elif s == 0:
            assert np.all(got[0][0] == -1) and list(got[0][1]) == [0, -1, -1, -1, -1]


def test_ties_and_edge_cases(world):
    c, queries = world["c"], world["qp"]
    # exact duplicates of a pose at several indices, on both sides of a partition boundary: the lower indices first; the -q twin of a
    # pose is the same rotation: distance 0, ranked by its index among the duplicates
    nd = world["np"][:1500].copy()
    for j in (7, 400, 1023, 1024, 1499):
        nd[j] = nd[3]
    nd[400, 3:7] = -nd[3, 3:7]
    rm = _rm(c, None, nd)
    for qs in (nd[3:4], np.concatenate([nd[3:4], queries[:20]])):
        got = _knn(rm, qs, 5)
        _same(got, reference(nd, qs, 5))
        assert list(got[0][0]) == [3, 7, 400, 1023, 1024] and not got[1][0].any()
    twin = _knn(rm, nd[400:401], 2, KNN_NOT_SELF, 400)
    assert list(twin[0][0]) == [3, 7] and not twin[1][0].any()
    # NaN in a position or in a quaternion: never returned; a NaN query has no neighbour; an infinite position is a distance (the last)
    nd = world["np"][:1100].copy()
    nd[5, 1] = np.nan
    nd[1050, 6] = np.nan
    nd[9, 0] = np.inf
    qs = np.concatenate([nd[4:7], queries[:10]])
    qs[1] = nd[6]
    qs[2, 4] = np.nan
    rm = _rm(c, None, nd)
    for part in (qs[:3], qs):
        got = _knn(rm, part, 16)
        _same(got, reference(nd, part, 16))
        assert not np.any(np.isin(got[0], (5, 1050))) and np.all(got[0][2] == -1) and np.all(np.isinf(got[1][2]))
    got = _knn(_rm(c, None, nd[:12]), qs[:1], 16)
    assert got[0][0, 10] == 9 and np.isinf(got[1][0, 10]) and np.all(got[0][0, 11:] == -1)
    # the pad is written as 0 whatever the caller passed, and never read
    nd = world["np"][:40].copy()
    nd[:, 7] = np.nan
    rm = _rm(c, None, nd)
    assert not rm.read()[1].cpu().numpy()[:, 7].any()
    _same(_knn(rm, queries[:9], 5), world["table"].rank(5, n_nodes=40, n_queries=9))


def test_launch_shape_independence(world):
    rm = _rm(world["c"], world["nj"][:2500], world["np"][:2500])
    whole = _knn(rm, world["qp"][:12], 5)
    for q in range(12):  # one query per thread against the partitioned form
        one = _knn(rm, world["qp"][q: q + 1], 5)
        assert np.array_equal(one[0][0], whole[0][q]) and _same_bits(one[1][0], whole[1][q])
    line_few, line_many = (_lib.describe(world["c"].ctx.handle, _lib.CALL_ROADMAP_KNN, n) for n in (FEW_QUERIES, 16))
    assert "knn_pose_few_kernel" in line_few and "knn_pose_many_kernel" in line_many and "tiles of %d poses" % TILE in line_many
    assert "min_partition=%d" % MIN_PARTITION in line_many


@pytest.mark.parametrize("variant", [None, "calibrated", "tilted"])
def test_derived_poses(gpu_ctx, oracle_det, variant):
    """append(joints, poses=None): compute_t_wo of the left arm, then Quaterniond(Matrix3d), bit for bit; the arms' general
    instantiations (calibration offsets, a tilted base of the left arm) included"""
    c = _constraint("Wine_Bottle", gpu_ctx)
    if variant == "calibrated":
        dh = (C.c_double * 28)(*[1e-3 * ((7 * i) % 5 - 2) for i in range(28)])
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), 0, dh) == 0
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), 1, dh) == 0
    elif variant == "tilted":
        a, b = 0.3, -0.7
        Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
        Rz = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1]])
        for k, v in enumerate((Rz @ Rx).reshape(-1)):
            c.problem.base_R[k] = float(v)  # the left arm: the one compute_t_wo runs
        c.setInitialPosition(np.array(c.problem.start_joint[:]))
    P = _oracle_problem(oracle_det, c)
    rng = np.random.default_rng(11)
    q = np.concatenate([load_roadmap("Wine_Bottle")[0], rng.uniform(-2.8, 2.8, size=(70, 14))])  # 64-thread blocks: two, the second ragged
    got = _poses_of(c, q)
    from closed_chain_motion_planner_amd import pose_from_t_wo

    for i in range(len(q)):
        R, p = oracle_det.compute_t_wo(P, q[i, :7])
        assert _same_bits(got[i], pose_of_numpy(R.reshape(9), p)), (variant, i)
        assert _same_bits(got[i], pose_from_t_wo(np.concatenate([R.reshape(9), p])))


def test_joint_metric_equals_knn_batch(world):
    import torch

    c = world["c"]
    nodes, queries = torch.as_tensor(world["nj"]).cuda(), torch.as_tensor(world["qj"]).cuda()
    rm = _rm(c, world["nj"], world["np"])
    for Q, k in ((3, 5), (40, 16), (Q_MAX, 1)):
        want = c.nearest_k_batch(nodes, queries[:Q].contiguous(), k)
        got = rm.nearest_k(queries[:Q].contiguous(), k, METRIC_JOINT)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int64), want[1].view(torch.int64))
    # a pose-only vertex (growTree: the object pose is known, the joints are not yet): NaN joints, no joint query returns it ...
    first = rm.append(None, torch.as_tensor(world["qp"][:1].copy()).cuda())
    assert first == N_MAX and len(rm) == N_MAX + 1
    j, p = rm.read(N_MAX, 1)
    assert torch.isnan(j).all() and _same_bits(p.cpu().numpy()[0, :7], world["qp"][0, :7])
    want = c.nearest_k_batch(nodes, queries[:1].contiguous(), 16)
    got = rm.nearest_k(queries[:1].contiguous(), 16, METRIC_JOINT)
    assert torch.equal(got[0], want[0]) and N_MAX not in got[0].cpu().numpy()
    # ... while the object metric does (distance 0), and set_joints is visible to the next joint query
    near = rm.nearest_k(torch.as_tensor(world["qp"][:1].copy()).cuda(), 1)
    assert near[0].item() == N_MAX and near[1].item() == 0.0
    rm.set_joints(N_MAX, queries[0])
    got = rm.nearest_k(queries[:1].contiguous(), 2, METRIC_JOINT)
    assert got[0][0, 0].item() == N_MAX and got[1][0, 0].item() == 0.0 and got[0][0, 1].item() == want[0][0, 0].item()
    rm.set_joints(N_MAX, world["qj"][1])  # a host pointer
    assert rm.nearest_k(queries[1:2].contiguous(), 1, METRIC_JOINT)[0].item() == N_MAX
    assert _same_bits(rm.read(N_MAX, 1)[1].cpu().numpy()[0, :7], world["qp"][0, :7])  # the pose row stayed


def test_store_semantics(world):
    import torch
    from test_gpu_usage_modes import _capture_and_replay

    c, nj, npz, qp = world["c"], world["nj"], world["np"], world["qp"]
    whole = _rm(c, nj)  # one append, poses derived
    grown = _rm(c, hint=4)
    at = 0
    for n in (1, 7, 300, 3791):  # 4 -> 8 -> 308 -> 4099 rows: three growths
        assert grown.append(torch.as_tensor(nj[at: at + n]).cuda()) == at
        at += n
    assert at == N_MAX == len(grown) == len(whole)
    for a, b in zip(grown.read(), whole.read()):
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert _same_bits(whole.read()[1].cpu().numpy(), npz)
    for Q in (2, 37):
        _same(_knn(grown, qp[:Q], 5), world["table"].rank(5, n_queries=Q))
    # remove the tail, append again: indices restart there and the old tail is gone
    grown.truncate(1000)
    assert len(grown) == 1000
    _same(_knn(grown, qp[:37], 5), world["table"].rank(5, n_nodes=1000, n_queries=37))
    tail = np.ascontiguousarray(nj[2000:2050])
    assert grown.append(torch.as_tensor(tail).cuda()) == 1000 and len(grown) == 1050
    mixed = np.concatenate([npz[:1000], npz[2000:2050]])
    assert _same_bits(grown.read()[1].cpu().numpy(), mixed)
    _same(_knn(grown, qp[:37], 5), reference(mixed, qp[:37], 5))
    with pytest.raises(_lib.CcmpError):
        grown.truncate(1051)  # only what exists can be dropped
    # after reserve an append is asynchronous on its stream and a query enqueued behind it sees the new vertex: both are captured
    # into one graph (a synchronising call cannot be) and replayed
    grown.reserve(5000)  # moves the rows (synchronous); from here on no append up to 5000 vertices grows the store
    assert len(grown) == 1050 and _same_bits(grown.read()[1].cpu().numpy(), mixed)
    row, qrow = torch.as_tensor(nj[3000:3001].copy()).cuda(), torch.as_tensor(npz[3000:3001].copy()).cuda()

    def work():
        grown.truncate(1050)
        assert grown.append(row) == 1050
        return grown.nearest_k(qrow, 3)

    ref = _capture_and_replay(work)
    assert ref[0][0, 0].item() == 1050 and ref[1][0, 0].item() == 0.0
    _same((ref[0].cpu().numpy(), ref[1].cpu().numpy()), reference(np.concatenate([mixed, npz[3000:3001]]), npz[3000:3001], 3))


N_C, Q_C, K_C, MAXS = 400, 40, 5, 16


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("with_scene", [False, True])
@pytest.mark.parametrize("metric", [METRIC_JOINT, METRIC_OBJECT])
def test_connect_equals_its_parts(world, gpu_ctx, metric, with_scene, mode):
    """FD and analytic mode, with and without a proxy scene, both metrics: the neighbour block is ccmp_roadmap_knn's and every edge
    output is ccmp_geodesic_batch_ex's / ccmp_geodesic_scene_batch's on the gathered endpoints; three nodes leave two empty slots"""
    import torch
    from closed_chain_motion_planner_amd.scene import ProxyScene, default_allowed, skeleton_spheres

    c = _constraint("Wine_Bottle", gpu_ctx, mode=mode)
    nodes, queries = torch.as_tensor(world["nj"][100: 100 + N_C]).cuda(), torch.as_tensor(world["qj"][:Q_C]).cuda()
    qposes = torch.as_tensor(world["qp"][:Q_C]).cuda()
    scene = ProxyScene(c, skeleton_spheres(c.problem), (), default_allowed()) if with_scene else None
    margin = 0.02 if with_scene else None
    for n_nodes in (N_C, 3):
        rm = _rm(c)
        rm.append(nodes[:n_nodes].contiguous())
        idx, dist = rm.nearest_k(queries if metric == METRIC_JOINT else qposes, K_C, metric)
        got = {k: v.cpu().numpy() for k, v in rm.connect(queries, K_C, metric, None, check_target=True, max_states=MAXS, round_budget=32, scene=scene,
                                                         margin=margin).items()}
        assert np.array_equal(got["nbr_idx"], idx.cpu().numpy()) and _same_bits(got["nbr_dist"], dist.cpu().numpy())
        if metric == METRIC_OBJECT:  # given poses rank as the derived ones
            again = rm.connect(queries, K_C, metric, qposes, check_target=True, max_states=MAXS, round_budget=32, scene=scene, margin=margin)
            assert all(torch.equal(again[k].cpu(), torch.as_tensor(got[k])) for k in ("nbr_idx", "n_states", "ok", "newton_iters", "blocked"))
        flat = idx.reshape(-1).long()
        occ_t = flat >= 0
        occ = occ_t.cpu().numpy()
        assert occ.reshape(Q_C, K_C)[:, : min(K_C, n_nodes)].all() and occ.sum() == Q_C * min(K_C, n_nodes)
        to = queries.repeat_interleave(K_C, dim=0)[occ_t].contiguous()
        frm = nodes[flat[occ_t]].contiguous()
        if with_scene:
            w = [t.cpu().numpy() for t in c.discrete_geodesic_scene_batch(frm, to, scene, margin, MAXS, check_target=True, want_carry=True, round_budget=32)]
            w_blocked, w_carry = w[4], w[5]
        else:
            w = [t.cpu().numpy() for t in c.discrete_geodesic_batch(frm, to, MAXS, check_target=True, want_carry=True, round_budget=32)]
            w_blocked, w_carry = np.zeros(len(frm), np.uint8), w[4]
        for i, e in enumerate(np.flatnonzero(occ)):
            assert got["n_states"][e] == w[1][i] and got["ok"][e] == w[2][i] and got["newton_iters"][e] == w[3][i] and got["blocked"][e] == w_blocked[i], e
            assert _same_bits(got["states"][e, : min(int(w[1][i]), MAXS)], w[0][i, : min(int(w[1][i]), MAXS)]) and _same_bits(got["carry"][e], w_carry[i]), e
        emp = ~occ  # as connect_fix_kernel leaves them
        for key in ("ok", "n_states", "newton_iters", "blocked"):
            assert not got[key][emp].any(), key
        assert not got["carry"][emp].any()
        print("metric %d mode %d scene %d N %d: %d of %d edges reached, %d blocked" %
              (metric, mode, with_scene, n_nodes, int((got["ok"] == 1).sum()), int(occ.sum()), int(got["blocked"].sum())))


def test_python_host_forms(world, gpu_ctx):
    """numpy in, numpy out: the synchronous *_host entry points give the bits of the device forms"""
    import torch
    from closed_chain_motion_planner_amd import Roadmap

    c, nj, qj, qp = world["c"], world["nj"][:1500], world["qj"][:Q_C], world["qp"][:Q_C]
    dev = _rm(c, nj)
    host = Roadmap(c, 16)
    assert host.append(nj[:700]) == 0 and host.append(nj[700:]) == 700 and len(host) == 1500  # poses derived, one growth
    torch.cuda.synchronize()
    hj, hp = host.read(host=True)
    assert isinstance(hj, np.ndarray) and _same_bits(hj, nj) and _same_bits(hp, dev.read()[1].cpu().numpy())
    assert _same_bits(host.read(10, 5, host=True)[1], hp[10:15])
    for metric, qs in ((METRIC_OBJECT, qp), (METRIC_JOINT, qj)):
        for Q in (1, Q_C):
            got = host.nearest_k(qs[:Q], 5, metric)
            assert isinstance(got[0], np.ndarray) and got[0].dtype == np.int32
            _same(got, _knn(dev, qs[:Q], 5, metric=metric))
    # a pose-only vertex and its joints through the host forms
    assert host.append(None, qp[:1]) == 1500
    assert host.nearest_k(qp[:1], 1)[0][0, 0] == 1500 and np.isnan(host.read(1500, 1, host=True)[0]).all()
    host.truncate(1500)
    a = host.connect(qj[:8], 5, METRIC_OBJECT, check_target=True, max_states=MAXS, round_budget=32)
    b = {k: v.cpu().numpy() for k, v in dev.connect(torch.as_tensor(qj[:8]).cuda(), 5, METRIC_OBJECT, check_target=True, max_states=MAXS, round_budget=32).items()}
    assert np.array_equal(a["nbr_idx"], b["nbr_idx"]) and _same_bits(a["nbr_dist"], b["nbr_dist"])
    for key in ("n_states", "ok", "newton_iters", "blocked"):
        assert np.array_equal(a[key], b[key]), key
    assert _same_bits(a["carry"], b["carry"])
    for e in range(40):
        m = min(int(b["n_states"][e]), MAXS)
        assert _same_bits(a["states"][e, :m], b["states"][e, :m])
    # arguments
    L = _lib.lib()
    one = np.zeros(14)
    p = one.ctypes.data_as(C.POINTER(C.c_double))
    out = np.zeros(32, dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    assert L.ccmp_roadmap_knn_host(host._h, 2, p, 1, 1, 0, 0, out, None) == -1
    assert L.ccmp_roadmap_knn_host(host._h, 1, p, 1, 17, 0, 0, out, None) == -1
    assert L.ccmp_roadmap_knn_host(host._h, 1, p, 1, 1, 3, 0, out, None) == -1
    assert L.ccmp_roadmap_knn_host(host._h, 1, None, 0, 1, 0, 0, None, None) == 0  # Q == 0 touches nothing
    assert L.ccmp_roadmap_set_joints(host._h, 1500, p, None) == -1 and L.ccmp_roadmap_set_joints_host(host._h, 1500, p) == -1 and L.ccmp_roadmap_read_host(host._h, 1499, 2, p, None) == -1
    assert L.ccmp_roadmap_append_host(host._h, None, None, None, 1, None) == -1
    assert L.ccmp_roadmap_append_host(host._h, None, p, None, 1, None) == -1  # derived poses need the problem
    assert L.ccmp_roadmap_knn_host(None, 1, p, 1, 1, 0, 0, out, None) == -1  # with a device a NULL store is an argument error
    # everything is checked before anything is launched: a round budget without carries, an invalid problem
    bad = _lib.CcmpProblem.from_buffer_copy(bytes(c.problem))
    bad.tol_pos = 0.0
    st, n8, ok8 = np.zeros((5, MAXS, 14)), np.zeros(5, np.int32), np.zeros(5, np.uint8)
    args = lambda prob, budget: (host._h, C.byref(prob), None, 0.0, 1, qj[:1].ctypes.data_as(C.POINTER(C.c_double)), None, 1, 5, 0, 0, 1, MAXS, budget, out, None,
                                 st.ctypes.data_as(C.POINTER(C.c_double)), n8.ctypes.data_as(C.POINTER(C.c_int32)), ok8.ctypes.data_as(C.POINTER(C.c_uint8)),
                                 None, None, None)
    assert L.ccmp_roadmap_connect_host(*args(c.problem, 32)) == -1 and L.ccmp_roadmap_connect_host(*args(bad, 0)) == -1
    assert L.ccmp_roadmap_connect_host(*args(c.problem, 0)) == 0


# ---- every list size, merge width, node order and tie pattern under the object metric (tests/test_gpu_knn.py has the joint metric's) --
from knn_reference import MERGE_NARROW, described_shape, nodes_for_partitions, plan, plan_constants  # noqa: E402

K_SIZES = (2, 3, 4, 6, 8, 9, 15)
Q0 = np.array([0.5, 0.5, 0.5, 0.5])  # a unit quaternion whose products are exact
Q_OTHER = np.array([0.0, 0.0, 0.0, 1.0])


def _plan(c, Q, N):
    """(few form?, poses per partition, partitions) of an object-metric call on this chip"""
    return plan(c.ctx.num_cus, Q, N, TILE, *plan_constants(_lib.describe(c.ctx.handle, _lib.CALL_ROADMAP_KNN, Q)))


def _random_poses(rng, n):
    p = np.zeros((n, 8))
    p[:, :3] = rng.uniform(-1.0, 1.0, size=(n, 3))
    q = rng.normal(size=(n, 4))
    p[:, 3:7] = q / np.linalg.norm(q, axis=1)[:, None]
    return p


def test_plan_restated(world):
    c = world["c"]
    assert plan_constants(_lib.describe(c.ctx.handle, _lib.CALL_ROADMAP_KNN, 1)) == (FEW_QUERIES, MIN_PARTITION, 256)
    for Q in (1, FEW_QUERIES, FEW_QUERIES + 1, Q_MAX, 5000):  # the describe line assumes 65 536 poses
        line = _lib.describe(c.ctx.handle, _lib.CALL_ROADMAP_KNN, Q)
        few, part, partitions = _plan(c, Q, 65536)
        assert described_shape(line) == (partitions, part) and few == ("knn_pose_few_kernel" in line), line
    assert _plan(c, 1, N_MAX)[2] == _plan(c, Q_MAX, N_MAX)[2] == 5 and _plan(c, 37, 1000)[2] == 1


@pytest.mark.parametrize("N", [3, 1000, N_MAX])
@pytest.mark.parametrize("Q", [1, 37, Q_MAX])
def test_every_list_size(world, N, Q):
    c = world["c"]
    rm = _rm(c, world["nj"][:N], world["np"][:N])
    assert _plan(c, Q, N)[::2] == (Q <= FEW_QUERIES, 5 if N == N_MAX else 1)
    for k in K_SIZES:
        got = _knn(rm, world["qp"][:Q], k)
        _same(got, world["table"].rank(k, n_nodes=N, n_queries=Q))
        assert (got[0] >= 0).sum() == Q * min(k, N) and np.all(np.isinf(got[1][got[0] < 0]))


@pytest.mark.parametrize("mode", [KNN_NOT_SELF, KNN_EARLIER])
def test_modes_in_the_second_partition(world, mode):
    """queries = rows 1030 .. of 1 300 vertices (self_base in the second partition), and self_base + q >= N, where the mode excludes
    nothing"""
    c = world["c"]
    nd = world["np"][:1300]
    rm = _rm(c, world["nj"][:1300], nd)
    own = PoseDistanceTable(nd[1030:1070], nd)
    assert _plan(c, 5, 1300)[1:] == _plan(c, 40, 1300)[1:] == (1024, 2)
    for Q in (5, 40):
        for k in K_SIZES:
            got = _knn(rm, nd[1030: 1030 + Q], k, mode, 1030)
            _same(got, own.rank(k, mode, 1030, n_queries=Q))
            if mode == KNN_NOT_SELF:
                assert not np.any(got[0] == (1030 + np.arange(Q))[:, None])
            else:
                assert np.all(got[0] < (1030 + np.arange(Q))[:, None]) and np.all(got[0] >= 0)
    for s in (1295, 1300):
        for Q, k in ((5, 3), (40, 8), (40, 15)):
            got = _knn(rm, world["qp"][:Q], k, mode, s)
            _same(got, world["table"].rank(k, mode, s, n_nodes=1300, n_queries=Q))
            _same((got[0][max(0, 1300 - s):], got[1][max(0, 1300 - s):]),
                  tuple(a[max(0, 1300 - s):] for a in world["table"].rank(k, n_nodes=1300, n_queries=Q)))


# query 0's nearest poses are planted as in tests/test_gpu_knn.py: the last pose of each node count first, then the first, both sides of
# a partition boundary and indices across the range, so the lists that reach the result come from the highest merge threads too
PLANTED = (262144, 262143, 65536, 204800, 0, 1023, 1024, 32773, 40000, 66000, 100000, 131072, 200000, 230000, 250000, 261000)


@pytest.fixture(scope="module")
def big():
    """random positions with unit quaternions (k-NN does not need the manifold) and tables over them, made on demand and shared: a
    table over fewer poses or queries is a slice of one that exists"""
    state = {"nodes": np.empty((0, 8)), "tables": []}
    queries = _random_poses(np.random.default_rng(0xB16), 9)

    def get(Q, N):
        if N > len(state["nodes"]):  # (only on another CU count: the first request is the largest here)
            state["nodes"] = np.ascontiguousarray(np.concatenate([state["nodes"], _random_poses(np.random.default_rng(N), N - len(state["nodes"]))]))
            state["tables"] = []
            for r, j in enumerate(PLANTED):  # query 0's nearest poses, nearest first, whatever the node count: its rotation, 1e-3 apart in x
                if j < len(state["nodes"]):
                    state["nodes"][j] = queries[0]
                    state["nodes"][j, 0] += 1e-3 * (1 + r)
        for t in state["tables"]:
            if t.D.shape[0] >= Q and t.D.shape[1] >= N:
                return state["nodes"][:N], queries[:Q], t
        state["tables"].append(PoseDistanceTable(queries[:Q], state["nodes"][:N]))
        return state["nodes"][:N], queries[:Q], state["tables"][-1]

    return get


# on 256 CUs: 262 145 poses are past the clamp at 256 partitions (partitions of 1 536), 262 144 are 256 partitions, 65 537 are 65
@pytest.mark.parametrize("want,N256,Q", [(171, 262145, 1), (256, 262144, 1), (65, 65537, 9), (65, 65537, 1)])
def test_wide_merge(world, big, want, N256, Q):
    c = world["c"]
    consts = plan_constants(_lib.describe(c.ctx.handle, _lib.CALL_ROADMAP_KNN, Q))
    N = nodes_for_partitions(c.ctx.num_cus, Q, TILE, consts, want, N256)
    few, part, partitions = _plan(c, Q, N)
    assert partitions == want > MERGE_NARROW and few == (Q == 1) and partitions <= consts[2]
    assert (part > consts[1]) == (want == 171)  # past the clamp the partitions grow beyond their least size
    nodes, queries, table = big(Q, N)
    rm = _rm(c, None, nodes)
    for k in (3, 16):
        want_idx, want_dist = table.rank(k, n_nodes=N, n_queries=Q)
        if c.ctx.num_cus == 256:  # the planted poses are query 0's list: from the last partition down
            planted = [j for j in PLANTED if j < N][:k]
            assert list(want_idx[0, :len(planted)]) == planted and planted[0] // part == partitions - 1 and len(planted) >= min(k, 6)
        _same(_knn(rm, queries, k), (want_idx, want_dist))
    rm.close()


@pytest.mark.parametrize("order", ["descending", "ascending"])
def test_sorted_node_orders(world, order):
    """the vertices by decreasing reference distance to query 0: every one enters query 0's list and its bound shrinks at every insert;
    by increasing distance: the list is final after k vertices and the pre-filter on |dp| refuses what it can"""
    d = world["table"].D[0]
    perm = np.lexsort((np.arange(N_MAX), -d if order == "descending" else d))
    t = world["table"].take(perm)
    assert np.all(np.diff(t.D[0]) <= 0 if order == "descending" else np.diff(t.D[0]) >= 0)
    rm = _rm(world["c"], None, t.nodes)
    for Q in (1, 9):
        for k in (4, 16):
            _same(_knn(rm, world["qp"][:Q], k), t.rank(k, n_queries=Q))


def _pose_lattice(side):
    """4 099 poses on a side^3 lattice of step 0.125 (position index j mod side^3, so positions repeat), quaternions cycling through q0,
    -q0 (the same rotation) and one other with the next digit of j, in an order drawn from a fixed seed with three poses of the tie
    class of query 2 moved into the last partition (three poses).  Queries, all with q0: the zero position, 0.25 on every axis, 0.125
    on every axis.  Every |dp|^2 and every quaternion product is exact, so the distances are a few dozen values.  side = 16: all but
    three positions are distinct and the first places hold small ties; side = 3: about a hundred poses share each query's position
    and rotation — distance 0, ranked by the index alone."""
    j = np.arange(N_MAX)
    cell = j % side ** 3
    p = np.zeros((N_MAX, 8))
    for a in range(3):
        p[:, a] = 0.125 * ((cell // side ** a) % side)
    p[:, 3:7] = np.array([Q0, -Q0, Q_OTHER])[(j // side ** 3) % 3 if side == 3 else j % 3]
    p = p[np.random.default_rng(0x7135 + side).permutation(N_MAX)]
    queries = np.zeros((3, 8))
    queries[:, 3:7] = Q0
    queries[1, :3], queries[2, :3] = 0.25, 0.125
    tied = np.flatnonzero((p[:, :3] == 0.125).all(axis=1) & (np.abs(p[:, 3:7] @ Q0) == 1.0))
    last = np.arange(4 * MIN_PARTITION, N_MAX)
    swap = tied[tied < 4 * MIN_PARTITION][:len(last)]  # (side = 16: one pose; side = 3: three)
    last = last[:len(swap)]
    p[np.concatenate([last, swap])] = p[np.concatenate([swap, last])]
    return np.ascontiguousarray(p), queries


@pytest.fixture(scope="module")
def pose_lattices():
    out = {}
    for side in (16, 3):
        p, queries = _pose_lattice(side)
        out[side] = (p, queries, PoseDistanceTable(queries, p))
    return out


@pytest.mark.parametrize("side", [16, 3])
def test_lattice_ties(world, pose_lattices, side):
    c = world["c"]
    p, queries, table = pose_lattices[side]
    assert side != 3 or len(np.unique(table.D)) <= 96  # a few dozen distinct distances over 3 x 4 099 pairs
    part = _plan(c, 1, N_MAX)[1]
    assert _plan(c, 3, N_MAX)[2] == _plan(c, 9, N_MAX)[2] == 5
    rm = _rm(c, None, p)
    for k in (1, 4, 8, 16):
        if side == 3:  # at the k-th place, in every partition, for every query
            for q in range(3):
                ties = table.ties_at(k, q)
                assert len(ties) >= 50 and (q != 2 or set(ties // part) == set(range(5))), (k, q, len(ties))
                assert set(ties // part) >= set(range(4))
        for qs in (queries, np.concatenate([queries] * 3)):  # 3 queries: the partitioned form; 9: one query per thread
            got = _knn(rm, qs, k)
            _same(got, tuple(np.concatenate([a] * (len(qs) // 3)) for a in table.rank(k)))
            assert side != 3 or not got[1].any()  # the coarse lattice: k poses at distance 0 for every query
    print("side %d: ties at the k-th place, k = 1, 4, 8, 16, per query:" % side, [[len(table.ties_at(k, q)) for k in (1, 4, 8, 16)] for q in range(3)])


def test_lattice_ties_through_the_wide_merge(world, pose_lattices):
    """the coarse lattice tiled to 65 537 poses (pose j = lattice pose j mod 4 099), the three queries in the partitioned form: 65
    lists per query meet in knn_merge_kernel<KC, 256>"""
    c = world["c"]
    p, queries, table = pose_lattices[3]
    consts = plan_constants(_lib.describe(c.ctx.handle, _lib.CALL_ROADMAP_KNN, 3))
    N = nodes_for_partitions(c.ctx.num_cus, 3, TILE, consts, 65, 65537)
    t = table.take(np.arange(N) % N_MAX)
    assert _plan(c, 3, N)[2] == 65 > MERGE_NARROW and _plan(c, 3, N)[0]
    rm = _rm(c, None, t.nodes)
    for k in (4, 16):
        assert all(len(t.ties_at(k, q)) >= 50 * 15 for q in range(3))
        _same(_knn(rm, queries, k), t.rank(k))
    rm.close()


@pytest.mark.parametrize("term", ["rotation", "translation", "interleaved"])
def test_one_term_at_a_time(world, term):
    """every vertex at query 0's position with random rotations (d2 = 0 always passes the pre-filter: the rank is by rot alone); every
    vertex with query 0's quaternion (rot = 0: by |dp| alone); the two kinds alternating.  1 300 vertices, two partitions."""
    rng = np.random.default_rng({"rotation": 1, "translation": 2, "interleaved": 3}[term])
    queries = _random_poses(rng, 9)
    nodes = _random_poses(rng, 1300)
    same_place = np.ones(1300, bool) if term == "rotation" else np.zeros(1300, bool) if term == "translation" else np.arange(1300) % 2 == 0
    nodes[same_place, :3] = queries[0, :3]
    nodes[~same_place, 3:7] = queries[0, 3:7]
    table = PoseDistanceTable(queries, nodes)
    if term != "translation":  # the distances of the vertices at the query's position are their rotations: distinct, and not 0
        assert len(np.unique(table.D[0, same_place])) > 1000 * same_place.mean() and table.D[0, same_place].min() > 0
    rm = _rm(world["c"], None, nodes)
    assert _plan(world["c"], 1, 1300)[2] == 2
    for Q in (1, 9):
        for k in (1, 4, 16):
            _same(_knn(rm, queries[:Q], k), table.rank(k, n_queries=Q))
