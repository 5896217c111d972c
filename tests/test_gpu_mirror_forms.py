"""The mirror's two array kinds on a device (closed_chain_motion_planner_amd/_arrays.py): what the device kind refuses, where its outputs
land, and — for every call that is written once for both kinds — that the numpy form and the tensor form answer the same input with the
same bits.  Shapes are the smallest that reach every branch of a wrapper: a store of four vertices with one pose-only, Q = 2, k = 2,
max_states = 8, one path of three waypoints in rows of four, F = 0 and Q = 0 once each, every optional output asked for once."""
import numpy as np
import pytest

from object_cases import box_mesh, random_poses, workspace
from test_gpu_parity import _constraint

from closed_chain_motion_planner_amd._arrays import HOST, device_kind, kind_of
from closed_chain_motion_planner_amd._lib import METRIC_JOINT, METRIC_OBJECT

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
Q, K, MS, MARGIN = 2, 2, 8, -0.03
EDGE_KEYS = ("nbr_idx", "nbr_dist", "n_states", "ok", "newton_iters", "blocked", "carry")


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(a):
    return np.ascontiguousarray(a.cpu().numpy() if hasattr(a, "cpu") else a)


def _same(host, dev, what=""):
    """a numpy result and a tensor result: shape, width and every bit (uint32 masks are int32 tensors of the same bits)"""
    assert isinstance(host, np.ndarray) and not isinstance(dev, np.ndarray) and dev.is_cuda, what
    a, b = np.ascontiguousarray(host), _np(dev)
    assert a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes(), what


def _same_dict(host, dev, what, keys=None):
    assert list(host) == list(dev), what
    for key in keys if keys is not None else host:
        if isinstance(host[key], np.ndarray):
            _same(host[key], dev[key], (what, key))
        else:
            assert host[key] == dev[key], (what, key)


def _same_edges(host, dev, keys, what):
    """connect / grow: the named arrays, and the state lists up to what each edge stored (rows beyond n_states are not written)"""
    _same_dict(host, dev, what, keys)
    for e, n in enumerate(host["n_states"]):
        m = min(int(n), MS)
        _same(host["states"][e, :m], dev["states"][e, :m], (what, "states", e))


@pytest.fixture(scope="module")
def world(gpu_ctx):
    from closed_chain_motion_planner_amd import ProxyScene, ProxyValidityChecker, Roadmap, default_allowed, skeleton_spheres

    c = _constraint(OBJ, gpu_ctx)
    q, ok, _, _ = c.sample_project_batch(0x4B4E, 0, 1024, want_iters=False)
    joints = np.ascontiguousarray(q[ok != 0].cpu().numpy()[:12])
    assert len(joints) == 12
    rm = Roadmap(c, 16)
    rm.append(_dev(joints))
    poses = _np(rm.read()[1])
    rm.close()
    scene = ProxyScene(c, skeleton_spheres(c.problem), [ProxyValidityChecker.SUB_TABLE], default_allowed())
    return {"c": c, "joints": joints, "poses": poses, "scene": scene, "mesh": box_mesh(0.04, 0.04, 0.1), "boxes": workspace(),
            "obj_poses": random_poses(np.random.default_rng(5), 3)}


def _store(w, to=lambda a: a):
    """four vertices, vertex 3 pose-only, and the edges 0-1, 1-2; filled through the forms `to` selects (identity: numpy, _dev: tensors)"""
    from closed_chain_motion_planner_amd import Roadmap

    rm = Roadmap(w["c"], 16)
    assert rm.append(to(w["joints"][:3])) == 0 and rm.append(None, to(w["poses"][3:4])) == 3
    assert rm.add_edges(to(np.array([[0, 1], [1, 2]], dtype=np.int32))) == 0
    return rm


def _same_store(host, dev, what):
    for a, b in zip(host.read(host=True) + host.edges(host=True) + (host.labels(host=True),), dev.read() + dev.edges() + (dev.labels(),)):
        _same(a, b, what)


# ---- the device kind -------------------------------------------------------------------------------------------------------------------
def test_device_kind_expect_refuses_without_copying(gpu_ctx):
    import torch

    good = torch.zeros((4, 14), dtype=torch.float64, device="cuda")
    kind = kind_of(good)
    assert kind is not HOST and kind.device == good.device
    assert kind.expect(good, "float64", (None, 14), "rows") is good and kind.expect(good, "float64", 56, "rows") is good
    wide = torch.zeros((4, 28), dtype=torch.float64, device="cuda")
    for bad in (good.cpu(), good.float(), wide[:, ::2], torch.zeros((4, 13), dtype=torch.float64, device="cuda"), good.cpu().numpy()):
        with pytest.raises(ValueError):
            kind.expect(bad, "float64", (None, 14), "rows")
    with pytest.raises(ValueError):
        kind.expect(good, "float64", (3, 14), "rows")
    with pytest.raises(ValueError):
        kind.expect(good, "float64", 55, "rows")


def test_device_kind_arg_and_outputs(gpu_ctx):
    import torch

    ref = torch.zeros((0, 14), dtype=torch.float64, device="cuda")
    kind = kind_of(ref)
    assert kind.arg(None) is None and kind.arg(ref, empty_is_null=True) is None
    t = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert kind.arg(t) == t.data_ptr() and kind.arg(t, empty_is_null=True) == t.data_ptr()
    widths = {"float64": torch.float64, "int32": torch.int32, "uint8": torch.uint8, "uint32": torch.int32, "int16": torch.int16}
    for name, dtype in widths.items():
        e, z, f = kind.empty((2, 3), name), kind.zeros((2, 3), name), kind.full((2, 3), name, 7)
        for a in (e, z, f):
            assert a.dtype == dtype and tuple(a.shape) == (2, 3) and a.device == ref.device and a.is_contiguous()
        assert bool((z == 0).all()) and bool((f == 7).all())
    c = kind.copy_of(t)
    assert c.data_ptr() != t.data_ptr() and c.device == t.device and c.dtype == t.dtype
    assert device_kind(torch.device("cuda", gpu_ctx.device)).empty(1, "uint8").device.index == gpu_ctx.device


def test_outputs_land_on_the_reference_tensor(world):
    rm = _store(world, _dev)
    q = _dev(world["poses"][4:6])
    for out in rm.nearest_k(q, K) + rm.read() + tuple(world["c"].pose_ik_batch(q, _dev(world["joints"][4:6].reshape(2, 1, 14))).values()):
        assert out.device == q.device
    rm.close()


# ---- one text, two forms: the roadmap --------------------------------------------------------------------------------------------------
def test_store_append_set_joints_read(world):
    host, dev = _store(world), _store(world, _dev)
    _same_store(host, dev, "append")
    assert np.isnan(host.read(host=True)[0][3]).all()
    host.set_joints(3, world["joints"][3])
    dev.set_joints(3, _dev(world["joints"][3]))
    _same_store(host, dev, "set_joints")
    for a, b in zip(host.read(1, 2, host=True), dev.read(1, 2)):
        _same(a, b, "read(1, 2)")
    assert host.read(host=True)[0][3].tobytes() == world["joints"][3].tobytes()
    host.close()
    dev.close()


@pytest.mark.parametrize("n", [Q, 0])
def test_nearest_k_and_connect(world, n):
    rm = _store(world)
    qj, qp = world["joints"][4:4 + n], world["poses"][4:4 + n]
    for metric, queries in ((METRIC_OBJECT, qp), (METRIC_JOINT, qj)):
        for a, b in zip(rm.nearest_k(queries, K, metric), rm.nearest_k(_dev(queries), K, metric)):
            _same(a, b, ("nearest_k", metric))
            assert a.shape == (n, K)
    for kw in ({}, {"query_poses": True, "scene": world["scene"], "margin": MARGIN}):
        hk, dk = dict(kw), dict(kw)
        if kw:
            hk["query_poses"], dk["query_poses"] = qp, _dev(qp)
        _same_edges(rm.connect(qj, K, max_states=MS, **hk), rm.connect(_dev(qj), K, max_states=MS, **dk), EDGE_KEYS, ("connect", n, bool(kw)))
    rm.close()


@pytest.mark.parametrize("vet", [False, True])
def test_grow(world, vet):
    from closed_chain_motion_planner_amd import ik_options

    rm = _store(world)
    kw = dict(rng_seed=11, first_index=3, opts=ik_options(restarts=2), max_states=MS, scene=world["scene"], margin=MARGIN, vet=vet)
    host, dev = rm.grow(world["poses"][4:4 + Q], K, **kw), rm.grow(_dev(world["poses"][4:4 + Q]), K, **kw)
    keys = EDGE_KEYS[:2] + ("q_new", "ik_ok", "ik_which") + (("ik_clearance",) if vet else ()) + EDGE_KEYS[2:]
    assert [k for k in host if k != "states"] == list(keys)  # ik_clearance behind ik_which, and only with vet
    _same_edges(host, dev, keys, ("grow", vet))
    rm.close()


def test_commit_edges_labels_closest(world):
    """`connect`'s answers committed with state lists, a goal pose, roots and vertex flags: the two forms leave the same store behind"""
    host, dev = _store(world), _store(world, _dev)
    qj, qp = world["joints"][4:4 + Q], world["poses"][4:4 + Q]
    con = host.connect(qj, K, max_states=MS)
    args = (con["nbr_idx"], con["ok"], con["n_states"], qj, qp)
    kw = dict(goal_pose=world["poses"][9], roots=(0,), flags=1)
    a = host.commit(*args, states=con["states"], vertex_ok=np.ones(Q, np.uint8), **kw)
    b = dev.commit(*[_dev(x) for x in args], states=_dev(con["states"]), vertex_ok=_dev(np.ones(Q, np.uint8)), **kw)
    _same_dict(a, b, "commit")
    assert a["vertices_added"] >= 1 and list(a)[-2:] == ["vertices_added", "edges_added"]  # (a list of eight can leave a query unsettled)
    _same_store(host, dev, "commit")
    # without state lists, with a stated limit; goal_pose as a tensor
    a = host.commit(*args, max_states=MS, goal_pose=world["poses"][9])
    b = dev.commit(*[_dev(x) for x in args], max_states=MS, goal_pose=_dev(world["poses"][9]))
    _same_dict(a, b, "commit without states")
    _same_store(host, dev, "commit without states")
    for x, y in zip(host.edges(1, 1, host=True) + (host.labels(2, 3, host=True),), dev.edges(1, 1) + (dev.labels(2, 3),)):
        _same(x, y, "edges / labels of a range")
    froms = np.array([0, 3], dtype=np.int32)
    for x, y in zip(host.closest(froms, world["poses"][9]), host.closest(_dev(froms), _dev(world["poses"][9]))):
        _same(x, y, "closest")
    host.close()
    dev.close()


@pytest.mark.parametrize("max_len, full", [(4, True), (2, False)], ids=["fits-full", "retry"])
def test_shortest_paths(world, max_len, full):
    rm = _store(world)
    src, dst = np.array([0, 2], dtype=np.int32), np.array([2, 3], dtype=np.int32)
    host = rm.shortest_paths(src, dst, max_len=max_len, host=True, full=full)
    for dev in (rm.shortest_paths(src, dst, max_len=max_len, full=full), rm.shortest_paths(_dev(src), _dev(dst), max_len=max_len, full=full)):
        _same_dict(host, dev, ("shortest_paths", max_len))
    assert host["path_len"].tolist() == [3, 0] and host["path"].shape == (2, max(max_len, 3)) and ("dist" in host) == full
    assert host["path"][0, :3].tolist() == [0, 1, 2] and (host["path"][1] == -1).all() and np.isnan(host["joints"][1]).all() and np.isnan(host["poses"][1]).all()
    none = np.zeros(0, dtype=np.int32)
    _same_dict(rm.shortest_paths(none, none, max_len=max_len, host=True), rm.shortest_paths(none, none, max_len=max_len), "F = 0")
    rm.close()


# ---- one text, two forms: IK, paths, object, scene -------------------------------------------------------------------------------------
@pytest.mark.parametrize("vetted", [False, True])
def test_pose_ik(world, vetted):
    from closed_chain_motion_planner_amd import ik_options

    tp, seeds = world["poses"][4:6], np.ascontiguousarray(world["joints"][6:10].reshape(2, 2, 14))
    kw = dict(rng_seed=7, first_index=2, opts=ik_options(restarts=2), want_candidates=True)
    if vetted:
        kw.update(scene=world["scene"], margin=MARGIN)
    host, dev = world["c"].pose_ik_batch(tp, seeds, **kw), world["c"].pose_ik_batch(_dev(tp), _dev(seeds), **kw)
    assert len(host) == (8 if vetted else 5) and host["cand_q"].shape == (2, 2, 2, 3, 7)
    _same_dict(host, dev, ("pose_ik", vetted))


def _path(w, F=1):
    """one path of three waypoints in rows of four: a row behind its length"""
    pj = np.ascontiguousarray(w["joints"][:4].reshape(1, 4, 14))[:F]
    return pj, np.array([3], dtype=np.int32)[:F]


@pytest.mark.parametrize("F", [1, 0])
def test_densify(world, F):
    pj, pl = _path(world, F)
    for kw in ({}, {"scene": world["scene"], "margin": MARGIN, "distinct": True}):
        host, dev = world["c"].densify_paths(pj, pl, **kw), world["c"].densify_paths(_dev(pj), _dev(pl), **kw)
        _same_dict(host, dev, ("densify", F, bool(kw)))
        assert len(host) == (13 if kw else 9) and host["seg_first"].shape == (F, 3) and host["joints"].shape == (host["rows"], 14)


@pytest.mark.parametrize("F", [1, 0])
def test_shortcut_and_select(world, F):
    pj, pl = _path(world, F)
    host, dev = world["c"].shortcut_paths(pj, pl, pairs=True), world["c"].shortcut_paths(_dev(pj), _dev(pl), pairs=True)
    _same_dict(host, dev, ("shortcut", F))
    assert len(host) == 8 and host["pair_ok"].shape == (F, 4, 4)
    if F:
        assert host["joints"][0, 3].tobytes() == pj[0, 3].tobytes() and host["kept"][0, int(host["out_len"][0]):].tolist() == [-1] * (4 - int(host["out_len"][0]))
    from closed_chain_motion_planner_amd import shortcut_select

    sel_h = shortcut_select(world["c"].ctx, pj, pl, host["pair_ok"])
    sel_d = shortcut_select(world["c"].ctx, _dev(pj), _dev(pl), dev["pair_ok"])
    _same_dict(sel_h, sel_d, ("shortcut_select", F))
    plain = world["c"].shortcut_paths(_dev(pj), _dev(pl), scene=world["scene"], margin=MARGIN)
    _same_dict(world["c"].shortcut_paths(pj, pl, scene=world["scene"], margin=MARGIN), plain, ("shortcut with a scene", F))


@pytest.mark.parametrize("F", [1, 0])
def test_smooth(world, F):
    pj, pl = _path(world, F)
    for kw in ({"stats": True}, {"out_max_len": 4}, {"scene": world["scene"], "margin": MARGIN}):
        host = world["c"].smooth_paths(pj, pl, max_steps=1, **kw)
        dev = world["c"].smooth_paths(_dev(pj), _dev(pl), max_steps=1, **kw)
        _same_dict(host, dev, ("smooth", F, tuple(kw)))
        assert ("stats" in host) == ("stats" in kw) and host["joints"].shape == (F, 4 if "out_max_len" in kw else 7, 14)
        if F:
            assert host["joints"][0, int(host["out_len"][0]):4].tobytes() == pj[0, int(host["out_len"][0]):4].tobytes()


@pytest.mark.parametrize("n", [3, 0])
def test_object_valid_and_propose(world, gpu_ctx, n):
    from closed_chain_motion_planner_amd import ObjectChecker

    ch = ObjectChecker(gpu_ctx, world["mesh"], world["boxes"])
    poses = world["obj_poses"][:n]
    _same(ch.valid(poses), ch.valid(_dev(poses)), "valid")
    for a, b in zip(ch.valid(poses, want_mask=True), ch.valid(_dev(poses), want_mask=True)):
        _same(a, b, "valid with the mask")
    kw = dict(attempts=2, rng_seed=3, first_index=1, want_candidates=True)
    for goal in (world["obj_poses"][2], world["obj_poses"][2:3], world["obj_poses"][:n][::-1].copy()):
        host, dev = ch.propose(poses, goal, **kw), ch.propose(_dev(poses), _dev(goal), **kw)
        _same_dict(host, dev, ("propose", goal.shape))
        assert list(host) == ["pose", "which", "cand_pose", "cand_valid"] and host["cand_pose"].shape == (n, 2, 8)
    assert list(ch.propose(poses, world["obj_poses"][2], attempts=2)) == ["pose", "which"]
    ch.close()


def test_arm_clearance(world):
    q7 = np.ascontiguousarray(world["joints"][:3, 7:])
    for a, b in zip(world["scene"].arm_clearance_batch(1, q7, MARGIN), world["scene"].arm_clearance_batch(1, _dev(q7), MARGIN)):
        _same(a, b, "arm_clearance_batch")
    one = world["scene"].arm_clearance_batch(1, q7[0], MARGIN)
    many = world["scene"].arm_clearance_batch(1, q7.tolist(), MARGIN)  # no tensor: the host's
    assert isinstance(one[0], float) and isinstance(one[1], bool) and one[0] == many[0][0] and one[1] == bool(many[1][0])
