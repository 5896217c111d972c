"""The object checker on the device (object_valid_kernel, object_propose_kernel; Roadmap.grow_toward) against the same text on the host.

ccmp_object_valid_ref / ccmp_object_propose_ref are the checkers: one text (csrc/ccmp_object.h) in one rounding model, so every output is
compared BIT FOR BIT.  Shapes are the smallest at which the kernels can go wrong: M = 1, 63, 64, 65 (a wavefront and its neighbours), 255,
256, 257 (a chunk of the block and its neighbours), 1 004 (four chunks, the last ragged); 1, 6 and 8 boxes; 1, 3 and 130 poses."""
import numpy as np
import pytest

from conftest import config_path, load_roadmap
from object_cases import box_mesh, dumbbell, quat_to_R, random_poses, soup, workspace

pytestmark = pytest.mark.gpu
OBJ = "Wine_Bottle"
MS = (1, 63, 64, 65, 255, 256, 257, 1004)
FREE = np.array([0.65, 0.0, 1.5, 0, 0, 0, 1, 0], dtype=np.float64)
LO, HI = (0.1, -0.5, 1.25), (1.2, 0.5, 1.8)


def boxes_n(n):
    """1: the table; 6: the fixture workspace; 8: that and two tilted boxes inside it"""
    ws = workspace()
    if n == 1:
        return ws[:1]
    tilted = [{"c": (0.5, 0.2, 1.55), "half": (0.1, 0.03, 0.06), "R": quat_to_R(np.array([0.1, 0.3, -0.2, 0.9]) / np.linalg.norm([0.1, 0.3, -0.2, 0.9]))},
              {"c": (0.9, -0.25, 1.4), "half": (0.04, 0.12, 0.05), "R": quat_to_R(np.array([-0.5, 0.2, 0.4, 0.7]) / np.linalg.norm([-0.5, 0.2, 0.4, 0.7]))}]
    return ws + tilted[:n - 6]


def mesh_m(M):
    return dumbbell() if M == 1004 else soup(np.random.default_rng(M), M)


def _bits(a):
    """the bytes of an array; every NaN as one canonical NaN (a NaN's sign and payload are not part of any result: the host's and the
    device's arithmetic generate different ones), everything else bit for bit"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    a = np.ascontiguousarray(a)
    if a.dtype == np.float64:
        a = np.where(np.isnan(a), np.nan, a)
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("n_boxes", [1, 6, 8])
@pytest.mark.parametrize("M", MS)
def test_valid_bit_for_bit_against_the_host_form(gpu_ctx, M, n_boxes):
    import torch
    from closed_chain_motion_planner_amd import ObjectChecker, object_valid_ref

    mesh, boxes = mesh_m(M), boxes_n(n_boxes)
    assert len(mesh) == M
    chk = ObjectChecker(gpu_ctx, mesh, boxes)
    assert len(chk) == M
    poses = random_poses(np.random.default_rng(1000 * M + n_boxes), 130)
    poses[7, 3:7] *= 1.2  # not normalised
    for T in (1, 3, 130):
        p = np.ascontiguousarray(poses[130 - T:])
        ref_valid, ref_mask = object_valid_ref(mesh, boxes, p, want_mask=True)
        pd = torch.from_numpy(p).cuda()
        valid, mask = chk.valid(pd, want_mask=True)
        quick = chk.valid(pd)  # the form that leaves at the first hit
        torch.cuda.synchronize()
        assert np.array_equal(valid.cpu().numpy(), ref_valid) and np.array_equal(mask.cpu().numpy().view(np.uint32), ref_mask), (T,)
        assert np.array_equal(quick.cpu().numpy(), ref_valid), (T,)
        inflated = chk.valid(pd, inflate=0.04, want_mask=True)
        ref_inflated = object_valid_ref(mesh, boxes, p, inflate=0.04, want_mask=True)
        assert np.array_equal(inflated[0].cpu().numpy(), ref_inflated[0]) and np.array_equal(inflated[1].cpu().numpy().view(np.uint32), ref_inflated[1])
    if M >= 63 and n_boxes >= 6:
        assert 0 < int(ref_valid.sum()) < 130  # both answers occur in the batch of 130
    # the host form: the same launch on staged buffers
    hv, hm = chk.valid(poses, want_mask=True)
    assert np.array_equal(hv, ref_valid) and np.array_equal(hm, ref_mask) and np.array_equal(chk.valid(poses), ref_valid)
    chk.close()


@pytest.mark.parametrize("M", MS)
def test_the_last_triangle_alone_is_found(gpu_ctx, M):
    """M - 1 small triangles around the object's origin, free at the pose, and triangle M - 1 alone 0.4 m above them, inside the ceiling:
    the last lane of the last chunk decides, against the last box only"""
    import torch
    from closed_chain_motion_planner_amd import ObjectChecker, object_valid_ref

    mesh = np.concatenate([soup(np.random.default_rng(M), M - 1, extent=0.03, size=0.02), soup(np.random.default_rng(1), 1, extent=0.0, size=0.02) + [0, 0, 0.4] * 3])
    boxes = workspace()
    chk = ObjectChecker(gpu_ctx, mesh, boxes)
    pd = torch.from_numpy(FREE.reshape(1, 8)).cuda()
    valid, mask = chk.valid(pd, want_mask=True)
    quick = chk.valid(pd)
    torch.cuda.synchronize()
    assert valid.item() == 0 and quick.item() == 0 and mask.item() == 1 << 5
    assert object_valid_ref(mesh, boxes, FREE, want_mask=True)[1][0] == 1 << 5
    if M > 1:
        without = ObjectChecker(gpu_ctx, mesh[:M - 1], boxes)
        assert without.valid(pd).item() == 1
        without.close()
    chk.close()


def test_a_nan_pose_is_not_tested_and_leaves_its_neighbours_alone(gpu_ctx):
    import torch
    from closed_chain_motion_planner_amd import ObjectChecker

    chk = ObjectChecker(gpu_ctx, dumbbell(), workspace())
    poses = random_poses(np.random.default_rng(4), 9)
    clean = chk.valid(torch.from_numpy(poses).cuda(), want_mask=True)
    bad = poses.copy()
    bad[4, 5] = np.nan
    bad[6, 0] = np.inf
    got = chk.valid(torch.from_numpy(bad).cuda(), want_mask=True)
    quick = chk.valid(torch.from_numpy(bad).cuda())
    torch.cuda.synchronize()
    keep = [i for i in range(9) if i not in (4, 6)]
    for a, b in zip(got, clean):
        assert torch.equal(a[keep], b[keep]) and (a[[4, 6]] == 0).all()
    assert torch.equal(quick, got[0])
    chk.close()


@pytest.mark.parametrize("A", [1, 2, 16])
@pytest.mark.parametrize("G", [1, 5, 130])
def test_propose_bit_for_bit_against_the_host_form(gpu_ctx, G, A):
    import torch
    from closed_chain_motion_planner_amd import ObjectChecker, object_propose_ref, pose_interpolate

    mesh, boxes = dumbbell(), workspace()
    chk = ObjectChecker(gpu_ctx, mesh, boxes)
    rng = np.random.default_rng(100 * G + A)
    frm = random_poses(rng, G, lo=(0.2, -0.45, 1.25), hi=(1.1, 0.45, 1.8))
    to = random_poses(rng, G, lo=(0.2, -0.45, 1.25), hi=(1.1, 0.45, 1.8))
    if G > 1:
        frm[G - 1, 2] = np.nan  # a grow index whose candidates are all non-finite
    kw = dict(t=0.3, sigma=0.2, lo=LO, hi=HI, attempts=A, rng_seed=0x0B1EC7, first_index=17)
    for goal in (to, to[:1]):  # to_stride 8 and 0
        ref = object_propose_ref(mesh, boxes, frm, goal, want_candidates=True, **kw)
        dev = chk.propose(torch.from_numpy(frm).cuda(), torch.from_numpy(np.ascontiguousarray(goal)).cuda(), want_candidates=True, **kw)
        quick = chk.propose(torch.from_numpy(frm).cuda(), torch.from_numpy(np.ascontiguousarray(goal)).cuda(), **kw)
        torch.cuda.synchronize()
        for name in ("pose", "which", "cand_pose", "cand_valid"):
            assert np.array_equal(_bits(dev[name]), _bits(ref[name])), (name, len(goal))
        for name in ("pose", "which"):
            assert np.array_equal(_bits(quick[name]), _bits(ref[name])), (name, len(goal))
        host = chk.propose(frm, np.ascontiguousarray(goal), want_candidates=True, **kw)  # the host form: the same launch
        for name in host:
            assert np.array_equal(_bits(host[name]), _bits(ref[name])), name
        if G > 1:
            assert ref["which"][G - 1] == -1 and np.isnan(ref["pose"][G - 1, :7]).all()
        if G == 130 and A >= 2:
            assert (ref["which"] == 0).any() and (ref["which"] > 0).any() and ref["cand_valid"].min() == 0
    # sigma = 0: the candidate is the interpolated pose itself
    z = chk.propose(torch.from_numpy(frm).cuda(), torch.from_numpy(to).cuda(), want_candidates=True, **dict(kw, sigma=0.0))
    torch.cuda.synchronize()
    cand = z["cand_pose"].cpu().numpy()
    for g in range(G - 1 if G > 1 else G):
        assert np.array_equal(cand[g, 0].view(np.uint64), pose_interpolate(frm[g], to[g], 0.3).view(np.uint64))
    chk.close()


def test_valid_batch_replays_from_a_graph(gpu_ctx):
    """one capture of valid_batch (both forms) into a HIP graph, after an eager call at that size: the replay gives the eager bits"""
    import torch
    from closed_chain_motion_planner_amd import ObjectChecker

    chk = ObjectChecker(gpu_ctx, dumbbell(), workspace())
    pd = torch.from_numpy(random_poses(np.random.default_rng(8), 130)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # the eager call, outside the capture
        eager = chk.valid(pd, want_mask=True)
        eager_quick = chk.valid(pd)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = chk.valid(pd, want_mask=True)
        cap_quick = chk.valid(pd)
    for x in (*cap, cap_quick):
        x.fill_(7)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap[0], eager[0]) and torch.equal(cap[1], eager[1]) and torch.equal(cap_quick, eager_quick)
    assert 0 < int(eager[0].sum()) < 130
    del g
    chk.close()


def test_ladder_equals_nine_valid_calls(gpu_ctx):
    from closed_chain_motion_planner_amd import ObjectChecker, pose_interpolate

    chk = ObjectChecker(gpu_ctx, dumbbell(), workspace())
    goal = np.array([0.65, 0.0, 1.0, 0, 0, 0.38268343236508978, 0.92387953251128674, 0])  # inside the table: the ladder walks into it
    for frm, want_all in ((FREE, False), (FREE + [0.1, 0.1, 0.1, 0, 0, 0, 0, 0], False), (goal, None)):
        poses, n = chk.ladder(frm, goal)
        assert poses.shape == (9, 8)
        flags = []
        for i in range(1, 10):
            step = pose_interpolate(frm, goal, 0.1 * i)
            assert np.array_equal(poses[i - 1].view(np.uint64), step.view(np.uint64))
            flags.append(int(chk.valid(step.reshape(1, 8))[0]))
        assert n == (flags.index(0) if 0 in flags else 9)
        if want_all is False:
            assert 0 < n < 9
        else:
            assert n == 0
    free_goal = FREE + [0.2, -0.1, 0.1, 0, 0, 0, 0, 0]
    assert chk.ladder(FREE, free_goal)[1] == 9
    chk.close()


def test_grow_toward_equals_propose_then_grow(gpu_ctx):
    """Roadmap.grow_toward on the recorded Wine_Bottle roadmap, a small cube as the object, the fixture workspace: its rows are those of
    propose followed by grow called by hand on the kept poses; indices with which = -1 never reach grow"""
    import torch
    from closed_chain_motion_planner_amd import KinematicChainConstraint, ObjectChecker, Roadmap

    c = KinematicChainConstraint.from_yaml(config_path(OBJ), ctx=gpu_ctx)
    nodes, _ = load_roadmap(OBJ)
    rm = Roadmap(c, capacity_hint=len(nodes))
    rm.append(joints=torch.from_numpy(nodes).cuda())
    _, poses = rm.read()
    chk = ObjectChecker(c, box_mesh(0.01, 0.01, 0.01), workspace())
    frm = torch.cat([poses, torch.full((1, 8), float("nan"), dtype=torch.float64, device=poses.device)]).contiguous()
    goal = poses[len(nodes) - 1:].contiguous()
    kw = dict(t=0.3, sigma=0.2, lo=LO, hi=HI, attempts=2, rng_seed=0x6A0, first_index=40)
    out = rm.grow_toward(chk, frm, goal, 3, max_states=8, **kw)
    prop = chk.propose(frm, goal, **kw)
    torch.cuda.synchronize()
    which = prop["which"].cpu().numpy()
    assert np.array_equal(out["which"].cpu().numpy(), which) and which[-1] == -1 and (which >= 0).any()
    rows = np.flatnonzero(which >= 0)
    assert np.array_equal(out["rows"], rows)
    kept = prop["pose"][torch.from_numpy(rows).cuda()].contiguous()
    assert torch.equal(out["poses"], kept) and not torch.isnan(kept).any()
    by_hand = rm.grow(kept, 3, rng_seed=0x6A0, first_index=40, max_states=8)
    torch.cuda.synchronize()
    assert set(by_hand) <= set(out)
    for name, want in by_hand.items():
        assert out[name].shape[0] in (len(rows), 3 * len(rows))
        if name == "states":  # rows beyond n_states are not written
            n = by_hand["n_states"].cpu().numpy()
            for e in range(len(n)):
                m = min(int(n[e]), 8)
                assert torch.equal(out[name][e, :m], want[e, :m]), (name, e)
        else:
            assert np.array_equal(_bits(out[name]), _bits(want)), name
    # the numpy form makes the same decisions
    out_h = rm.grow_toward(chk, frm.cpu().numpy(), goal.cpu().numpy(), 3, max_states=8, **kw)
    assert np.array_equal(out_h["which"], which) and np.array_equal(out_h["rows"], rows) and np.array_equal(_bits(out_h["q_new"]), _bits(by_hand["q_new"]))
    chk.close()
    rm.close()
