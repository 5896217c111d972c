"""The two cuts of the throughput kernel's STOCK instantiations (the short rotation and the folded base frame)
against the det oracle, bit for bit — joints, flags, iteration counts — at throughput-kernel size (> 10 240 samples):

  * the short rotation of the general joints is taken only by wavefronts none of whose samples holds a joint within 1e-8 of
    zero, so the batches carry rows with joints of exactly 0.0 — one joint, the four general joints, a whole arm — spread so that
    they share wavefronts (ten samples each) with ordinary rows: the guard's fall-back and the short form both run, side by side;
  * the base frame's +-1 factors are folded into the other arm's pose: Wine_Bottle (both frames the identity), stefan (arm 1 on
    base 2, d = (-1, -1, 1)) and stefan with its arms in the other order (arm 0 on base 2);
  * one bulk extend call runs the same Newton round inside geodesic_group_kernel, with edges whose joints stay exactly 0.0.

(The identities themselves are checked on the host by tests/test_rot_x0_host.py.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import NCPU
from test_gpu_parity import _constraint, _oracle_problem
from test_gpu_uniform_fastpaths import B, _near_and_far

pytestmark = pytest.mark.gpu


def _problem(name, gpu_ctx):
    from closed_chain_motion_planner_amd import _lib

    if name != "stefan_swapped":
        return _constraint(name, gpu_ctx)
    c = _constraint("stefan", gpu_ctx)
    assert list(c.problem.arm_index) == [0, 2]
    assert _lib.lib().ccmp_set_arms(C.byref(c.problem), b"panda_top", 2, b"panda_left", 0) == 0
    assert list(c.problem.arm_index) == [2, 0] and (c.problem.base_R[0], c.problem.base_R[4], c.problem.base_R[8]) == (-1.0, -1.0, 1.0)
    return c


def _with_zero_joints(q):
    """every third row gets joints of exactly 0.0 (so every wavefront of ten samples holds three or four such rows and six or
    seven ordinary ones): one joint in turn; every 15th row the general joints of both arms; every 33rd row all of arm 1"""
    q = q.copy()
    rows = np.arange(0, len(q), 3)
    q[rows, (rows // 3) % 14] = 0.0
    for j in (1, 3, 5, 6, 8, 10, 12, 13):
        q[::15, j] = 0.0
    q[::33, 7:] = 0.0
    q[5::330, :] = -0.0
    return np.ascontiguousarray(q)


@pytest.mark.parametrize("name", ["Wine_Bottle", "stefan", "stefan_swapped"])
def test_projection_bitwise_with_zero_joints_in_mixed_wavefronts(gpu_ctx, oracle_det, name):
    import torch

    c = _problem(name, gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    near, far = _near_and_far(c, oracle_det, P, 0xC075)
    mixed = np.empty_like(near)
    mixed[0::2], mixed[1::2] = near[0::2], far[1::2]
    assert len(mixed) > 10240
    for q in (_with_zero_joints(mixed), _with_zero_joints(near), np.ascontiguousarray(far)):
        q_gpu, ok_gpu, it_gpu = c.project_batch(torch.as_tensor(q).cuda())
        q_cpu, ok_cpu, it_cpu = oracle_det.project_batch(P, q, NCPU)
        assert np.array_equal(q_gpu.cpu().numpy().view(np.uint64), q_cpu.view(np.uint64))
        assert np.array_equal(ok_gpu.cpu().numpy(), ok_cpu)
        assert np.array_equal(it_gpu.cpu().numpy().astype(np.int32), it_cpu)
        assert 0 < int(ok_cpu.sum()) < len(q)  # both outcomes occur


def test_fused_sampler_bitwise(gpu_ctx, oracle_det):
    """project_fd_kernel<1, true> (sampleUniform: ambient sample, projection, enforceBounds in one kernel) carries the same cuts"""
    c = _problem("stefan", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    q_gpu, ok_gpu, it_gpu, _ = c.sample_project_batch(0xC076, 0, B)
    q_cpu, ok_cpu, it_cpu = oracle_det.sample_project_batch(P, 0xC076, 0, B, NCPU)[:3]
    assert np.array_equal(q_gpu.cpu().numpy().view(np.uint64), q_cpu.view(np.uint64))
    assert np.array_equal(ok_gpu.cpu().numpy(), ok_cpu)
    assert np.array_equal(it_gpu.cpu().numpy().astype(np.int32), it_cpu)


def test_extend_step_on_the_throughput_layout_bitwise(gpu_ctx, oracle_det):
    """every edge of a bulk extend call forced onto geodesic_group_kernel; a fifth of the edges keep one joint at exactly 0.0 in
    `from` and `to` — the interpolated states then hold that zero and their wavefronts take the fall-back.  Equal to the latency
    kernel's result everywhere and to the oracle's on a slice."""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _problem("stefan", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    E = 8 * gpu_ctx.num_cus + 1200
    q, ok, _, _ = c.sample_project_batch(0xC077, 0, 8 * E, want_iters=False)
    frm = q[ok == 1][:E].contiguous()
    assert frm.shape[0] == E
    to, _, _, _ = c.sample_near_project_batch(0xC078, 0, frm, 0.6, E, want_iters=False)
    rows = torch.arange(0, E, 5, device=frm.device)
    frm[rows, (rows // 5) % 14] = 0.0
    to[rows, (rows // 5) % 14] = 0.0
    cap, budget = 4, 30
    opts = ("geodesic_group", "geodesic_group_min", "geodesic_group_pred", "geodesic_group_permille", "geodesic_scout_min", "geodesic_group_handover_pct")
    try:
        gpu_ctx.set_option("geodesic_scout_min", 0)
        gpu_ctx.set_option("geodesic_group", 0)
        ref = c.discrete_geodesic_batch(frm, to, cap, want_carry=True, round_budget=budget)
        torch.cuda.synchronize()
        gpu_ctx.set_option("geodesic_group", 1)
        gpu_ctx.set_option("geodesic_group_min", 0)
        gpu_ctx.set_option("geodesic_group_pred", 1023)
        gpu_ctx.set_option("geodesic_group_permille", 0)
        gpu_ctx.set_option("geodesic_group_handover_pct", 0)
        got = c.discrete_geodesic_batch(frm, to, cap, want_carry=True, round_budget=budget)
        torch.cuda.synchronize()
    finally:
        for name in opts:
            gpu_ctx.set_option(name, _lib.get_option(None, name))
    live = torch.arange(cap, device=frm.device)[None, :] < ref[1].clamp(max=cap)[:, None]
    for k in (1, 2, 3, 4):
        assert torch.equal(got[k], ref[k]), k
    assert torch.equal(got[0][live], ref[0][live])
    assert int((got[1] > 1).sum()) > E // 2  # the edges were traversed
    st, n, okf, its, _ = got
    checked = 0
    for e in range(0, 200):
        if int(okf[e]) == 2:
            continue  # suspended by the round budget: the oracle's count is of the whole traversal
        ok_e, st_e, n_e, its_e, _ = oracle_det.discrete_geodesic_ex(P, frm[e].cpu().numpy(), to[e].cpu().numpy(), cap)
        assert int(n[e]) == n_e and bool(okf[e]) == bool(ok_e) and int(its[e]) == its_e, e
        assert np.array_equal(st[e, : min(n_e, cap)].cpu().numpy().view(np.uint64), st_e.view(np.uint64)), e
        checked += 1
    assert checked > 50
