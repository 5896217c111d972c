"""The minimum-norm solve spread over a group's six lanes (closed_chain_motion_planner_amd/csrc/ccmp_fd_newton_phase2.inc) against the det oracle, bit for bit — joints, flags, iteration counts — at throughput-kernel size
(> 10 240 samples, so that every group slot of a wavefront refills while its neighbours are in the middle of a projection):

  * the throughput kernel alone (schedule 0) and the default policy; Wine_Bottle, stefan and dumbbell; the reference's tolerances
    and half of them;
  * the general instantiation: calibrated arms, and the stock problem sent through the general kernels;
  * the fused sampler (project_fd_kernel<1, true>);
  * one bulk extend call with every edge on geodesic_group_kernel, which includes the same text.

(The composition of the solve's pieces is checked on the host by tests/test_group_solve_host.py.)"""
import ctypes as C

import numpy as np
import pytest

from conftest import NCPU, OBJECTS
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
B = 12288


def _same(got, ref):
    q_gpu, ok_gpu, it_gpu = got[:3]
    q_cpu, ok_cpu, it_cpu = ref[:3]
    assert np.array_equal(q_gpu.cpu().numpy().view(np.uint64), q_cpu.view(np.uint64))
    assert np.array_equal(ok_gpu.cpu().numpy(), ok_cpu)
    assert np.array_equal(it_gpu.cpu().numpy().astype(np.int32), it_cpu)


@pytest.mark.parametrize("tol", [(1e-3, 5e-3), (5e-4, 2.5e-3)])
@pytest.mark.parametrize("obj", OBJECTS)
def test_projection_bitwise_throughput_kernel_alone_and_default_policy(gpu_ctx, oracle_det, obj, tol):
    import torch

    c = _constraint(obj, gpu_ctx)
    c.setTolerance(*tol)
    P = _oracle_problem(oracle_det, c)
    assert (P.tol_pos, P.tol_rot) == tol
    q = oracle_det.ambient_uniform_batch(P, 0x6507, 0, B)
    ref = oracle_det.project_batch(P, q, NCPU)
    assert 0 < int(ref[1].sum()) < B and ref[2].max() > 60
    for schedule in (0, 1):
        gpu_ctx.set_schedule(schedule, 0) if schedule == 0 else gpu_ctx.set_schedule(1)
        try:
            got = c.project_batch(torch.as_tensor(q).cuda())
            torch.cuda.synchronize()
        finally:
            gpu_ctx.set_schedule(1)
        _same(got, ref)


@pytest.mark.parametrize("calibrated", [True, False])
def test_general_instantiation_bitwise(gpu_ctx, oracle_det, calibrated):
    """project_fd_kernel<0, false>: calibrated arms (offsets differing per arm), and the stock problem with the stock kernels off"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", gpu_ctx)
    if calibrated:
        for arm in (0, 1):
            dh = (C.c_double * 28)(*[1e-3 * ((5 * i + 2 * arm) % 7 - 3) for i in range(28)])
            assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    P = _oracle_problem(oracle_det, c)
    q = oracle_det.ambient_uniform_batch(P, 0x6508, 0, B)
    ref = oracle_det.project_batch(P, q, NCPU)
    for schedule in (0, 1):
        gpu_ctx.set_schedule(schedule, 0) if schedule == 0 else gpu_ctx.set_schedule(1)
        gpu_ctx.set_option("stock_kernels", 0)
        try:
            got = c.project_batch(torch.as_tensor(q).cuda())
            torch.cuda.synchronize()
        finally:
            gpu_ctx.set_schedule(1)
            gpu_ctx.set_option("stock_kernels", 1)
        _same(got, ref)


@pytest.mark.parametrize("obj", ["Wine_Bottle", "stefan"])
def test_fused_sampler_bitwise(gpu_ctx, oracle_det, obj):
    c = _constraint(obj, gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    ref = oracle_det.sample_project_batch(P, 0x6509, 0, B, NCPU)
    for schedule in (0, 1):
        gpu_ctx.set_schedule(schedule, 0) if schedule == 0 else gpu_ctx.set_schedule(1)
        try:
            got = c.sample_project_batch(0x6509, 0, B)
        finally:
            gpu_ctx.set_schedule(1)
        _same(got, ref)


def test_extend_step_on_the_throughput_layout_bitwise(gpu_ctx, oracle_det):
    """every edge of a bulk extend call forced onto geodesic_group_kernel: equal to the latency kernel's result everywhere —
    states, counts, flags, Newton iterations, carried lengths — and to the oracle's on a slice"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    E = 8 * gpu_ctx.num_cus + 1200
    q, ok, _, _ = c.sample_project_batch(0x650A, 0, 8 * E, want_iters=False)
    frm = q[ok == 1][:E].contiguous()
    assert frm.shape[0] == E
    to, _, _, _ = c.sample_near_project_batch(0x650B, 0, frm, 0.6, E, want_iters=False)
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
