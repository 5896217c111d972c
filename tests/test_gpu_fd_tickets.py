"""The throughput kernel's tickets (closed_chain_motion_planner_amd/csrc/ccmp_kernels_fd.hip: the refill at the top of
project_fd_kernel's loop) at the smallest sizes where ticket arithmetic can go wrong.  S = 10 x the wavefronts the policy launches
(read from ccmp_ctx_describe): a batch of S - 1, S, S + 1 samples ends one short of, exactly at and one past the first fill of
every group slot, and 10 241 samples leave most groups without a sample.  (Written with a static first fill of the tickets, which
was measured slower and is not in the tree — DESIGN_experiments.md section 5.6; the sizes pin the queue's start whatever hands it out.)

For each size: every row, flag and iteration count equal to a second GPU run forced onto the latency kernel alone (complete and
cheap: that kernel takes no ticket from this queue), and the first and last 1 024 rows equal, bit for bit, to the det oracle."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import NCPU
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
EDGE = 1024


def _wavefronts(ctx, kind, n):
    m = re.search(r"project_fd_kernel x (\d+) wavefronts", ctx.describe(kind, n))
    assert m, ctx.describe(kind, n)
    return int(m.group(1))


def _full_fill(ctx, kind):
    """S with 10 x wavefronts(S) == S under the policy in force (the grid depends on the batch: a split launch leaves wavefronts out)"""
    s = 10 * _wavefronts(ctx, kind, 1 << 22)
    for _ in range(8):
        nxt = 10 * _wavefronts(ctx, kind, s)
        if nxt == s:
            return s
        s = nxt
    raise AssertionError("no batch size fills the throughput kernel's grid exactly")


def _np(got):
    return got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy(), got[2].cpu().numpy().astype(np.int32)


def _check_project(c, ctx, oracle, n, seed):
    import torch

    q = c.ambient_uniform_batch(seed, 0, n)
    got = _np(c.project_batch(q))
    ctx.set_schedule(2)
    try:
        ref = _np(c.project_batch(q))
        torch.cuda.synchronize()
    finally:
        ctx.set_schedule(1)
    for a, b, what in zip(got, ref, ("rows", "ok", "iterations")):
        assert np.array_equal(a, b), (n, what, np.argwhere(a != b)[:4])
    assert 0 < int(got[1].sum()) < n
    P = _oracle_problem(oracle, c)
    qh = q.cpu().numpy()
    for sl in (slice(0, EDGE), slice(n - EDGE, n)):
        q_cpu, ok_cpu, it_cpu = oracle.project_batch(P, qh[sl], NCPU)
        assert np.array_equal(got[0][sl], q_cpu.view(np.uint64)), (n, sl)
        assert np.array_equal(got[1][sl], ok_cpu) and np.array_equal(got[2][sl], it_cpu), (n, sl)


def _sizes(ctx):
    from closed_chain_motion_planner_amd import _lib

    s = _full_fill(ctx, _lib.CALL_PROJECT)
    split = next(n for n in (20000, 24000, 40000, 65536) if "split launch" in ctx.describe(_lib.CALL_PROJECT, n))
    return [10241, s - 1, s, s + 1, 16384 + 37, split]


def test_sizes_cover_the_kernel_and_its_launch_shapes(gpu_ctx):
    from closed_chain_motion_planner_amd import _lib

    sizes = _sizes(gpu_ctx)
    for n in sizes:
        assert "project_fd_kernel x" in gpu_ctx.describe(_lib.CALL_PROJECT, n), n
    s = sizes[2]
    assert 10 * _wavefronts(gpu_ctx, _lib.CALL_PROJECT, s) == s and 10 * _wavefronts(gpu_ctx, _lib.CALL_PROJECT, s + 1) == s
    assert 10 * _wavefronts(gpu_ctx, _lib.CALL_PROJECT, 10241) > 10241  # most wavefronts' groups get no sample
    assert "FP32 scout" in gpu_ctx.describe(_lib.CALL_PROJECT, 16384 + 37)


@pytest.mark.parametrize("which", range(6))
def test_project_bitwise_at_ticket_boundaries(gpu_ctx, oracle_det, which):
    c = _constraint("Wine_Bottle", gpu_ctx)
    _check_project(c, gpu_ctx, oracle_det, _sizes(gpu_ctx)[which], 0x71C0 + which)


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_plain_launch_alone_at_its_own_fill(gpu_ctx, oracle_det, delta):
    """the throughput kernel alone (no split, no hand-over): the fill of the FULL grid"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", gpu_ctx)
    gpu_ctx.set_schedule(0, 0)
    try:
        s = _full_fill(gpu_ctx, _lib.CALL_PROJECT)
        q = c.ambient_uniform_batch(0x71D0, 0, s + delta)
        got = _np(c.project_batch(q))
    finally:
        gpu_ctx.set_schedule(1)
    gpu_ctx.set_schedule(2)
    try:
        ref = _np(c.project_batch(q))
    finally:
        gpu_ctx.set_schedule(1)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b), (s + delta, np.argwhere(a != b)[:4])


def test_general_instantiation_at_the_fill(gpu_ctx, oracle_det):
    """project_fd_kernel<0, false>: calibrated arms at S + 1"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", gpu_ctx)
    for arm in (0, 1):
        dh = (C.c_double * 28)(*[1e-3 * ((5 * i + 2 * arm) % 7 - 3) for i in range(28)])
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    _check_project(c, gpu_ctx, oracle_det, _full_fill(gpu_ctx, _lib.CALL_PROJECT) + 1, 0x71E0)


def test_fused_sampler_at_the_fill(gpu_ctx, oracle_det):
    """project_fd_kernel<1, true>: sampleUniform at S + 1"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", gpu_ctx)
    n = _full_fill(gpu_ctx, _lib.CALL_SAMPLE_PROJECT) + 1
    assert "project_fd_kernel x" in gpu_ctx.describe(_lib.CALL_SAMPLE_PROJECT, n)
    got = _np(c.sample_project_batch(0x71F0, 0, n))
    gpu_ctx.set_schedule(2)
    try:
        ref = _np(c.sample_project_batch(0x71F0, 0, n))
    finally:
        gpu_ctx.set_schedule(1)
    for a, b in zip(got, ref):
        assert np.array_equal(a, b), np.argwhere(a != b)[:4]
    P = _oracle_problem(oracle_det, c)
    for first in (0, n - EDGE):
        q_cpu, ok_cpu, it_cpu = oracle_det.sample_project_batch(P, 0x71F0, first, EDGE, NCPU)[:3]
        sl = slice(first, first + EDGE)
        assert np.array_equal(got[0][sl], q_cpu.view(np.uint64)), first
        assert np.array_equal(got[1][sl], ok_cpu) and np.array_equal(got[2][sl], it_cpu), first
