"""The staged hand-over between the projector's two launches (closed_chain_motion_planner_amd/csrc/ccmp_kernels_fd.hip: FdPart): the
head stops BEHIND function(x) and the loop test of round `fd_head_rounds` and leaves, for every sample that goes on, what that evaluation
computed (ccmp_launch.h: kStagedRow); the resume launch admits a sample behind its finish block, straight into the Jacobian of the round
its predecessor ended in (stock twin arms; calibrated arms keep the earlier form).  No operation on any sample is added, removed or reordered, so every case is compared bit for bit — rows,
flags, iteration counts — with the det oracle, and with the same context at fd_head_rounds = 0 (one launch).

The path is forced with fd_head_min_batch = 1 and the persistent grid is shrunk to one wavefront per CU: 10 x num_cus group slots
(2 560 on 256 CUs), so that from 2 561 samples on groups admit a second sample behind the finish block; below that every admission is a
first fill — the same code path.  Sizes: a lone group (1), one workgroup exact and one either side (9, 10, 11), a ragged workgroup
behind several (61), one sample short of / past the grid's slots (2 559, 2 561), several admissions per group (4 099).

What no device test reaches: rot_x0_round_ok failing for an ADMITTED sample needs a joint within 4e-5 of a multiple of 2 pi (ccmp_kin.h) behind
several Newton rounds; inputs cannot place one there.  That the row's flag is the one the head's phase 1 computed is checked on the
rows themselves (tests/fd_staged_cases.py, on the debug library); the resume loop's ballot over the flags is covered by review."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import NCPU
from test_gpu_fd_head_resume import _both, _check, _np, _same, _uniform
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
SIZES = [1, 9, 10, 11, 61, 2559, 2561, 4099]
NMAX = 4099  # (the uniform batch of tests/test_gpu_fd_head_resume.py: one oracle run serves both modules)
ROUNDS = [1, 5, 251]


@pytest.fixture(scope="module")
def staged_ctx(ccmp_built):
    """a context of this module's own: the throughput kernel alone, scout order and the head from one sample on, one wavefront per CU"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from closed_chain_motion_planner_amd import Context

    ctx = Context(0)
    ctx.set_schedule(0, 0)
    ctx.set_lpt(1, 0)
    ctx.set_option("fd_head_min_batch", 1)
    ctx.set_waves_per_cu(1)
    return ctx


def _slots(ctx):
    return 10 * ctx.get_option("num_cus")


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_rounds(staged_ctx, oracle_det, n, rounds):
    """uniform samples (15 rounds and more each): at 1 and 5 rounds every sample is staged, at 251 (max_iter is 250) every sample ends in
    the head and the resume launch draws finished rows only"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", staged_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    assert it_cpu.max() < 250 and it_cpu.min() > 5
    if n > _slots(staged_ctx):
        assert "project_fd_kernel x %d wavefronts" % (_slots(staged_ctx) // 10) in staged_ctx.describe(_lib.CALL_PROJECT, n)
    _check(c, staged_ctx, rounds, q[:n], (q_cpu[:n], ok_cpu[:n], it_cpu[:n]), (n, rounds))


_STORE = {}


def _nearby(oracle_det, c, scale):
    """the batch's valid states moved by up to 0.05 * scale rad, and the oracle's projection of them (once per scale): at 0.1 they take
    0 to 16 rounds, two thirds of them 4, 5 or 6; at 0.03 they take 0 to 6, most of them 1 or 2"""
    if scale not in _STORE:
        P = _oracle_problem(oracle_det, c)
        _, q_cpu, ok_cpu, _ = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
        on = q_cpu[ok_cpu != 0][:900]
        assert len(on) == 900
        near = on + scale * np.random.default_rng(0x57A6).uniform(-0.05, 0.05, on.shape)
        _STORE[scale] = (near,) + tuple(oracle_det.project_batch(P, near, NCPU))
    return _STORE[scale]


def _mixed(oracle_det, c):
    """2 900 samples, more than the grid's group slots: 900 that end around the head's fifth round and 900 uniform ones (15 rounds and
    more) alternating, 1 100 more uniform ones behind them — with the oracle's answers"""
    near = _nearby(oracle_det, c, 0.1)
    uni = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    pair = lambda a, b: np.concatenate([np.stack([a, b[:900]], 1).reshape((1800,) + a.shape[1:]), b[900:2000]])
    return tuple(pair(a, b) for a, b in zip(near, uni))


@pytest.mark.parametrize("rounds", [1, 5])
def test_a_sample_that_ends_in_the_heads_last_evaluation(staged_ctx, oracle_det, rounds):
    """samples with EXACTLY `rounds` updates: the loop test that ends them is the one of the head's last phase 1 — the head writes them
    back there and stages nothing of them (that their rows are marked finished: tests/fd_staged_cases.py).  Beside them samples that
    take one round fewer and one more — ended a round earlier; staged and ended by the resume launch's first loop test — and others."""
    c = _constraint("Wine_Bottle", staged_ctx)
    x, q_cpu, ok_cpu, it = _nearby(oracle_det, c, 0.1 if rounds == 5 else 0.03)
    assert all(np.count_nonzero(it == k) >= 100 for k in (rounds - 1, rounds, rounds + 1)), np.bincount(it)
    _check(c, staged_ctx, rounds, x, (q_cpu, ok_cpu, it), ("last evaluation", rounds))


def test_finished_and_staged_rows_side_by_side(staged_ctx, oracle_det):
    """more samples than group slots, a third of them ending within the head: admissions behind the finish block draw finished rows
    between staged ones — in the scout's order, and in index order with a stretch sorted by rounds, where the finished rows come in
    runs far longer than the kResumeDraws draws of one admission (the group then waits a round) and the head stops at 8 rounds"""
    c = _constraint("Wine_Bottle", staged_ctx)
    x, q_cpu, ok_cpu, it = _mixed(oracle_det, c)
    assert len(x) > _slots(staged_ctx) and np.count_nonzero(it <= 5) >= 400 and np.count_nonzero(it > 8) >= 2000
    _check(c, staged_ctx, 5, x, (q_cpu, ok_cpu, it), "mixed")
    staged_ctx.set_lpt(0, 0)
    try:
        order = np.concatenate([np.argsort(it[:2000], kind="stable"), np.arange(2000, len(x))])
        _check(c, staged_ctx, 8, x[order], (q_cpu[order], ok_cpu[order], it[order]), "mixed, index order, runs of finished rows")
    finally:
        staged_ctx.set_lpt(1, 0)


def test_stefan_outlives_everything(staged_ctx, oracle_det):
    """stefan: samples that run all 250 rounds hold their groups while the neighbours admit sample after sample"""
    c = _constraint("stefan", staged_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "stefan", 0x5C, 3000)
    assert it_cpu.max() == 250 and len(q) > _slots(staged_ctx)
    _check(c, staged_ctx, 5, q, (q_cpu, ok_cpu, it_cpu), "stefan")


@pytest.mark.parametrize("rounds", ROUNDS)
def test_fused_sampler(staged_ctx, oracle_det, rounds):
    """sampleUniform (project_fd_kernel<3, true>, <5, true>): the head draws the ambient sample, whichever launch ends a sample wraps it"""
    c = _constraint("Wine_Bottle", staged_ctx)
    P = _oracle_problem(oracle_det, c)
    n, seed, first = 2600, 0x57A7, 3
    if "sampler" not in _STORE:
        _STORE["sampler"] = oracle_det.sample_project_batch(P, seed, first, n, NCPU)[:3] + (oracle_det.ambient_uniform_batch(P, seed, first, n),)
    q_cpu, ok_cpu, it_cpu, amb_cpu = _STORE["sampler"]
    assert n > _slots(staged_ctx)

    def work():
        out = c.sample_project_batch(seed, first, n, want_ambient=True)
        return _np(out) + (out[3].cpu().numpy().view(np.uint64),)

    got, plain = _both(staged_ctx, rounds, work)
    _same(got[:3], plain[:3], (rounds, "against one launch"))
    _same(got[:3], (q_cpu.view(np.uint64), ok_cpu, it_cpu), (rounds, "against the oracle"))
    assert np.array_equal(got[3], amb_cpu.view(np.uint64)) and np.array_equal(plain[3], got[3])


def test_calibrated_arms(staged_ctx, oracle_det):
    """the general instantiations (project_fd_kernel<2, false>, <4, false>) keep the hand-over record between the two launches and the
    refill at the loop top (their register allocation is pinned: tests/test_gpu_fd_round_facts.py); the workspace is sized for their
    rows, and on this grid their groups refill a second time"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", staged_ctx)
    for arm in (0, 1):
        dh = (C.c_double * 28)(*[1e-3 * ((5 * i + 2 * arm) % 7 - 3) for i in range(28)])
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    P = _oracle_problem(oracle_det, c)
    n = _slots(staged_ctx) + 41
    q = oracle_det.ambient_uniform_batch(P, 0x57A8, 0, n)
    ref = oracle_det.project_batch(P, q, NCPU)
    _check(c, staged_ctx, 5, q, ref, "calibrated")


def test_in_place_call(staged_ctx, oracle_det):
    """q_out on q_in: the head overwrites the rows of the samples it ends; the resume launch reads no input row at all"""
    import torch

    c = _constraint("Wine_Bottle", staged_ctx)
    x, q_cpu, ok_cpu, it = _mixed(oracle_det, c)
    full = (q_cpu, ok_cpu, it)
    assert len(x) > _slots(staged_ctx) and np.count_nonzero(it <= 5) >= 400

    def work():
        qd = torch.as_tensor(x).cuda()
        out = c.project_batch(qd, out=qd)
        assert out[0].data_ptr() == qd.data_ptr()
        return _np(out)

    got, plain = _both(staged_ctx, 5, work)
    _same(got, plain, "in place, against one launch")
    _same(got, (full[0].view(np.uint64), full[1], full[2]), "in place, against the oracle")


def test_replays_from_a_graph(staged_ctx, oracle_det):
    """head, scout beside it, sort and resume captured on one stream and replayed once: the workspace is sized by the eager call"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", staged_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    qd = torch.as_tensor(q).cuda()
    staged_ctx.set_option("fd_head_rounds", 5)
    try:
        assert "(head)" in staged_ctx.describe(_lib.CALL_PROJECT, NMAX)
        c.project_batch(qd)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = c.project_batch(qd)
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        replayed = _np(outs)
        staged_ctx.set_option("fd_head_rounds", 0)
        one_launch = _np(c.project_batch(qd))
        torch.cuda.synchronize()
    finally:
        staged_ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))
    _same(replayed, (q_cpu.view(np.uint64), ok_cpu, it_cpu), "replay, against the oracle")
    _same(replayed, one_launch, "replay, against one launch")


def test_staged_rows_on_the_debug_library(ccmp_built):
    """what the head leaves in the workspace — finished marks, counters, the x0 flag of the head's own phase 1, and nothing at all of a
    sample that its last loop test ends: tests/fd_staged_cases.py, once, in a process of its own against lib/libccmp_debug.so, which
    exports the read-back of the rows (ccmp_ctx_debug_fd_state; the default library does not)"""
    from closed_chain_motion_planner_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.exists(_lib.DEBUG_LIBPATH), "lib/libccmp_debug.so is built beside lib/libccmp.so (closed_chain_motion_planner_amd/build.py)"
    env = dict(os.environ, CCMP_LIBRARY=_lib.DEBUG_LIBPATH)
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "fd_staged_cases.py"), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"],
                         capture_output=True, text=True, timeout=300, cwd=root, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout, out.stdout[-500:]
