"""The projector's two-launch form for large batches (closed_chain_motion_planner_amd/csrc/ccmp_kernels_fd.hip: FdPart): a head
launch runs the first `fd_head_rounds` Newton rounds of every sample, ten samples to a one-wavefront workgroup in index order,
and leaves a record per sample; the persistent kernel resumes from the records.  `fd_head_min_batch` is lowered so that the path is
taken at the smallest sizes where it can go wrong: a lone group (1), one workgroup exact and one either side (9, 10, 11), a
ragged last workgroup behind several (641), more workgroups than one generation of the resume grid's tickets (4 099).

Every case is compared bit for bit — rows, flags, iteration counts — with the det oracle, and with the same context at
fd_head_rounds = 0 (one launch, the form every other size takes)."""
import ctypes as C

import numpy as np
import pytest

from conftest import NCPU
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
SIZES = [1, 9, 10, 11, 641, 4099]
NMAX = max(SIZES)
_CACHE = {}


def _default_rounds():
    from closed_chain_motion_planner_amd import _lib

    return _lib.get_option(None, "fd_head_rounds") or 5  # (0 = the form is shipped switched off: test it where the sweep put it)


ROUNDS = ["one", "default", "past_the_cap"]


def _rounds(name):
    return {"one": 1, "default": _default_rounds(), "past_the_cap": 251}[name]


@pytest.fixture(scope="module")
def head_ctx(ccmp_built):
    """a context of this module's own: the throughput kernel alone at every size, scout order from one sample on, the head from one sample on"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from closed_chain_motion_planner_amd import Context

    ctx = Context(0)
    ctx.set_schedule(0, 0)
    ctx.set_lpt(1, 0)
    ctx.set_option("fd_head_min_batch", 0)
    return ctx


def _np(got):
    return got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy(), got[2].cpu().numpy().astype(np.int32)


def _both(ctx, n0, work):
    """work() with the head launch of n0 rounds, then on the same context without it"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    ctx.set_option("fd_head_rounds", n0)
    try:
        kind = _lib.CALL_PROJECT
        assert "(head)" in ctx.describe(kind, 1) and "no hand-over" in ctx.describe(kind, 1), ctx.describe(kind, 1)
        with_head = work()
        torch.cuda.synchronize()
        ctx.set_option("fd_head_rounds", 0)
        assert "(head)" not in ctx.describe(kind, 1)
        one_launch = work()
        torch.cuda.synchronize()
    finally:
        ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))
    return with_head, one_launch


def _same(a, b, what):
    for x, y, name in zip(a, b, ("rows", "ok", "iterations")):
        assert np.array_equal(x, y), (what, name, np.argwhere(x != y)[:4])


def _check(c, ctx, n0, q, ref, what):
    import torch

    qd = torch.as_tensor(np.ascontiguousarray(q)).cuda()
    got, plain = _both(ctx, n0, lambda: _np(c.project_batch(qd)))
    _same(got, plain, (what, "against one launch"))
    _same(got, (ref[0].view(np.uint64), ref[1], ref[2]), (what, "against the oracle"))


def _uniform(oracle, c, obj, seed, n):
    """n ambient samples of `obj` and the oracle's projection of them, computed once per (fixture, seed, n)"""
    key = (obj, seed, n)
    if key not in _CACHE:
        P = _oracle_problem(oracle, c)
        q = oracle.ambient_uniform_batch(P, seed, 0, n)
        _CACHE[key] = (q,) + oracle.project_batch(P, q, NCPU)
    return _CACHE[key]


@pytest.mark.parametrize("rounds", ROUNDS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_rounds(head_ctx, oracle_det, n, rounds):
    """uniform samples: at 1 round everything is resumed, at 251 (max_iter is 250) everything ends in the head and the resume launch
    meets finished records only.  (That it then WRITES nothing is not tested: the outputs can be looked at only behind both
    launches, where a row rewritten with the same bits cannot be told from one left alone; the kernel's text has no store to
    q_out, ok or iters outside the write-back of a sample it iterated on.)"""
    c = _constraint("Wine_Bottle", head_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    assert it_cpu.max() < 250 and it_cpu.min() > _default_rounds()  # every sample crosses the default head's end
    _check(c, head_ctx, _rounds(rounds), q[:n], (q_cpu[:n], ok_cpu[:n], it_cpu[:n]), (n, rounds))


@pytest.mark.parametrize("kind", ["on_the_manifold", "nearby", "mixed"])
def test_samples_that_end_inside_the_head(head_ctx, oracle_det, kind):
    """states already on the manifold (0 rounds), valid states moved by up to 0.05 rad (5 to 30 rounds: the quickest end in the head's
    last round or in the very evaluation the resume launch starts with, most later), and these half-and-half with uniform samples:
    the resume launch sees finished and live records side by side"""
    c = _constraint("Wine_Bottle", head_ctx)
    P = _oracle_problem(oracle_det, c)
    q, q_cpu, ok_cpu, _ = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    on = q_cpu[ok_cpu != 0][:641]
    assert len(on) == 641
    rng = np.random.default_rng(0x4EAE)
    near = on + rng.uniform(-0.05, 0.05, on.shape)
    if kind == "on_the_manifold":
        x = on
    elif kind == "nearby":
        x = near
    else:
        x = np.empty((1282, 14))
        x[0::4], x[2::4] = on[0::2], near[0::2][:320]  # finished, live, finished-early, live, ...
        x[1::2] = q[:641]
    ref = oracle_det.project_batch(P, x, NCPU)
    n0 = _default_rounds()
    if kind == "on_the_manifold":
        assert ref[2].max() == 0
    elif kind == "nearby":
        assert 0 < ref[2].min() and (ref[2] <= n0).any() and (ref[2] > n0).any()
    else:
        assert np.count_nonzero(ref[2] < n0) >= 321 and np.count_nonzero(ref[2] > n0) >= 641
    _check(c, head_ctx, n0, x, ref, kind)


def test_never_converging_samples_reach_the_cap_in_the_resume_launch(head_ctx, oracle_det):
    """stefan: some samples run all 250 rounds — the counters survive the record, the cap is met where it always was"""
    c = _constraint("stefan", head_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "stefan", 0x5C, 3000)
    assert it_cpu.max() == 250
    _check(c, head_ctx, _default_rounds(), q, (q_cpu, ok_cpu, it_cpu), "stefan")


@pytest.mark.parametrize("rounds", ROUNDS)
def test_fused_sampler(head_ctx, oracle_det, rounds):
    """sampleUniform: the head draws the ambient sample (and writes q_ambient), whichever launch ends a sample wraps it"""
    c = _constraint("Wine_Bottle", head_ctx)
    P = _oracle_problem(oracle_det, c)
    n, seed, first = 641, 0x4EAF, 5
    key = ("sampler", seed, first, n)
    if key not in _CACHE:
        _CACHE[key] = oracle_det.sample_project_batch(P, seed, first, n, NCPU)[:3] + (oracle_det.ambient_uniform_batch(P, seed, first, n),)
    q_cpu, ok_cpu, it_cpu, amb_cpu = _CACHE[key]

    def work():
        out = c.sample_project_batch(seed, first, n, want_ambient=True)
        return _np(out) + (out[3].cpu().numpy().view(np.uint64),)

    got, plain = _both(head_ctx, _rounds(rounds), work)
    _same(got[:3], plain[:3], (rounds, "against one launch"))
    _same(got[:3], (q_cpu.view(np.uint64), ok_cpu, it_cpu), (rounds, "against the oracle"))
    assert np.array_equal(got[3], amb_cpu.view(np.uint64)) and np.array_equal(plain[3], got[3])


def test_calibrated_arms_take_the_path(head_ctx, oracle_det):
    """the general instantiations (project_fd_kernel<2, false>, <4, false>): both fit the build's scratch rules and take the path"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", head_ctx)
    for arm in (0, 1):
        dh = (C.c_double * 28)(*[1e-3 * ((5 * i + 2 * arm) % 7 - 3) for i in range(28)])
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    P = _oracle_problem(oracle_det, c)
    q = oracle_det.ambient_uniform_batch(P, 0x4EB0, 0, 641)
    ref = oracle_det.project_batch(P, q, NCPU)
    _check(c, head_ctx, _default_rounds(), q, ref, "calibrated")


def test_more_than_one_generation_of_workgroups(head_ctx, oracle_det):
    """one sample more than the head workgroups the chip holds at once (twelve per CU) and one more take: the last workgroups are
    dispatched as the first retire, the very last holds a single sample — every row against one launch, the first and last 512
    against the oracle"""
    c = _constraint("Wine_Bottle", head_ctx)
    n = 10 * (12 * head_ctx.get_option("num_cus") + 1) + 1
    q = c.ambient_uniform_batch(0x4EB1, 0, n)
    got, plain = _both(head_ctx, _default_rounds(), lambda: _np(c.project_batch(q)))
    _same(got, plain, "against one launch")
    P = _oracle_problem(oracle_det, c)
    qh = q.cpu().numpy()
    for sl in (slice(0, 512), slice(n - 512, n)):
        ref = oracle_det.project_batch(P, qh[sl], NCPU)
        _same(tuple(a[sl] for a in got), (ref[0].view(np.uint64), ref[1], ref[2]), ("against the oracle", sl))


def test_in_place_call(head_ctx, oracle_det):
    """q_out on q_in (include/ccmp.h): the head overwrites the rows of the samples that end within its rounds — here every other
    row is on the manifold and ends in round 0 — so the scout runs in front of the head, not beside it; the describe line says so"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", head_ctx)
    P = _oracle_problem(oracle_det, c)
    q, q_cpu, ok_cpu, _ = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    x = np.empty((1282, 14))
    x[0::2] = q_cpu[ok_cpu != 0][:641]
    x[1::2] = q[:641]
    ref = oracle_det.project_batch(P, x, NCPU)
    assert np.count_nonzero(ref[2] == 0) >= 641 and np.count_nonzero(ref[2] > _default_rounds()) >= 641
    assert "in place" in head_ctx.describe(_lib.CALL_PROJECT, 1282) or _lib.get_option(None, "fd_head_rounds") == 0

    def work():
        qd = torch.as_tensor(x).cuda()
        out = c.project_batch(qd, out=qd)
        assert out[0].data_ptr() == qd.data_ptr()
        return _np(out)

    got, plain = _both(head_ctx, _default_rounds(), work)
    _same(got, plain, "in place, against one launch")
    _same(got, (ref[0].view(np.uint64), ref[1], ref[2]), "in place, against the oracle")


def test_index_order(head_ctx, oracle_det):
    """lpt 0: no scout, the resume launch takes the records in index order"""
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", head_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    head_ctx.set_lpt(0, 0)
    try:
        assert "FP32 scout" not in head_ctx.describe(_lib.CALL_PROJECT, NMAX)
        _check(c, head_ctx, _default_rounds(), q, (q_cpu, ok_cpu, it_cpu), "index order")
    finally:
        head_ctx.set_lpt(1, 0)
    assert "FP32 scout" in head_ctx.describe(_lib.CALL_PROJECT, NMAX)


def test_replays_from_a_graph(head_ctx, oracle_det):
    """scout beside the head on the side stream, then the resume launch: captured on one stream, replayed once"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", head_ctx)
    q, q_cpu, ok_cpu, it_cpu = _uniform(oracle_det, c, "Wine_Bottle", 0x4EAD, NMAX)
    qd = torch.as_tensor(q).cuda()
    head_ctx.set_option("fd_head_rounds", _default_rounds())
    try:
        assert "(head)" in head_ctx.describe(_lib.CALL_PROJECT, NMAX)
        c.project_batch(qd)  # eager: the workspaces grow before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            outs = c.project_batch(qd)
        for t in outs:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
    finally:
        head_ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))
    replayed = _np(outs)
    _same(replayed, (q_cpu.view(np.uint64), ok_cpu, it_cpu), "replay, against the oracle")
    head_ctx.set_option("fd_head_rounds", 0)
    try:
        one_launch = _np(c.project_batch(qd))
        torch.cuda.synchronize()
    finally:
        head_ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))
    _same(replayed, one_launch, "replay, against one launch")
