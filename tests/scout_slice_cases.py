"""The FP32 scout's predictions (closed_chain_motion_planner_amd/csrc/ccmp_kernels_scout.hip: scout_kernel, one contiguous slice of
the batch per wavefront, idle lanes refill from it) read back through ccmp_ctx_debug_lpt_pred.  NOT collected by the suite directly
(the default library exports no such symbol): tests/test_gpu_scout_slices.py runs this file once, in a process of its own, with
CCMP_LIBRARY = lib/libccmp_debug.so.  No reference numbers: a prediction depends on its sample alone, so it must not depend on the
batch around it, on the sample's place in the batch, or on what the buffer held before."""
import numpy as np
import pytest

from test_gpu_parity import _constraint

from closed_chain_motion_planner_amd import _lib

pytestmark = pytest.mark.gpu
CAP = 96  # the scout's cap on Newton updates (kScoutCap)
PAIR_MAX = 32768  # up to here the policy sends a stock batch to scout_pair_kernel (one block of 128 pairs per CU and sample pair at once)


@pytest.fixture(scope="module")
def rig(gpu_ctx):
    c = _constraint("Wine_Bottle", gpu_ctx)
    q = c.ambient_uniform_batch(0x5C07, 0, 40001)
    return c, gpu_ctx, q


def _pred(c, ctx, q):
    """predictions of the scout pass of one projector call on q"""
    n = q.shape[0]
    assert "FP32 scout" in ctx.describe(_lib.CALL_PROJECT, n), ctx.describe(_lib.CALL_PROJECT, n)
    c.project_batch(q.contiguous(), want_iters=False)
    pred = np.full(n, 0xFFFF, dtype=np.uint16)
    _lib.check(_lib.lib().ccmp_ctx_debug_lpt_pred(ctx.handle, pred.ctypes.data, n), "ccmp_ctx_debug_lpt_pred")
    return pred


def test_prediction_does_not_depend_on_the_batch_around_it(rig):
    """slice boundaries move with the batch size (16 384: a multiple of every grid; + 37: slices of unequal length, no multiple of 64;
    40 001: other slices altogether): the first 16 384 predictions stay what they are.  All three on scout_kernel (lane pairs off:
    below 32 769 samples the policy would send the first two to scout_pair_kernel, whose predictions may differ in a sum's last bit)."""
    c, ctx, q = rig
    ctx.set_option("scout_pairs", 0)
    try:
        a, b, d = (_pred(c, ctx, q[:n])[:16384] for n in (16384, 16384 + 37, 40001))
    finally:
        ctx.set_option("scout_pairs", 1)
    assert np.array_equal(a, b) and np.array_equal(a, d)
    assert a.max() <= CAP and len(np.unique(a)) > 20  # every entry written, and not by one constant


def test_few_samples_per_wavefront(rig):
    """the smallest batch the policy gives scout_kernel (latency kernel alone in the scout's order, lane pairs off): fewer samples
    than lanes in every wavefront, so no lane refills and some never get a sample"""
    c, ctx, q = rig
    n = 8 * ctx.num_cus + 53  # just past one sample per latency block
    ctx.set_option("scout_pairs", 0)
    ctx.set_option("latency_order_min", 0)
    try:
        assert "latency kernel alone" in ctx.describe(_lib.CALL_PROJECT, n)
        _pred(c, ctx, q[20000:20000 + n])  # other content first
        small = _pred(c, ctx, q[:n])
        full = _pred(c, ctx, q)
    finally:
        ctx.set_option("scout_pairs", 1)
        ctx.set_option("latency_order_min", _lib.get_option(None, "latency_order_min"))
    assert np.array_equal(small, full[:n]) and small.max() <= CAP


@pytest.mark.parametrize("n", [PAIR_MAX + 1, 40001, 16384 + 37])
def test_permuted_batch_gives_permuted_predictions(rig, n):
    """default policy: scout_kernel above 32 768 samples, scout_pair_kernel (untouched) below.  A batch of other content runs first,
    so that a lane that never wrote cannot hide behind the last call's value at the same place."""
    import torch

    c, ctx, q = rig
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(q.device)
    base = _pred(c, ctx, q[:n])
    other = c.ambient_uniform_batch(0x5C08, 0, n)
    assert not np.array_equal(_pred(c, ctx, other), base)
    got = _pred(c, ctx, q[:n][perm])
    assert np.array_equal(got, base[perm.cpu().numpy()])
    assert got.min() >= 0 and got.max() <= CAP
