"""The rows that the projector's head launch leaves for its resume launch (closed_chain_motion_planner_amd/csrc/ccmp_launch.h:
kStagedRow), read back through ccmp_ctx_debug_fd_state.  NOT collected by the suite directly (the default library exports no such
symbol): tests/test_gpu_fd_staged_resume.py runs this file once, in a process of its own, with CCMP_LIBRARY = lib/libccmp_debug.so."""
import numpy as np
import pytest

from conftest import NCPU
from test_gpu_parity import _constraint, _oracle_problem

from closed_chain_motion_planner_amd import _lib

pytestmark = pytest.mark.gpu
LDS, F, TAG, NORM, X0 = 150, 150, 152, 154, 156  # the parts of a row, in doubles


def _rows(ctx, n):
    k = np.zeros(1, dtype=np.int32)
    _lib.check(_lib.lib().ccmp_ctx_debug_fd_state(ctx.handle, None, 0, k.ctypes.data), "ccmp_ctx_debug_fd_state")
    assert k[0] == 158
    rows = np.full((n, int(k[0])), np.nan)
    _lib.check(_lib.lib().ccmp_ctx_debug_fd_state(ctx.handle, rows.ctypes.data, n, k.ctypes.data), "ccmp_ctx_debug_fd_state")
    return rows


@pytest.mark.parametrize("rounds", [1, 5])
def test_rows_behind_a_call(gpu_ctx, oracle_det, rounds):
    """states on the manifold moved a little (0 to 16 rounds) and uniform ones (15 and more), head of `rounds` rounds.  A sample with at
    most `rounds` updates — with exactly `rounds`, the loop test of the head's last function(x) ends it — is marked finished and
    NOTHING of it is staged (the row's other doubles are what the previous call left: NaN painted over them shows it); every other row
    holds its index, the counters behind that loop test's increment, and the flag that its own sines and cosines call for"""
    import torch

    c = _constraint("Wine_Bottle", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    q = oracle_det.ambient_uniform_batch(P, 0x57A9, 0, 700)
    q_cpu, ok_cpu, _ = oracle_det.project_batch(P, q, NCPU)
    on = q_cpu[ok_cpu != 0][:120]
    near = on + (0.005 if rounds == 5 else 0.0015) * np.random.default_rng(0x57AA).uniform(-1, 1, on.shape)
    x = np.concatenate([near, q[:301]])
    it = oracle_det.project_batch(P, x, NCPU)[2]
    assert all(np.count_nonzero(it == k) >= 5 for k in (rounds - 1, rounds, rounds + 1)), np.bincount(it)[:10]
    gpu_ctx.set_schedule(0, 0)
    gpu_ctx.set_lpt(1, 0)
    gpu_ctx.set_option("fd_head_min_batch", 1)
    gpu_ctx.set_option("fd_head_rounds", 251)
    try:
        xd = torch.as_tensor(x).cuda()
        c.project_batch(xd)  # every row marked finished, whatever the workspace held
        gpu_ctx.set_option("fd_head_rounds", rounds)
        assert "(head)" in gpu_ctx.describe(_lib.CALL_PROJECT, len(x))
        before = _rows(gpu_ctx, len(x))
        assert (before[:, TAG].view(np.int64) == -1).all()
        got = c.project_batch(xd)
        assert np.array_equal(got[2].cpu().numpy().astype(np.int32), it)
        rows = _rows(gpu_ctx, len(x))
    finally:
        for name in ("fd_head_min_batch", "fd_head_rounds"):
            gpu_ctx.set_option(name, _lib.get_option(None, name))
        gpu_ctx.set_schedule(1, None)
        gpu_ctx.set_lpt(1, None)
    tag = rows[:, TAG].view(np.int64)
    ended = it <= rounds
    assert (tag[ended] == -1).all()
    keep = np.ones(158, dtype=bool)
    keep[TAG] = False
    assert np.array_equal(rows[ended][:, keep].view(np.uint64), before[ended][:, keep].view(np.uint64))  # nothing of them staged
    st = rows[~ended]
    assert np.array_equal(tag[~ended], np.flatnonzero(~ended))
    counters = st[:, TAG + 1].view(np.uint64)
    assert (counters & 0xFFFFFFFF == rounds + 1).all() and (counters >> 32 == rounds).all()  # iter behind the increment, updates
    tol_pos, tol_rot = P.tol_pos, P.tol_rot
    assert ((st[:, F] > tol_pos) | (st[:, F + 1] > tol_rot)).all()  # the loop test said go on
    assert np.isin(st[:, NORM], (0.0, 1.0)).all()  # norm1 = (f0 > tol1), the reference's quirk
    xs, sin, cos = st[:, :14], st[:, 14:42:2], st[:, 15:42:2]
    assert np.allclose(sin, np.sin(xs), atol=1e-15) and np.allclose(cos, np.cos(xs), atol=1e-15)
    flag = ((~(cos < 1.0 - 2.0 ** -30)) | (np.abs(xs) > 512.0)).any(axis=1)  # rot_x0_round_ok (ccmp_kin.h) on the row's own values
    assert np.array_equal(st[:, X0], flag.astype(np.float64))
    assert (st[:, X0 + 1] == 0.0).all()
