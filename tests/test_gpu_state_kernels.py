"""The small per-state kernels and the stream compaction (the bottom of csrc/ccmp_kernels_fd.hip) at ragged sizes and edges.

Every comparison is bit for bit — int64 views of doubles, array_equal for bytes and integers — against the CPU oracle and the
plain restatements of tests/state_kernel_cases.py (proven on the CPU by tests/test_state_kernel_cases.py); the one liberty is
that a NaN matches a NaN, whose sign and payload IEEE 754 leaves open.  Every output buffer is one row (or byte, or word) longer
than the call is told and pre-filled with a sentinel, -7.0 or 0xA5, which must survive.  The calls go through the C ABI with the
test's own buffers where the Python wrapper would allocate the output itself."""
import ctypes as C
import math

import numpy as np
import pytest

import state_kernel_cases as sk
from conftest import NCPU, load_cfg
from test_gpu_parity import _constraint, _oracle_problem

from closed_chain_motion_planner_amd import _lib
from closed_chain_motion_planner_amd._lib import check
from closed_chain_motion_planner_amd.constraint import _stream_handle

pytestmark = pytest.mark.gpu

SENT = -7.0
SENT_BITS = int(np.float64(SENT).view(np.int64))
SENT_BYTE = 0xA5
CNT_GUARD = 0x5A5A5A5A5A5A5A5A


def _t():
    import torch

    return torch


def _dev(a):
    return _t().as_tensor(np.ascontiguousarray(a)).cuda()


def _rows(n, cols):
    """(n + 1, cols) doubles on the device, all sentinel: the call is told about n rows"""
    return _t().full((n + 1, cols), SENT, dtype=_t().float64, device="cuda")


def _bytes(n):
    return _t().full((n + 1,), SENT_BYTE, dtype=_t().uint8, device="cuda")


def _tail_intact(t, n):
    """rows (bytes) n.. of a sentinel-filled buffer are still the sentinel"""
    torch = _t()
    if t.dtype == torch.uint8:
        return bool((t[n:] == SENT_BYTE).all())
    return bool((t[n:].contiguous().view(torch.int64) == SENT_BITS).all())


def _same_bits_dev(got, want):
    """device tensors of doubles: the same bits everywhere"""
    torch = _t()
    return torch.equal(got.contiguous().view(torch.int64), want.contiguous().view(torch.int64))


def _L():
    return _lib.lib()


def _pp(c):
    return C.byref(c.problem)


# ---- raw calls with the test's own output buffers ----------------------------------------------------------------------------
def _function(c, q, B):
    f = _rows(B, 2)
    check(_L().ccmp_function_batch(c.ctx.handle, _pp(c), q.data_ptr(), f.data_ptr(), B, _stream_handle(None)), "ccmp_function_batch")
    return f


def _flags_call(name, c, q, B):
    ok = _bytes(B)
    check(getattr(_L(), name)(c.ctx.handle, _pp(c), q.data_ptr(), ok.data_ptr(), B, _stream_handle(None)), name)
    return ok


def _t_wo(c, q, B):
    out = _rows(B, 12)
    check(_L().ccmp_compute_t_wo_batch(c.ctx.handle, _pp(c), q.data_ptr(), q.shape[1], out.data_ptr(), B, _stream_handle(None)),
          "ccmp_compute_t_wo_batch")
    return out


def _uniform(c, seed, first, B):
    out = _rows(B, 14)
    check(_L().ccmp_ambient_uniform_batch(c.ctx.handle, _pp(c), seed, first, out.data_ptr(), B, _stream_handle(None)), "ccmp_ambient_uniform_batch")
    return out


# ---- stream compaction -----------------------------------------------------------------------------------------------------
_INDEX_ROWS = {}  # B -> (host rows, device rows): built once per size


def _index_rows(B):
    if B not in _INDEX_ROWS:
        h = sk.index_rows(B)
        _INDEX_ROWS[B] = (h, _dev(h))
    return _INDEX_ROWS[B]


def _check_compact(c, q_h, q_d, ok_h, via, cap=None, what=""):
    """one compaction of (q, ok) into a sentinel-filled buffer of `cap` rows plus a guard row, the count word starting as -1:
    the count, the first min(count, cap) rows as bits, the sentinel everywhere behind them"""
    torch = _t()
    B = q_h.shape[0]
    cap = B if cap is None else cap
    want_rows, want_n = sk.compact_restated(q_h, ok_h, cap)
    ok_d = _dev(ok_h)
    out = _rows(cap, 14)
    cnt = torch.tensor([-1, CNT_GUARD], dtype=torch.int64, device="cuda")
    if via == "wrapper":  # KinematicChainConstraint.compact_valid -> ccmp_compact_valid_capped
        r_out, r_cnt = c.compact_valid(q_d, ok_d, out=out[:cap], cnt=cnt[:1])
        assert r_out.data_ptr() == out.data_ptr() and r_cnt.data_ptr() == cnt.data_ptr()
    elif via == "plain":  # ccmp_compact_valid: the capacity is B
        assert cap == B
        check(_L().ccmp_compact_valid(c.ctx.handle, q_d.data_ptr(), ok_d.data_ptr(), B, out.data_ptr(), cnt.data_ptr(), _stream_handle(None)),
              "ccmp_compact_valid")
    else:
        check(_L().ccmp_compact_valid_capped(c.ctx.handle, q_d.data_ptr(), ok_d.data_ptr(), B, out.data_ptr(), cap, cnt.data_ptr(),
                                             _stream_handle(None)), "ccmp_compact_valid_capped")
    n, guard = cnt.cpu().tolist()
    tag = "B=%d cap=%d %s via %s" % (B, cap, what, via)
    assert guard == CNT_GUARD, tag
    assert n == want_n, "%s: count %d, expected %d" % (tag, n, want_n)
    m = min(want_n, cap)
    assert want_rows.shape[0] == m
    got = out.view(torch.int64)
    head_bad = (got[:m] != _dev(want_rows).view(torch.int64).reshape(m, 14)).any(dim=1)
    tail_bad = (got[m:] != SENT_BITS).any(dim=1)
    if bool(head_bad.any()) or bool(tail_bad.any()):  # only the mismatches come back
        hb, tb = head_bad.nonzero().flatten()[:6].cpu().tolist(), (tail_bad.nonzero().flatten()[:6] + m).cpu().tolist()
        msg = ["%s: %d of %d rows wrong, %d rows written behind them" % (tag, int(head_bad.sum()), m, int(tail_bad.sum()))]
        msg += ["  out[%d] = %r, expected %r" % (k, out[k].cpu().tolist()[:3], want_rows[k].tolist()[:3]) for k in hb]
        msg += ["  out[%d] = %r, expected the sentinel" % (k, out[k].cpu().tolist()[:3]) for k in tb]
        raise AssertionError("\n".join(msg))
    return n


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1023])
def test_compact_at_wavefront_and_block_boundaries(gpu_ctx, B):
    c = _constraint("Wine_Bottle", gpu_ctx)
    q_h, q_d = _index_rows(B)
    for pattern in sk.FLAG_PATTERNS:
        ok_h = sk.flags(B, pattern)
        for via in ("wrapper", "plain"):
            _check_compact(c, q_h, q_d, ok_h, via, what=pattern)


@pytest.mark.parametrize("pattern", ["p0.5", "last", "all"])
@pytest.mark.parametrize("B", [262144, 262145, 600001])
def test_compact_where_the_scan_chunks(gpu_ctx, B, pattern):
    """1 024 blocks: one per scan thread; 1 025: two per thread, thread 512 holds one and the later ones none; 2 344: three per
    thread, thread 781 holds one"""
    c = _constraint("Wine_Bottle", gpu_ctx)
    nblocks = (B + 255) // 256
    per = (nblocks + 1023) // 1024
    assert (nblocks, per) == {262144: (1024, 1), 262145: (1025, 2), 600001: (2344, 3)}[B]
    q_h, q_d = _index_rows(B)
    ok_h = sk.flags(B, pattern)
    for via in ("wrapper", "plain"):
        _check_compact(c, q_h, q_d, ok_h, via, what=pattern)


def test_compact_moves_nan_and_negative_zero_rows_as_bits(gpu_ctx):
    c = _constraint("Wine_Bottle", gpu_ctx)
    B = 257
    q_h = sk.index_rows(B)
    q_h[:, 1] = math.nan
    q_h[:, 2] = -0.0
    q_h[:, 3] = np.where(np.arange(B) % 2 == 0, math.inf, -math.inf)
    q_h[:, 4] = np.float64(5e-324)
    q_h[:, 5] = np.array([0x7FF0000000000001 + i for i in range(B)], dtype=np.uint64).view(np.float64)  # signalling NaNs with a payload
    q_d = _dev(q_h)
    for pattern in ("bytes", "all", "p0.5"):
        for via in ("wrapper", "plain"):
            _check_compact(c, q_h, q_d, sk.flags(B, pattern), via, what=pattern)


def test_compact_into_a_buffer_below_the_count(gpu_ctx):
    """rows past the capacity are dropped, the count is still complete (what distributed.py and ccmp_comm.cpp rely on)"""
    c = _constraint("Wine_Bottle", gpu_ctx)
    B = 1000
    q_h, q_d = _index_rows(B)
    for pattern in ("p0.5", "bytes"):  # both of density 0.5: flags 0 / 1, and flags 0 / 1 / 2 / 128 / 255
        ok_h = sk.flags(B, pattern)
        count = int((ok_h != 0).sum())
        assert 400 < count < 600
        for cap in (1, count - 1, count, count + 1):
            for via in ("wrapper", "capped"):
                assert _check_compact(c, q_h, q_d, ok_h, via, cap=cap, what=pattern) == count


def test_compact_count_word_and_shared_workspace(ccmp_built, gpu_ctx):
    """B = 0 clears the count and writes nothing else; then, on a context of its own, a small call, a large one (the scan
    workspace grows) and the small one again, which runs with the large call's counts lying behind its own"""
    torch = _t()
    from closed_chain_motion_planner_amd import Context

    c = _constraint("Wine_Bottle", gpu_ctx)
    q0 = torch.empty((0, 14), dtype=torch.float64, device="cuda")
    ok0 = torch.empty((0,), dtype=torch.uint8, device="cuda")
    for via in ("wrapper", "plain", "capped"):
        out = _rows(0, 14)
        cnt = torch.tensor([-1, CNT_GUARD], dtype=torch.int64, device="cuda")
        if via == "wrapper":
            c.compact_valid(q0, ok0, out=out[:0], cnt=cnt[:1])
        elif via == "plain":
            check(_L().ccmp_compact_valid(c.ctx.handle, None, None, 0, out.data_ptr(), cnt.data_ptr(), _stream_handle(None)), "ccmp_compact_valid")
        else:
            check(_L().ccmp_compact_valid_capped(c.ctx.handle, None, None, 0, out.data_ptr(), 0, cnt.data_ptr(), _stream_handle(None)),
                  "ccmp_compact_valid_capped")
        assert cnt.cpu().tolist() == [0, CNT_GUARD], via
        assert _tail_intact(out, 0), via
    own = Context(0)
    try:
        c2 = _constraint("Wine_Bottle", own)
        small, large = 300, 70001
        for B, pattern in ((small, "bytes"), (large, "all"), (small, "bytes"), (small, "none"), (small, "last")):
            q_h, q_d = _index_rows(B)
            _check_compact(c2, q_h, q_d, sk.flags(B, pattern), "wrapper", what=pattern)
    finally:
        torch.cuda.synchronize()
        own.close()


# ---- enforce_bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [19, 1, 18])
def test_enforce_bounds_on_edge_values(gpu_ctx, oracle_det, B):
    """19 rows = 266 doubles cross the 256-thread block, 18 rows = 252 do not"""
    c = _constraint("Wine_Bottle", gpu_ctx)
    v = sk.wrap_values()[:B]
    buf = _rows(B, 14)
    buf[:B] = _dev(v)
    ret = c.enforce_bounds_batch(buf[:B])
    assert ret.data_ptr() == buf.data_ptr()
    got = buf.cpu().numpy()
    assert _tail_intact(buf, B)
    want_o = np.array([oracle_det.enforce_bounds(r) for r in v])
    want_r = sk.wrap_restated(v)
    for name, want in (("oracle", want_o), ("restatement", want_r)):
        same = sk.same_bits(got[:B], want)
        assert same.all(), "%s: wrap(%r) = %r, expected %r" % (name, v[~same][:6], got[:B][~same][:6], want[~same][:6])
    fin = np.isfinite(got[:B])
    assert np.array_equal(fin, np.isfinite(v))
    assert (got[:B][fin] >= -math.pi).all() and (got[:B][fin] < math.pi).all()


# ---- joint_valid --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obj", ["Wine_Bottle", "stefan"])
def test_joint_valid_exactly_at_the_limits(gpu_ctx, oracle_det, obj):
    c = _constraint(obj, gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    rows = sk.limit_rows(c.problem)
    want = np.array([oracle_det.joint_valid(P, r) for r in rows], dtype=np.uint8)
    assert np.array_equal(want, sk.joint_valid_restated(P, rows)) and 0 < want.sum() < len(want)
    for B in (140, 1, 63, 64, 65, 257):
        ok = _flags_call("ccmp_joint_valid_batch", c, _dev(sk.fit_rows(rows, B)), B)
        got = ok.cpu().numpy()
        bad = np.flatnonzero(got[:B] != sk.fit_rows(want, B))
        assert bad.size == 0, "B=%d: rows %s (coordinate, kind: %s)" % (B, bad[:8], [(k % 140 // 10, sk.LIMIT_KINDS[k % 10]) for k in bad[:8]])
        assert _tail_intact(ok, B), B
    assert np.array_equal(c.joint_valid_batch(_dev(rows)).cpu().numpy(), want)
    # one state at a time: the device form on the ten values of a second-arm coordinate, the host form (it polls the completion
    # word behind the flag) on every row
    for k in range(100, 110):
        ok = _flags_call("ccmp_joint_valid_batch", c, _dev(rows[k: k + 1]), 1)
        assert ok.cpu().tolist() == [int(want[k]), SENT_BYTE], sk.LIMIT_KINDS[k % 10]
    single = np.array([c.jointValid(r) for r in rows], dtype=np.uint8)
    assert np.array_equal(single, want), np.flatnonzero(single != want)


# ---- is_satisfied -------------------------------------------------------------------------------------------------------------
def _nonfinite_rows(base):
    rows = []
    for e, v in ((2, math.nan), (9, math.nan), (0, math.inf), (13, -math.inf), (8, math.inf), (5, -math.inf)):
        r = base.copy()
        r[e] = v
        rows.append(r)
    return np.array(rows)


@pytest.mark.parametrize("kind", ["ambient", "projected"])
def test_is_satisfied_at_the_tolerance_itself(gpu_ctx, oracle_det, kind):
    """f == tolerance is satisfied (isSatisfied compares with <=, project with <); one ulp less on either residual is not"""
    c0 = _constraint("Wine_Bottle", gpu_ctx)
    P0 = _oracle_problem(oracle_det, c0)
    amb = oracle_det.ambient_uniform_batch(P0, 0x15A7, 0, 64)
    proj = [x for ok, x, _ in (oracle_det.project(P0, a) for a in amb) if ok][:8]
    assert len(proj) == 8
    x = amb[0] if kind == "ambient" else proj[0]
    f = oracle_det.function(P0, x)
    assert np.isfinite(f).all() and f[0] > 0 and f[1] > 0
    nonfinite = _nonfinite_rows(amb[1])
    pool = np.concatenate([x[None], amb[1:41], np.array(proj), nonfinite])  # 55 rows: whole in a batch of 63
    nf = np.arange(len(pool) - len(nonfinite), len(pool))
    for t0, t1, expect in ((f[0], f[1], True), (np.nextafter(f[0], 0), f[1], False), (f[0], np.nextafter(f[1], 0), False)):
        c = _constraint("Wine_Bottle", gpu_ctx)  # a fresh constraint
        c.setTolerance(t0, t1)
        Pb = oracle_det.problem_from_bytes(bytes(c.problem))
        assert (Pb.tol_pos, Pb.tol_rot) == (t0, t1)
        assert oracle_det.is_satisfied(Pb, x) is expect
        want_pool = np.array([oracle_det.is_satisfied(Pb, r) for r in pool], dtype=np.uint8)
        assert not want_pool[nf].any()
        for B in (1, 63, 64, 65):
            ok = _flags_call("ccmp_is_satisfied_batch", c, _dev(sk.fit_rows(pool, B)), B)
            got = ok.cpu().numpy()
            assert got[0] == int(expect), (t0, t1, B)
            assert np.array_equal(got[:B], sk.fit_rows(want_pool, B)), (t0, t1, B, np.flatnonzero(got[:B] != sk.fit_rows(want_pool, B)))
            assert _tail_intact(ok, B), B
            if B >= 63:
                assert not got[nf].any()
        assert c.isSatisfied(x) is expect
        assert np.array_equal(c.is_satisfied_batch(_dev(pool)).cpu().numpy(), want_pool)
    if kind == "ambient":  # the pool is a real mix under this tolerance
        assert 0 < want_pool.sum() < len(pool) - len(nonfinite)


# ---- function, compute_t_wo ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 64, 65])
def test_function_and_t_wo_at_ragged_sizes(gpu_ctx, oracle_det, B):
    c = _constraint("dumbbell", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    q = oracle_det.ambient_uniform_batch(P, 0xF7, 7, B)
    f = _function(c, _dev(q), B)
    f_want = oracle_det.function_batch(P, q, NCPU)
    assert np.array_equal(f[:B].cpu().numpy().view(np.uint64), f_want.view(np.uint64))
    assert _tail_intact(f, B)
    t_want = np.array([np.concatenate([R.reshape(9), p]) for R, p in (oracle_det.compute_t_wo(P, r[:7]) for r in q)])
    t14 = _t_wo(c, _dev(q), B)             # (B, 14): stride 14
    t7 = _t_wo(c, _dev(q[:, :7]), B)       # (B, 7): the same left arm, stride 7
    assert _tail_intact(t14, B) and _tail_intact(t7, B)
    assert _same_bits_dev(t14, t7)
    assert np.array_equal(t7[:B].cpu().numpy().view(np.uint64), t_want.view(np.uint64))
    assert _same_bits_dev(c.compute_t_wo_batch(_dev(q[:, :7])), t7[:B])


# ---- samplers -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [2 ** 32 - 3, 2 ** 32, 2 ** 40 + 5, 2 ** 63 - 2])
def test_ambient_uniform_far_above_32_bits(gpu_ctx, oracle_det, first):
    """the sample index is 64-bit (first + t / 14): the shards of a multi-GPU run sit far above 2^32"""
    torch = _t()
    c = _constraint("Wine_Bottle", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    seed = 0x5EED0001
    whole = None
    for B in (1, 18, 19, 257):
        out = _uniform(c, seed, first, B)
        want = oracle_det.ambient_uniform_batch(P, seed, first, B)
        got = out[:B].cpu().numpy()
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (B, np.flatnonzero((got != want).any(axis=1))[:8])
        assert _tail_intact(out, B), B
        whole = out[:B]
    a, b = _uniform(c, seed, first, 100), _uniform(c, seed, first + 100, 157)
    assert _same_bits_dev(torch.cat([a[:100], b[:157]]), whole)
    assert _same_bits_dev(c.ambient_uniform_batch(seed, first, 257), whole)
    # an index taken modulo 2^32 would give these instead (from row 3 on every one of the four offsets is past 2^32).  Not at
    # 2^63: the generator's counter is index * 14 modulo 2^64, in the oracle as in the kernel, so 2^63 + 1 and 1 are one sample
    if (first + 257) * 14 < 2 ** 64:
        assert not np.array_equal(oracle_det.ambient_uniform_batch(P, seed, (first + 3) % 2 ** 32, 4), whole[3:7].cpu().numpy())


@pytest.mark.parametrize("kind", ["near", "gaussian"])
def test_ambient_near_and_gaussian_far_above_32_bits(gpu_ctx, oracle_det, kind):
    torch = _t()
    c = _constraint("dumbbell", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    B, seed, first = 19, 0x77, 2 ** 40 + 5
    name = "ccmp_sample_near_project_batch" if kind == "near" else "ccmp_sample_gaussian_project_batch"
    ref_shared = np.array(load_cfg("dumbbell")["start_joint"])
    ref_each = oracle_det.ambient_uniform_batch(P, 5, 0, B)
    for ref, param in ((ref_shared, 0.3), (ref_each, 0.15)):
        ref_d = _dev(ref)
        out, amb, ok = _rows(B, 14), _rows(B, 14), _bytes(B)
        check(getattr(_L(), name)(c.ctx.handle, _pp(c), seed, first, ref_d.data_ptr(), 0 if ref.ndim == 1 else 14, param, out.data_ptr(),
                                  ok.data_ptr(), None, amb.data_ptr(), B, _stream_handle(None)), name)
        want = oracle_det.ambient_ref_batch(P, kind, seed, first, ref, param, B)
        assert np.array_equal(amb[:B].cpu().numpy().view(np.uint64), want.view(np.uint64))
        assert _tail_intact(amb, B) and _tail_intact(out, B) and _tail_intact(ok, B)
        fn = c.sample_near_project_batch if kind == "near" else c.sample_gaussian_project_batch
        q2, ok2, _, amb2 = fn(seed, first, ref_d, param, B, want_iters=False, want_ambient=True)
        assert _same_bits_dev(amb2, amb[:B]) and _same_bits_dev(q2, out[:B]) and torch.equal(ok2, ok[:B])
        assert not np.array_equal(oracle_det.ambient_ref_batch(P, kind, seed, first % 2 ** 32, ref, param, 4), want[:4])


# ---- host-pointer forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 65])
def test_host_pointer_forms_give_the_device_forms_bits(gpu_ctx, oracle_det, B):
    c = _constraint("Wine_Bottle", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    L, dp, u8p = _L(), C.POINTER(C.c_double), C.POINTER(C.c_uint8)
    amb = oracle_det.ambient_uniform_batch(P, 0x405, 0, 48)
    proj = np.array([x for ok, x, _ in (oracle_det.project(P, a) for a in amb) if ok][:6])
    assert len(proj) == 6
    lim = sk.limit_rows(c.problem)
    pool = np.concatenate([proj, amb[:20], _nonfinite_rows(amb[2]), lim[3:]])
    batches = [sk.fit_rows(pool, B)] if B > 1 else [pool[0:1].copy(), lim[3:4].copy(), amb[:1].copy()]  # valid and satisfied; outside the limits; neither
    for q in batches:
        f_h = np.full(2 * B + 1, SENT)
        s_h, j_h = np.full(B + 1, SENT_BYTE, dtype=np.uint8), np.full(B + 1, SENT_BYTE, dtype=np.uint8)
        check(L.ccmp_function_host(c.ctx.handle, _pp(c), q.ctypes.data_as(dp), f_h.ctypes.data_as(dp), B), "ccmp_function_host")
        check(L.ccmp_is_satisfied_host(c.ctx.handle, _pp(c), q.ctypes.data_as(dp), s_h.ctypes.data_as(u8p), B), "ccmp_is_satisfied_host")
        check(L.ccmp_joint_valid_host(c.ctx.handle, _pp(c), q.ctypes.data_as(dp), j_h.ctypes.data_as(u8p), B), "ccmp_joint_valid_host")
        assert f_h[-1:].view(np.int64)[0] == SENT_BITS and s_h[-1] == SENT_BYTE and j_h[-1] == SENT_BYTE
        q_d = _dev(q)
        f_d = _function(c, q_d, B).cpu().numpy()[:B]
        s_d = _flags_call("ccmp_is_satisfied_batch", c, q_d, B).cpu().numpy()[:B]
        j_d = _flags_call("ccmp_joint_valid_batch", c, q_d, B).cpu().numpy()[:B]
        assert sk.same_bits(f_h[:-1].reshape(B, 2), f_d).all()
        assert np.array_equal(s_h[:-1], s_d) and np.array_equal(j_h[:-1], j_d)
        # and all three are the oracle's
        assert sk.same_bits(f_d, np.array([oracle_det.function(P, r) for r in q])).all()
        assert np.array_equal(s_d, np.array([oracle_det.is_satisfied(P, r) for r in q], dtype=np.uint8))
        assert np.array_equal(j_d, np.array([oracle_det.joint_valid(P, r) for r in q], dtype=np.uint8))
    if B > 1:
        assert 0 < s_d.sum() < B and 0 < j_d.sum() < B
