"""The extend step in analytic mode (jacobian_mode = CCMP_JAC_ANALYTIC) through every public entry point: the host ABI, the
device ABI without Newton counts, the round budget, the C++ adapter and stream capture.  The traversal is one launch of
geodesic_row16_kernel (ccmp_kernels_fast.hip); everything is compared bit for bit with the oracle's analytic mode."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from arm_model_cases import edges as _edges, tilt as _tilt  # (one text: tests/arm_model_cases.py)
from conftest import NCPU, ROOT, config_path
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu

dp = C.POINTER(C.c_double)


def _analytic(gpu_ctx, oracle_det, variant=None):
    c = _constraint("Wine_Bottle", gpu_ctx, mode=1)
    if variant == "tilted":
        _tilt(c)
    P = _oracle_problem(oracle_det, c)
    assert P.jacobian_mode == 1
    return c, P


def _host_call(fn, c, gpu_ctx, f, t, ms, *extra):
    E = f.shape[0]
    st = np.full((E, ms, 14), 7.0)
    n = np.zeros(E, dtype=np.int32)
    ok = np.full(E, 9, dtype=np.uint8)
    rc = fn(gpu_ctx.handle, C.byref(c.problem), f.ctypes.data_as(dp), t.ctypes.data_as(dp), E, ms, st.ctypes.data_as(dp),
            n.ctypes.data_as(C.POINTER(C.c_int32)), ok.ctypes.data_as(C.POINTER(C.c_uint8)), *extra)
    assert rc == 0, rc
    return st, n, ok


def _same_lists(st, n, so, no, ms):
    live = np.arange(ms)[None, :] < np.minimum(n, ms)[:, None]
    return np.array_equal(n, no) and np.array_equal(st[live].view(np.uint64), so[live].view(np.uint64))


@pytest.mark.parametrize("E,variant", [(1, None), (5, None), (700, None), (5, "tilted")])
def test_host_entry_points_in_analytic_mode(gpu_ctx, oracle_det, E, variant):
    """ccmp_geodesic_host, ccmp_check_motion_host and ccmp_geodesic_host_ex (the adapter's only way to the extend step) in analytic
    mode: lists, counts and flags equal orc_discrete_geodesic_batch; an edge whose target is off the manifold reports n = 1, ok = 0
    under checkMotion"""
    from closed_chain_motion_planner_amd import _lib

    L = _lib.lib()
    c, P = _analytic(gpu_ctx, oracle_det, variant)
    frm, to = _edges(c, E, 0x8A0 + E)
    f = np.ascontiguousarray(frm.cpu().numpy())
    t = np.ascontiguousarray(to.cpu().numpy())
    t[E - 1] += 0.4  # off the manifold
    ms = 8
    so, no, oko, _ = oracle_det.discrete_geodesic_batch(P, f, t, ms, NCPU)
    st, n, ok = _host_call(L.ccmp_geodesic_host, c, gpu_ctx, f, t, ms)
    assert _same_lists(st, n, so, no, ms) and np.array_equal(ok, oko)
    carry = np.zeros((E, 2))
    st2, n2, ok2 = _host_call(L.ccmp_geodesic_host_ex, c, gpu_ctx, f, t, ms, None, carry.ctypes.data_as(dp), 0, 0)
    assert _same_lists(st2, n2, so, no, ms) and np.array_equal(ok2, oko)
    sat = np.array([oracle_det.is_satisfied(P, t[e]) for e in range(E)], dtype=bool)
    assert not sat[E - 1]
    stc, nc, okc = _host_call(L.ccmp_check_motion_host, c, gpu_ctx, f, t, ms)
    assert nc[E - 1] == 1 and okc[E - 1] == 0
    assert (nc[~sat] == 1).all() and (okc[~sat] == 0).all()
    assert np.array_equal(nc[sat], no[sat]) and np.array_equal(okc[sat], oko[sat])
    assert _same_lists(stc[sat], nc[sat], so[sat], no[sat], ms)
    stx, nx, okx = _host_call(L.ccmp_geodesic_host_ex, c, gpu_ctx, f, t, ms, None, None, 0, 1)
    assert np.array_equal(nx, nc) and np.array_equal(okx, okc) and _same_lists(stx, nx, stc, nc, ms)


def test_device_call_without_newton_counts(gpu_ctx, oracle_det):
    """ccmp_geodesic_batch_ex with newton_iters = NULL in analytic mode: the same lists, counts, flags and carries as the same
    call with the counts (plain, with check_target, with a round budget)"""
    import torch
    from closed_chain_motion_planner_amd import _lib
    from closed_chain_motion_planner_amd.constraint import _stream_handle

    c, _ = _analytic(gpu_ctx, oracle_det)
    E, ms = 700, 8
    frm, to = _edges(c, E, 0x8B0)
    to[3] = to[3] + 0.4
    for chk, budget in ((0, 0), (1, 0), (0, 12)):
        ref = c.discrete_geodesic_batch(frm, to, ms, check_target=bool(chk), want_carry=True, round_budget=budget)
        st = torch.full((E, ms, 14), 7.0, dtype=torch.float64, device=frm.device)
        n = torch.zeros(E, dtype=torch.int32, device=frm.device)
        ok = torch.full((E,), 9, dtype=torch.uint8, device=frm.device)
        carry = torch.zeros((E, 2), dtype=torch.float64, device=frm.device)
        rc = _lib.lib().ccmp_geodesic_batch_ex(gpu_ctx.handle, C.byref(c.problem), frm.data_ptr(), to.data_ptr(), E, ms, st.data_ptr(), n.data_ptr(),
                                               ok.data_ptr(), None, None, carry.data_ptr(), budget, chk, _stream_handle(None))
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert torch.equal(n, ref[1]) and torch.equal(ok, ref[2]), (chk, budget)
        assert torch.equal(carry.view(torch.int64), ref[4].view(torch.int64)), (chk, budget)
        live = torch.arange(ms, device=frm.device)[None, :] < n.clamp(max=ms)[:, None]
        assert torch.equal(st[live].view(torch.int64), ref[0][live].view(torch.int64)), (chk, budget)
        if budget:
            assert int((ok == 2).sum()) > 0


@pytest.mark.parametrize("E", [700, 3000, 20000])
def test_round_budget_in_analytic_mode(gpu_ctx, oracle_det, E):
    """round_budget = 12 with lists of 8: some edges stop between two states with ok = 2; first pass + continue_geodesics gives
    every edge the oracle's uninterrupted traversal (states, flag, Newton total); the edges that ended in the first pass equal
    the oracle's bounded call; and a suspended edge stopped at the first accepted state at which its rounds reached the budget"""
    c, P = _analytic(gpu_ctx, oracle_det)
    ms, budget = 8, 12
    frm, to = _edges(c, E, 0x8C0)
    st, n, ok, its, carry = c.discrete_geodesic_batch(frm, to, ms, want_carry=True, round_budget=budget)
    whole = c.continue_geodesics(to, st, n, ok, its, carry, ms, round_budget=budget)
    f_h, t_h = frm.cpu().numpy(), to.cpu().numpy()
    st_h, n_h, ok_h, it_h = st.cpu().numpy(), n.cpu().numpy(), ok.cpu().numpy(), its.cpu().numpy()
    sus = np.nonzero(ok_h == 2)[0]
    assert len(sus) > 0 and set(ok_h.tolist()) <= {0, 1, 2}
    # edges that ended in the first pass (arrived, gave up, list full): the oracle's call with the same list length
    so, no, oko, ito = oracle_det.discrete_geodesic_batch(P, f_h, t_h, ms, NCPU)
    done = ok_h != 2
    assert np.array_equal(n_h[done], no[done]) and np.array_equal(ok_h[done], oko[done]) and np.array_equal(it_h[done], ito[done])
    assert _same_lists(st_h[done], n_h[done], so[done], no[done], ms)
    assert (oko[sus] != 2).all()
    # first pass + continuation: the oracle's uninterrupted traversal
    assert set(whole) == set(np.nonzero((ok_h == 2) | (n_h == ms + 1))[0].tolist())
    rng = np.random.default_rng(E)
    keys = sorted(whole)
    for e in rng.choice(keys, size=min(150, len(keys)), replace=False).tolist() + [int(k) for k in sus[:20]]:
        st_e, ok_e, its_e = whole[e]
        okf, stf, itf = oracle_det.discrete_geodesic(P, f_h[e], t_h[e], interpolate=True, max_states=4096)
        assert stf.shape == st_e.shape and np.array_equal(np.ascontiguousarray(st_e).view(np.uint64), stf.view(np.uint64)), e
        assert bool(ok_e) == okf and its_e == itf, e
    # the suspension point: rounds = Newton updates + one per projection, counted through the accepted states
    for e in sus[:40].tolist():
        k = int(n_h[e])  # `from` + k - 1 accepted states
        assert k >= 2 and int(it_h[e]) + (k - 1) >= budget, e
        _, _, n_o, its_o, _ = oracle_det.discrete_geodesic_ex(P, f_h[e], t_h[e], k - 1)
        assert n_o == k  # the (k-1)-th accepted state found the list full: its updates are taken back
        assert its_o + (k - 2) < budget, e


def test_adapter_in_analytic_mode(ccmp_built, oracle_det, gpu_ctx, tmp_path):
    """the C++ adapter after setJacobianMode(1): ccmp::discreteGeodesicBatch over growTree's handful of edges and over 1 500
    edges (the budgeted first pass with lists of 16, then continuations) — reached flags and whole lists equal the oracle's"""
    c, P = _analytic(gpu_ctx, oracle_det)
    libdir = os.path.dirname(ccmp_built)
    exe = str(tmp_path / "adapter_analytic_check")
    subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-pthread", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "adapter_analytic_check.cpp"), "-L", libdir, "-lccmp", "-Wl,-rpath," + libdir,
                    "-Wl,-rpath,/opt/rocm/lib", "-o", exe], check=True)
    for E in (5, 1500):
        frm, to = _edges(c, E, 0x8D0 + E)
        f_h, t_h = frm.cpu().numpy(), to.cpu().numpy()
        path = tmp_path / ("edges%d.txt" % E)
        np.savetxt(path, np.concatenate([f_h, t_h]), fmt="%.17g")
        out = subprocess.run([exe, config_path("Wine_Bottle"), str(path), "64"], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        assert lines[0] == "error 0"
        i, reached = 1, []
        for e in range(E):
            head = lines[i].split()
            assert head[:2] == ["edge", str(e)]
            m = int(head[5])
            rows = np.array([[int(h, 16) for h in lines[i + 1 + k].split()] for k in range(m)], dtype=np.uint64).reshape(m, 14)
            i += 1 + m
            okf, stf, _ = oracle_det.discrete_geodesic(P, f_h[e], t_h[e], interpolate=True, max_states=4096)
            assert np.array_equal(rows, stf.view(np.uint64)) and int(head[3]) == int(okf), e
            reached.append(okf)
        assert any(reached)


def test_stream_capture_in_analytic_mode(gpu_ctx, oracle_det):
    """one analytic discrete_geodesic_batch with a round budget and carries, captured in a torch.cuda.graph on one stream and
    replayed twice: bitwise the eager call (first pass and its continuation through carry_in)"""
    import torch

    c, _ = _analytic(gpu_ctx, oracle_det)
    E, ms, budget = 3000, 8, 12
    frm, to = _edges(c, E, 0x8E0)
    eager = c.discrete_geodesic_batch(frm, to, ms, want_carry=True, round_budget=budget)
    torch.cuda.synchronize()
    # the continuation's inputs: every edge from its last stored state with its carry (edges that ended simply start again at it)
    last = eager[0][torch.arange(E, device=frm.device), (eager[1].clamp(max=ms) - 1).long()].contiguous()
    cin = eager[4].clone()
    eager2 = c.discrete_geodesic_batch(last, to, ms, carry_in=cin, want_carry=True, round_budget=budget)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        c.discrete_geodesic_batch(frm, to, ms, want_carry=True, round_budget=budget)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap1 = c.discrete_geodesic_batch(frm, to, ms, want_carry=True, round_budget=budget)
        cap2 = c.discrete_geodesic_batch(last, to, ms, carry_in=cin, want_carry=True, round_budget=budget)
    for _ in range(2):
        for got in (cap1, cap2):
            for x in got:
                x.fill_(0)
        g.replay()
        torch.cuda.synchronize()
        for got, ref in ((cap1, eager), (cap2, eager2)):
            live = torch.arange(ms, device=frm.device)[None, :] < ref[1].clamp(max=ms)[:, None]
            assert torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
            assert torch.equal(got[4].view(torch.int64), ref[4].view(torch.int64))
            assert torch.equal(got[0][live].view(torch.int64), ref[0][live].view(torch.int64))
    assert int((eager[2] == 2).sum()) > 0
