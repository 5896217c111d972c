"""The range facts of an in-range Newton round in the STOCK throughput kernels (ccmp_kernels_fd.hip: jacobian_columns<., true, X0 = true>
with ccmp_sincos_inr and quat_of_t<true>: no range test in the stencil's sines and cosines, the quaternion's root and quotient
without their guards, its case once per wavefront), end to end and bit for bit — rows, flags, iteration counts — against the det
oracle, on a context forced onto the throughput kernel at every size.

Sizes 1, 10, 11, 61 and 4 099 are prefixes of ONE batch per fixture (one oracle run), built wavefront by wavefront (ten samples):
near-manifold states (every lane in the fixture's case: the case bodies run), uniform samples (mixed cases: the branch-free text),
both kinds side by side, and wavefronts in which one sample holds a joint within 1e-9 of 2 pi, or one beyond +-512, or one so far
out that its sines are NaN from the first round on (each sends ITS wavefront's rounds through the old text while its neighbours
stay live).  Forms: one launch, head plus resume with a head of 1 and of 5 rounds, the fused sampler, and a bulk extend call of
16 384 + 1 edges on geodesic_group_kernel<true>.  Fixtures: Wine_Bottle (case 1), stefan and dumbbell (case 2), and Wine_Bottle with
two synthetic initial poses whose relative rotation has a positive trace (case 3) and a largest first diagonal entry (case 0).
One calibrated-arm batch runs the general instantiations, whose text and resource records the change leaves alone."""
import ctypes as C
import math

import numpy as np
import pytest

from conftest import NCPU
from test_gpu_parity import _constraint, _oracle_problem

pytestmark = pytest.mark.gpu
SIZES = [1, 10, 11, 61, 4099]
NMAX = max(SIZES)
FIXTURES = ["Wine_Bottle", "stefan", "dumbbell", "case3", "case0"]
FORMS = {"one_launch": 0, "head_1": 1, "head_5": 5}
CASE = {"Wine_Bottle": 1, "stefan": 2, "dumbbell": 2, "case3": 3, "case0": 0}  # Eigen's branch for the fixture's init_chain_
_CACHE = {}


@pytest.fixture(scope="module")
def tk_ctx(ccmp_built):
    """the throughput kernel alone at every size, scout order and the head launch from one sample on"""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from closed_chain_motion_planner_amd import Context

    ctx = Context(0)
    ctx.set_schedule(0, 0)
    ctx.set_lpt(1, 0)
    ctx.set_option("fd_head_min_batch", 0)
    return ctx


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def _problem(name, ctx):
    if name in ("Wine_Bottle", "stefan", "dumbbell"):
        return _constraint(name, ctx)
    c = _constraint("Wine_Bottle", ctx)
    # a synthetic init_chain_: a rotation whose quaternion falls into a case no shipped fixture has
    R = _rot((0.2, 0.3, 1.0), 0.4) if name == "case3" else _rot((1.0, 0.05, -0.08), math.pi - 0.03)
    tr, d = np.trace(R), np.diag(R)
    assert (tr > 0.5) if name == "case3" else (tr < -0.9 and d[0] > d[1] + 0.5 and d[0] > d[2] + 0.5)
    for k in range(9):
        c.problem.init_R[k] = float(R.reshape(-1)[k])
    return c


def _batch(oracle, c, name):
    """(q, oracle's rows, flags, iterations) of the fixture's one batch of NMAX samples"""
    if name in _CACHE:
        return _CACHE[name]
    P = _oracle_problem(oracle, c)
    far = oracle.ambient_uniform_batch(P, 0xFAC7, 0, 3 * NMAX)
    proj, ok, _ = oracle.project_batch(P, far, NCPU)
    on = proj[ok != 0]
    rng = np.random.default_rng(0xFAC8)
    assert len(on) >= 1000, (name, len(on))  # every fixture, the synthetic poses included, is reached by plenty of uniform samples
    pick = rng.integers(0, len(on), NMAX)
    near = on[pick] + rng.normal(0.0, 1e-3, (NMAX, 14))
    # the quaternion's case of the near-manifold states' relative rotation R2^T R1, on the host (every 16th of them): the fixture's
    # own, so that the wavefronts of near-manifold states agree on it and enter that case's body
    cases = set()
    for x in near[::16]:
        m = oracle.fk(P, 1, x[7:])[0].T @ oracle.fk(P, 0, x[:7])[0]
        cases.add(3 if np.trace(m) > 0.0 else int(np.argmax(np.diag(m))))
    assert cases == {CASE[name]}, (name, cases)
    q = np.empty((NMAX, 14))
    for w in range(0, NMAX, 10):  # wavefront by wavefront
        kind, sl = (w // 10) % 8, slice(w, min(w + 10, NMAX))
        if kind in (0, 1, 4):
            q[sl] = near[sl]
        elif kind in (2, 5):
            q[sl] = far[sl]
        else:
            q[sl] = near[sl]
            q[w:min(w + 10, NMAX):2] = far[w:min(w + 10, NMAX):2]
        row, j = min(w + 3, NMAX - 1), (w // 10) % 14
        if kind == 4:
            q[row, j] = 2 * math.pi - 5e-10 if (w // 80) % 2 else -2 * math.pi + 3e-10  # within 1e-9 of a multiple of 2 pi
        elif kind == 5:
            q[row, j] = 600.0 if (w // 80) % 2 else -513.0  # beyond +-512
        elif kind == 6:
            q[row, j] = 1e7 if (w // 80) % 2 else 1.6e6  # sines and cosines NaN at once / as soon as a step crosses 2^20 pi / 2
    q[0] = near[0]
    q = np.ascontiguousarray(q)
    _CACHE[name] = (q,) + tuple(oracle.project_batch(P, q, NCPU))
    return _CACHE[name]


def _same(got, ref, what):
    q, ok, it = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy().astype(np.int32)
    assert np.array_equal(ok, ref[1]), (what, "flags", np.argwhere(ok != ref[1])[:4])
    assert np.array_equal(it, ref[2]), (what, "iterations", np.argwhere(it != ref[2])[:4])
    same = (q.view(np.uint64) == ref[0].view(np.uint64)) | (np.isnan(q) & np.isnan(ref[0]))
    assert same.all(), (what, "rows", np.argwhere(~same)[:4])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", FIXTURES)
def test_projection_bitwise_at_every_size(tk_ctx, oracle_det, name, form):
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _problem(name, tk_ctx)
    q, q_cpu, ok_cpu, it_cpu = _batch(oracle_det, c, name)
    assert 1000 < int(ok_cpu.sum()) < NMAX and it_cpu.min() < 20 < it_cpu.max(), name  # both outcomes, short and long runs
    tk_ctx.set_option("fd_head_rounds", FORMS[form])
    try:
        assert ("(head)" in tk_ctx.describe(_lib.CALL_PROJECT, 1)) == (FORMS[form] > 0)
        for n in SIZES:
            got = c.project_batch(torch.as_tensor(q[:n]).cuda())
            torch.cuda.synchronize()
            _same(got, (q_cpu[:n], ok_cpu[:n], it_cpu[:n]), (name, form, n))
    finally:
        tk_ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))


@pytest.mark.parametrize("form", ["one_launch", "head_5"])
@pytest.mark.parametrize("name", ["Wine_Bottle", "stefan"])
def test_fused_sampler_bitwise(tk_ctx, oracle_det, name, form):
    from closed_chain_motion_planner_amd import _lib

    c = _problem(name, tk_ctx)
    P = _oracle_problem(oracle_det, c)
    key = ("sampler", name)
    if key not in _CACHE:
        _CACHE[key] = oracle_det.sample_project_batch(P, 0xFAC9, 7, NMAX, NCPU)[:3]
    ref = _CACHE[key]
    tk_ctx.set_option("fd_head_rounds", FORMS[form])
    try:
        for n in (11, NMAX):
            got = c.sample_project_batch(0xFAC9, 7, n)
            _same(got[:3], tuple(a[:n] for a in ref), (name, form, n, "sampler"))
    finally:
        tk_ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))


def test_calibrated_arms_are_left_alone(tk_ctx, oracle_det):
    """the general instantiations: the oracle's bits, and the resource records of the build (no scratch instruction; the stock
    kernels none at all) as closed_chain_motion_planner_amd/build.py checks them"""
    import torch
    from closed_chain_motion_planner_amd import _lib, build

    c = _constraint("Wine_Bottle", tk_ctx)
    for arm in (0, 1):
        dh = (C.c_double * 28)(*[1e-3 * ((3 * i + 5 * arm) % 7 - 3) for i in range(28)])
        assert _lib.lib().ccmp_set_calibration(C.byref(c.problem), arm, dh) == 0
    P = _oracle_problem(oracle_det, c)
    q = oracle_det.ambient_uniform_batch(P, 0xFACA, 0, 641)
    ref = oracle_det.project_batch(P, q, NCPU)
    for rounds in (0, 5):
        tk_ctx.set_option("fd_head_rounds", rounds)
        try:
            _same(c.project_batch(torch.as_tensor(q).cuda()), ref, ("calibrated", rounds))
        finally:
            tk_ctx.set_option("fd_head_rounds", _lib.get_option(None, "fd_head_rounds"))
    # the general instantiations' resource records as the build left them: the figures of the commit before this change (VGPRs,
    # private segment, SGPR spills: the same compiler gives the same text the same allocation), and the stock kernels' budget
    rep = {k["name"]: k for k in build.resource_report()["ccmp_kernels_fd.hip"]}
    general = {"project_fd_kernel<0, false>": (137, 132, 96), "project_fd_kernel<2, false>": (135, 132, 45),
               "project_fd_kernel<4, false>": (138, 132, 112), "geodesic_group_kernel<false>": (138, 132, 147)}
    for name, want in general.items():
        k = rep[name]
        assert (k["vgprs"], k["scratch"], k["sgpr_spill"]) == want and k["vgpr_spill"] == 0, k
    stock = [n for n in rep if n.startswith(("project_fd_kernel<", "geodesic_group_kernel<")) and n.endswith("true>")]
    assert len(stock) == 7
    for name in stock:
        k = rep[name]
        assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and k["vgprs"] <= 168, k


def test_bulk_extend_on_the_throughput_layout_bitwise(gpu_ctx, oracle_det):
    """16 384 + 1 edges forced onto geodesic_group_kernel<true>: equal to the latency kernel's result everywhere, to the oracle's on
    a slice"""
    import torch
    from closed_chain_motion_planner_amd import _lib

    c = _constraint("Wine_Bottle", gpu_ctx)
    P = _oracle_problem(oracle_det, c)
    E = 16384 + 1
    q, ok, _, _ = c.sample_project_batch(0xFACB, 0, 8 * E, want_iters=False)
    frm = q[ok == 1][:E].contiguous()
    assert frm.shape[0] == E
    to, _, _, _ = c.sample_near_project_batch(0xFACC, 0, frm, 0.6, E, want_iters=False)
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
    assert int((got[1] > 1).sum()) > E // 2
    st, n, okf, its, _ = got
    checked = 0
    for e in list(range(0, 60)) + [E - 1]:
        if int(okf[e]) == 2:
            continue  # suspended by the round budget: the oracle's count is of the whole traversal
        ok_e, st_e, n_e, its_e, _ = oracle_det.discrete_geodesic_ex(P, frm[e].cpu().numpy(), to[e].cpu().numpy(), cap)
        assert int(n[e]) == n_e and bool(okf[e]) == bool(ok_e) and int(its[e]) == its_e, e
        assert np.array_equal(st[e, : min(n_e, cap)].cpu().numpy().view(np.uint64), st_e.view(np.uint64)), e
        checked += 1
    assert checked > 15
