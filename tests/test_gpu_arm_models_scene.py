"""The proxy clearance and the extend step with a scene on every arm model the launchers switch on (tests/arm_model_cases.py: stock,
general_kernels, tilted, calibrated, calibrated_tilted), bit for bit against the det oracle: uint64 views, NaN equal to NaN, no
tolerance.  The stock suites (test_gpu_scene.py, test_gpu_scene_shapes.py, test_gpu_geodesic_scene.py) run _constraint("Wine_Bottle" |
"stefan") only; a stock shortcut taken on a calibrated problem, a dropped base_R product or a scene launcher that ignores K.stock
changes numbers on the other models alone.  Sizes are the smallest at which that code can go wrong (arm_model_cases.B_CLEAR, E_SCENE);
the seeds are chosen in tests/test_arm_model_cases.py, on the oracle alone.

What ran on no model but stock before, and the test that runs it now (planner: tests/test_gpu_arm_models_planner.py):

  geodesic_scene_kernel<false> (FD; also FD with twin_arms = 0)        test_extend_with_a_scene[0-general_kernels / tilted / calibrated /
                                                                       calibrated_tilted], test_scene_continuation_on_calibrated_arms[0]
  state_clearance<128> / <16>, clearance_kernel<4> / <10>,             test_clearance_against_the_oracle (both kernels, default and random
  clearance_state_kernel with calibrated K.axis / K.aprod /            scene, a non-diagonal K.base_R through clearance_batch),
  K.offset / K.ee / K.R_tool and with a non-diagonal K.base_R          test_clearance_general_kernels_equal_stock, test_extend_with_a_scene
  skeleton_spheres(problem) / ProxyValidityChecker(c) of a             test_clearance_against_the_oracle[default-calibrated*] (the scene
  calibrated problem                                                   differs from the stock one: test_arm_model_cases.py), and every
                                                                       scene test here and in the planner module
  geodesic_row16_scene_kernel<DIAG> on calibrated constants            test_extend_with_a_scene[1-calibrated / calibrated_tilted],
                                                                       test_scene_continuation_on_calibrated_arms[1]
  connect_batch(scene=), Roadmap.connect / grow, densify_paths,        planner: test_connect_equals_its_parts_and_the_oracle,
  shortcut_paths on a non-stock model                                  test_grow_and_the_store, test_densify_and_shortcut
  analytic extend step (geodesic_row16_kernel) on calibrated arms      planner: test_plain_analytic_extend_on_calibrated_arms
  smooth_paths on a non-stock model: the pass loop's own option        planner: test_smooth (tilted and calibrated, both modes, with and
  struct handed to densify, the projector, the pair tests and          without a scene; the seeds: arm_model_cases.SMOOTH_SEED)
  clearance_batch

Mutation check: changes of arithmetic only (no barrier, loop bound or index depends on them) on scratch builds, one run of this module
and of tests/test_gpu_arm_models_planner.py each; all gave wrong answers, none a fault or a hang.  What failed here (the planner
module's share is in its own docstring):
  ccmp_kernels_geo_scene.hip: the launcher always takes            test_extend_with_a_scene[0-calibrated], [0-calibrated_tilted],
  CCMP_LAUNCH_GEO_SCENE(true)                                      test_scene_continuation_on_calibrated_arms[0]  ([0-general_kernels] passes:
                                                                   on the stock problem the stock kernel is right)
  ccmp_kernels_fast.hip: CCMP_LAUNCH_GEO_ROW16_SCENE always        test_extend_with_a_scene[1-tilted], [1-calibrated_tilted]
  takes DIAG = true
  ccmp_clearance.h: the world transform takes K.base_R[0]          test_extend_with_a_scene[0-tilted], [0-calibrated_tilted], [1-tilted],
  for both arms                                                    [1-calibrated_tilted]  (test_clearance_against_the_oracle passes: the kernels
                                                                   of clearance_batch carry their own transform, next line)
  ccmp_kernels_scene.hip: likewise in clearance_kernel and         test_clearance_against_the_oracle[tilted-*] (4), [calibrated_tilted-*] (4),
  clearance_state_kernel                                           test_extend_with_a_scene[*-tilted] (2), [*-calibrated_tilted] (2): their margin
                                                                   comes from clearance_batch"""
import numpy as np
import pytest

import arm_model_cases as A
from test_gpu_geodesic_scene import OracleScene, _bits, _check_against_oracle, _pick_margin, _random_scene
from test_gpu_parity import _constraint, _oracle_problem
from test_gpu_scene import _bits_equal, _states

pytestmark = pytest.mark.gpu

NON_STOCK = ("tilted", "calibrated", "calibrated_tilted")
PER_STATE_MAX = {"tiles": 0, "per_state": 1 << 30}


def _scene(c, kind):
    from closed_chain_motion_planner_amd import scene as S

    return S.ProxyValidityChecker(c).scene if kind == "default" else _random_scene(c)


def _clearance(gpu_ctx, sc, q, margin, kernel):
    import torch

    gpu_ctx.set_option("clearance_per_state_max", PER_STATE_MAX[kernel])
    try:
        out = sc.clearance_batch(torch.as_tensor(q).cuda(), margin=margin)
        torch.cuda.synchronize()
    finally:
        gpu_ctx.set_option("clearance_per_state_max", 8192)
    return [x.cpu().numpy() for x in out]


@pytest.mark.parametrize("kernel", sorted(PER_STATE_MAX))
@pytest.mark.parametrize("kind", ["default", "random"])
@pytest.mark.parametrize("model", NON_STOCK)
def test_clearance_against_the_oracle(gpu_ctx, oracle_det, model, kind, kernel):
    """clearance_batch through the tile kernel and the per-state kernel, on the scene built AFTER the model is applied (the skeleton
    follows problem.offset) and on the random 64-sphere / 8-box scene: distance, pair code and free equal the oracle's"""
    c = _constraint(A.OBJ, gpu_ctx)
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        sc = _scene(c, kind)
        q = _states(oracle_det, P, A.B_CLEAR, A.CLEAR_SEED)
        clr_o, pair_o = oracle_det.clearance_batch(P, sc.spheres, sc.boxes, sc.allowed, q)
        margin = A.clear_margin(kind, clr_o)
        clr, pair, free = _clearance(gpu_ctx, sc, q, margin, kernel)
    print("%s %s %s: %d of %d free at margin %.4f" % (model, kind, kernel, int((clr_o > margin).sum()), A.B_CLEAR, margin))
    assert _bits_equal(clr, clr_o).all(), np.flatnonzero(~_bits_equal(clr, clr_o))[:8]
    assert np.array_equal(pair, pair_o)
    assert np.array_equal(free, (clr_o > margin).astype(np.uint8)) and 0 < int(free.sum()) < A.B_CLEAR
    if kind == "default":
        assert sc.spheres == A.default_scene_host(c.problem).spheres  # the host restatement the CPU test chose the seed on


@pytest.mark.parametrize("kind", ["default", "random"])
def test_clearance_general_kernels_equal_stock(gpu_ctx, oracle_det, kind):
    """option stock_kernels = 0 on the stock problem: the same bytes from both clearance kernels (no oracle needed)"""
    c = _constraint(A.OBJ, gpu_ctx)
    sc = _scene(c, kind)
    q = _states(oracle_det, _oracle_problem(oracle_det, c), A.B_CLEAR, A.CLEAR_SEED)
    for kernel in sorted(PER_STATE_MAX):
        stock = _clearance(gpu_ctx, sc, q, -0.03, kernel)
        with A.apply(c, gpu_ctx, "general_kernels"):
            assert gpu_ctx.get_option("stock_kernels") == 0
            general = _clearance(gpu_ctx, sc, q, -0.03, kernel)
        assert gpu_ctx.get_option("stock_kernels") == 1
        for a, b in zip(stock, general):
            assert a.tobytes() == b.tobytes(), (kind, kernel)


def _edges_checked(c, oracle, P, E, seed):
    """arm_model_cases.edges on the device; the oracle's restatement gives the same rows (the seeds were chosen on those)"""
    frm, to = A.edges(c, E, seed)
    f_o, t_o = A.oracle_edges(oracle, P, E, seed)
    assert np.array_equal(_bits(frm.cpu().numpy()), _bits(f_o)) and np.array_equal(_bits(to.cpu().numpy()), _bits(t_o))
    return frm, to


@pytest.mark.parametrize("model", A.MODELS)
@pytest.mark.parametrize("mode", [0, 1])
def test_extend_with_a_scene(gpu_ctx, oracle_det, mode, model):
    """discrete_geodesic_scene_batch(want_clearance, want_carry) on 32 edges with lists of 16 against the oracle's traversal behind the
    validity callback: states, counts, flags, Newton counts, blocked, clearances and carries; margin from _pick_margin (blocked share
    within 0.2 .. 0.8, an edge blocked at its first state).  general_kernels: also byte for byte the stock kernels' result"""
    from closed_chain_motion_planner_amd import scene as S

    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    E, ms, seed = A.E_SCENE, A.MS_SCENE, A.EXTEND_SEED[(model, mode)]
    stock = None
    if model == "general_kernels":
        sc = S.ProxyValidityChecker(c).scene
        frm, to = A.edges(c, E, seed)
        margin, _, _ = _pick_margin(c, sc, frm, to, ms)
        stock = [x.cpu().numpy() for x in c.discrete_geodesic_scene_batch(frm, to, sc, margin, ms, want_clearance=True, want_carry=True)]
    with A.apply(c, gpu_ctx, model):
        P = _oracle_problem(oracle_det, c)
        assert P.jacobian_mode == mode
        sc = S.ProxyValidityChecker(c).scene
        frm, to = _edges_checked(c, oracle_det, P, E, seed)
        margin, _, _ = _pick_margin(c, sc, frm, to, ms)
        assert margin == A.oracle_pick_margin(oracle_det, P, A.default_scene_host(c.problem), frm.cpu().numpy(), to.cpu().numpy(), ms)
        bl = _check_against_oracle(c, P, oracle_det, sc, margin, frm, to, ms)
        if stock is not None:
            general = [x.cpu().numpy() for x in c.discrete_geodesic_scene_batch(frm, to, sc, margin, ms, want_clearance=True, want_carry=True)]
            live = np.arange(ms)[None, :] < np.minimum(stock[1], ms)[:, None]
            for k in (1, 2, 3, 4, 5, 6):  # (clearance: NaN where unwritten, from the same fill)
                assert stock[k].tobytes() == general[k].tobytes(), k
            assert stock[0][live].tobytes() == general[0][live].tobytes()
    print("%s mode %d: margin %.6f blocks %d of %d edges" % (model, mode, margin, int(bl.sum()), E))


@pytest.mark.parametrize("mode", [0, 1])
def test_scene_continuation_on_calibrated_arms(gpu_ctx, oracle_det, mode):
    """round_budget = 6, then continue_geodesics with the same scene and margin: every edge's whole list, flag, Newton total and blocked
    equal the oracle's ONE uninterrupted traversal (the continuation loop hands carry and budget to the general kernels)"""
    from closed_chain_motion_planner_amd import scene as S

    c = _constraint(A.OBJ, gpu_ctx, mode=mode)
    E, ms, budget = A.E_SCENE, A.MS_SCENE, 6
    with A.apply(c, gpu_ctx, "calibrated"):
        P = _oracle_problem(oracle_det, c)
        sc = S.ProxyValidityChecker(c).scene
        frm, to = A.edges(c, E, A.EXTEND_SEED[("calibrated", mode)])
        margin, _, _ = _pick_margin(c, sc, frm, to, ms)
        st, n, ok, its, bl, carry = c.discrete_geodesic_scene_batch(frm, to, sc, margin, ms, want_carry=True, round_budget=budget)
        cont = c.continue_geodesics(to, st, n, ok, its, carry, ms, round_budget=budget, scene=sc, margin=margin)
    st_h, n_h, ok_h, its_h, bl_h = [x.cpu().numpy() for x in (st, n, ok, its, bl)]
    assert int((ok_h == 2).sum()) > 0 and set(cont) == set(np.flatnonzero((ok_h == 2) | (n_h > ms)).tolist())
    orc = OracleScene(oracle_det, P, sc, margin)
    f, t = frm.cpu().numpy(), to.cpu().numpy()
    for e in range(E):
        if e in cont:
            s_e, ok_e, its_e, bl_e = cont[e]
        else:
            s_e, ok_e, its_e, bl_e = st_h[e, :n_h[e]], ok_h[e], its_h[e], bl_h[e]
        ok_o, st_o, n_o, its_o, _, bl_o, _ = orc.edge(f[e], t[e], 4096)
        assert (len(s_e), ok_e, its_e, bl_e) == (n_o, ok_o, its_o, bl_o), e
        assert np.array_equal(_bits(s_e), _bits(st_o)), e
    print("mode %d: %d of %d edges suspended at %d rounds, %d continued" % (mode, int((ok_h == 2).sum()), E, budget, len(cont)))
