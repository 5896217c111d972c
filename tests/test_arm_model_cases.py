"""tests/arm_model_cases.py checked with the oracle alone (no device): the models are what they claim to be, and the seeds chosen there
give every test of tests/test_gpu_arm_models_scene.py and tests/test_gpu_arm_models_planner.py the cases it is about — so that no GPU
run is spent finding one.  The measured values behind each condition are printed (pytest -s)."""
import numpy as np
import pytest

import arm_model_cases as A
from conftest import NCPU, load_cfg
from dense_path_cases import oracle_segments
from shortcut_cases import oracle_pairs, pairs_py
from smooth_cases import BELOW, PROJECTED, REFUSED, Restatement, mirror_fill, same_f64, scene_restatement
from smooth_cases import expect as smooth_expect
from test_gpu_geodesic_scene import OracleScene, _random_proxies
from test_gpu_parity import _oracle_problem
from test_gpu_scene import _states

MODES = (0, 1)


def _model(oracle, model, mode=0):
    c = A.host_constraint(mode)
    with A.apply(c, None, model):
        pass
    return c, _oracle_problem(oracle, c)


@pytest.mark.parametrize("model", A.MODELS)
def test_problem_hand_over(oracle_det, model):
    """stock (and general_kernels, the same problem) goes to the checker as the oracle's OWN set-up of the fixture; every other model
    differs from it and is handed over as bytes"""
    c, P = _model(oracle_det, model, mode=1)
    own = oracle_det.problem(load_cfg(A.OBJ))
    own.jacobian_mode = 1
    assert bytes(P) == bytes(c.problem) and P.jacobian_mode == 1
    assert (bytes(P) == bytes(own)) == (model in ("stock", "general_kernels"))
    axis, off = np.array(P.axis[:]).reshape(2, 21), np.array(P.offset[:]).reshape(2, 21)
    base = np.array(P.base_R[:]).reshape(2, 3, 3)
    calibrated, tilted = model.startswith("calibrated"), model.endswith("tilted")
    assert (not np.array_equal(axis[0], axis[1])) == calibrated and (not np.array_equal(off[0], off[1])) == calibrated
    if calibrated:  # offsets of the order of 1e-3
        stock = np.array(own.offset[:]).reshape(2, 21)
        assert 1e-4 < np.abs(off - stock).max() < 1e-2
    assert (np.count_nonzero(base[1]) > 3) == tilted and np.count_nonzero(base[0]) == 3
    assert np.allclose(base[1] @ base[1].T, np.eye(3), atol=1e-15)


def test_apply_restores_the_option():
    class Ctx:
        def __init__(self):
            self.calls = []

        def set_option(self, name, value):
            self.calls.append((name, value))

    ctx = Ctx()
    with pytest.raises(RuntimeError):
        with A.apply(A.host_constraint(), ctx, "general_kernels"):
            assert ctx.calls == [("stock_kernels", 0)]
            raise RuntimeError("inside")
    assert ctx.calls == [("stock_kernels", 0), ("stock_kernels", 1)]
    with A.apply(A.host_constraint(), ctx, "tilted"):
        pass
    assert len(ctx.calls) == 2


def test_default_scene_follows_the_calibration(oracle_det):
    """the skeleton follows problem.offset: the calibrated default scene is another scene than the stock one; a tilted base leaves it"""
    stock = A.default_scene_host(_model(oracle_det, "stock")[0].problem)
    for model in ("tilted", "calibrated", "calibrated_tilted"):
        sc = A.default_scene_host(_model(oracle_det, model)[0].problem)
        moved = sum(a != b for a, b in zip(sc.spheres, stock.spheres))
        print("%s: %d spheres, %d differ from the stock scene's" % (model, len(sc.spheres), moved if len(sc.spheres) == len(stock.spheres) else -1))
        assert (sc.spheres != stock.spheres) == model.startswith("calibrated")


@pytest.mark.parametrize("scene", ["default", "random"])
@pytest.mark.parametrize("model", ["tilted", "calibrated", "calibrated_tilted"])
def test_clearance_states_have_both_signs(oracle_det, model, scene):
    """default scene: both signs of the clearance occur.  The random scene holds spheres that overlap whatever the state (the clearance is
    negative at every state, here as on stock), so there the flag is taken against clear_margin's median: both values of `free` occur
    and many different pairs attain the minimum"""
    c, P = _model(oracle_det, model)
    sc = A.default_scene_host(c.problem) if scene == "default" else A.HostScene(*_random_proxies())
    clr, pair = oracle_det.clearance_batch(P, sc.spheres, sc.boxes, sc.allowed, _states(oracle_det, P, A.B_CLEAR, A.CLEAR_SEED))
    margin = A.clear_margin(scene, clr)
    print("%s, %s scene: %d of %d states with a positive clearance, %d with a negative one; margin %.4f: %d free; %d different pairs"
          % (model, scene, int((clr > 0).sum()), len(clr), int((clr < 0).sum()), margin, int((clr > margin).sum()), len(set(pair.tolist()))))
    assert (clr > margin).any() and (clr <= margin).any() and len(set(pair.tolist())) > 20
    if scene == "default":
        assert margin == 0.0 and (clr > 0).any() and (clr < 0).any()


def extend_facts(O, c, P, seed):
    """(margin, blocked share, edges blocked at their first state, edges that arrived) of the scene extend test's edges"""
    sc = A.default_scene_host(c.problem)
    frm, to = A.oracle_edges(O, P, A.E_SCENE, seed)
    margin = A.oracle_pick_margin(O, P, sc, frm, to, A.MS_SCENE)
    orc = OracleScene(O, P, sc, margin)
    res = [orc.edge(frm[e], to[e], A.MS_SCENE) for e in range(A.E_SCENE)]
    blocked = np.array([r[5] for r in res])
    first = sum(1 for r in res if r[5] and r[2] == 1)
    return margin, float(blocked.mean()), first, sum(r[0] for r in res)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", A.MODELS)
def test_extend_seed_gives_blocked_and_free_edges(oracle_det, model, mode):
    """test_gpu_geodesic_scene._check_against_oracle's conditions on the oracle alone: blocked share within 0.2 .. 0.8 and at least one
    edge blocked at its first state"""
    c, P = _model(oracle_det, model, mode)
    margin, share, first, arrived = extend_facts(oracle_det, c, P, A.EXTEND_SEED[(model, mode)])
    print("%s mode %d: margin %.6f, blocked share %.3f, blocked at the first state %d, arrived %d of %d" % (model, mode, margin, share, first, arrived, A.E_SCENE))
    assert 0.2 <= share <= 0.8 and first >= 1


@pytest.mark.parametrize("model", ["calibrated", "calibrated_tilted"])
def test_plain_extend_seed_gives_both_flags(oracle_det, model):
    c, P = _model(oracle_det, model, 1)
    frm, to = A.oracle_edges(oracle_det, P, A.E_PLAIN, A.PLAIN_SEED)
    _, n, ok, _ = oracle_det.discrete_geodesic_batch(P, frm, to, A.MS_PLAIN, NCPU)
    print("%s mode 1: %d of %d edges arrived, %d lists full" % (model, int((ok == 1).sum()), A.E_PLAIN, int((n > A.MS_PLAIN).sum())))
    assert 0 < int((ok == 1).sum()) < A.E_PLAIN


def path_facts(O, c, P, model, mode):
    """per scene (False / True): (seg_ok counts, pair_ok counts beyond the neighbours, segments that end unreached behind a stored state)"""
    pj, pl = A.waypoint_paths(c, O, P, A.F_PATHS, A.L_PATHS, A.PATH_SEED[(model, mode)])
    segs = oracle_segments(O, P, pj, pl)
    seg_ok = [s[0] for s in segs.values()]
    zero_row = sum(1 for s in segs.values() if s[0] == 0 and len(s[1]) >= 2)
    sc = A.default_scene_host(c.problem)
    margin = A.oracle_pick_margin(O, P, sc, *A.oracle_edges(O, P, A.E_SCENE, A.EXTEND_SEED[(model, mode)]), A.MS_SCENE)
    out = {}
    for scene in (False, True):
        blocked = []
        ok = oracle_pairs(O, P, pj, pl, edge=A.scene_edge(OracleScene(O, P, sc, margin), blocked) if scene else None)[0]
        flags = [int(ok[f, i, j]) for f, i, j in pairs_py(pj, pl)]
        out[scene] = ((seg_ok.count(1), seg_ok.count(0)), (flags.count(1), flags.count(0)), zero_row, sum(blocked))
    return pl, out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", ["tilted", "calibrated"])
def test_path_seed_gives_both_outcomes(oracle_det, model, mode):
    """both seg_ok values occur; at least one pair beyond the neighbours passes and one does not, with and without the scene; and one
    segment ends unreached behind a state it stored — cut into one-state calls, its last continuation contributes no row"""
    c, P = _model(oracle_det, model, mode)
    pl, facts = path_facts(oracle_det, c, P, model, mode)
    assert pl.tolist() == [2, 3, A.L_PATHS, 1]
    for scene, (seg, pair, zero_row, blocked) in facts.items():
        print("%s mode %d scene %d: seg_ok 1 / 0 = %d / %d, pair_ok 1 / 0 = %d / %d (blocked by the scene: %d), unreached behind a stored state: %d"
              % (model, mode, scene, seg[0], seg[1], pair[0], pair[1], blocked, zero_row))
        assert min(seg) >= 1 and min(pair) >= 1 and zero_row >= 1


def smooth_facts(O, c, P, model, mode):
    """(path_joints, path_len, margin, {scene: the restated result of the smooth test}, the restatement of the same input on the stock problem)"""
    pj, pl = A.waypoint_paths(c, O, P, A.F_PATHS, A.L_PATHS, A.SMOOTH_SEED[(model, mode)])
    sc = A.default_scene_host(c.problem)
    margin = A.oracle_pick_margin(O, P, sc, *A.oracle_edges(O, P, A.E_SCENE, A.EXTEND_SEED[(model, mode)]), A.MS_SCENE)
    fill = mirror_fill(pj, A.SMOOTH_CAP)
    want = {scene: smooth_expect(scene_restatement(O, P, sc, margin) if scene else Restatement(O, P), pj, pl, A.SMOOTH_STEPS, 0.005, A.SMOOTH_CAP, fill)
            for scene in (False, True)}
    stock = smooth_expect(Restatement(O, _model(O, "stock", mode)[1]), pj, pl, A.SMOOTH_STEPS, 0.005, A.SMOOTH_CAP, fill)
    return pj, pl, margin, want, stock


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("model", ["tilted", "calibrated"])
def test_smooth_seed_gives_every_outcome(oracle_det, model, mode):
    """without and with the default scene: a vertex moves, one is refused or below min_change, a midpoint is projected; the result is
    not the stock problem's on the same input, and the scene changes it"""
    c, P = _model(oracle_det, model, mode)
    pj, pl, margin, want, stock = smooth_facts(oracle_det, c, P, model, mode)
    assert pl.tolist() == [2, 3, A.L_PATHS, 1] and A.SMOOTH_CAP == 2 ** A.SMOOTH_STEPS * (A.L_PATHS - 1) + 1
    for scene, w in want.items():
        s = w["stats"].sum(axis=0)
        print("%s mode %d scene %d (margin %.6f): moved %d, stats (projected, fallback, degenerate, refused, below) %s, stop %s, out_len %s"
              % (model, mode, scene, margin, w["moved"].sum(), s.tolist(), w["stop"].tolist(), w["out_len"].tolist()))
        assert w["moved"].sum() >= 1 and s[REFUSED] + s[BELOW] >= 1 and s[PROJECTED] >= 1
        assert not same_f64(w["joints"], stock["joints"])
    assert not same_f64(want[True]["joints"], want[False]["joints"])
