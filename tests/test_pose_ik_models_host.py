"""Pose-targeted IK on the host on every arm model (tests/arm_model_cases.py: stock, tilted, calibrated, calibrated_tilted), against the
ORACLE's kinematics and not against the solver's own text — no device.

ccmp_pose_ik_ref is csrc/ccmp_ik.h compiled for the host, and the device suites compare the kernels with it; what holds the header itself
is here.  Each model runs on targets and seeds sampled on its own manifold (pose_ik_cases.sampled_case(obj, model)).

  one step      with max_rounds = 1 a candidate's record is the iterate after exactly one step: it equals pose_ik_cases.restated_step —
                plain numpy on orc_fk alone, a Jacobian by Richardson central differences, no base frame — from the clamped seed.  A damped
                Newton iteration corrects itself, so only a step-by-step comparison tells a wrong lever arm, damping term or clamp from
                a right one.  The restatement tells the models apart: with the stock problem's arm at the same (q, target) it moves by
                more than 1 000 tolerances.
  trajectory    iterate k (max_rounds = k, k = 1..6) is the restated step from the library's iterate k - 1, and a record `rounds = r`
                means the restated max |e_i| is below eps at iterate r and not before.
  restarts      candidates r = 1..3 are the restated step from orc_ambient_gaussian at ((first_index + t) S + s) R + (r - 1).
  whole rule    tests/test_pose_ik_host.py's checks on every model: the oracle's FK of each solved hand, is_satisfied, joint_valid, the
                selection restated, the solved share.
  vetted rule   on the tilted models' default scene: candidate and slot clearances are the det oracle's, the selection restated.

The tolerance of a step comparison is measured on the restatement (pose_ik_cases.step_tolerance): 200 x the largest difference between
difference step sizes 2e-3 and 4e-3 over the rows of the test, at most 1e-6.

Measured (Wine_Bottle, 400 one-step rows per model):
                      spread      tolerance   library - restatement   clamped / unclamped / on a limit   solved    left out
  stock               1.9e-11     3.8e-9      1.4e-11                 384 / 16 / 102                     37 / 40   0 of 120
  tilted              1.4e-11     2.8e-9      1.3e-11                 376 / 24 / 129                     37 / 40   0 of 120
  calibrated          2.7e-11     5.3e-9      2.5e-11                 384 / 16 / 106                     36 / 40   0 of 120
  calibrated_tilted   1.6e-11     3.3e-9      1.2e-11                 375 / 25 / 131                     37 / 40   0 of 120
(spread: the restatement at the two difference step sizes; left out: trajectory rows within 1e-9 of eps.)  The stock arm at the same
(q, target) moves the step by at least 2.3e-3 rad on every row of the calibrated models and by at least 7.4e-2 rad on arm 1 of the
tilted ones.  The trajectory's 708 to 715 steps per model: spread 1.1e-11 to 6.4e-11, tolerance 2.3e-9 to 1.3e-8, library - restatement
at most 4.4e-11; 24 to 27 of 120 records converge within six rounds.  The 120 restart steps per model: spread at most 1.0e-11, tolerance
at most 2.1e-9, library - restatement at most 6.0e-12.  Vetted rule: margin 0.055 (tilted) and 0.044 (calibrated_tilted), 18 plain
answers kept and 19 refused on both, 24 and 26 of 40 targets solved.

Mutation check (each built into a scratch copy of the library and run against this module; none faulted or hung).  What failed:
  (a) ik_round takes K.base_R[0] for both arms          test_one_step_is_the_restated_step, test_trajectory and test_restart_starts on
                                                        tilted and calibrated_tilted (test_whole_rule passes: the turned error still
                                                        leads to 36 and 37 solved targets)
  (b) ik_fk<false> drops K.ee from ph                   test_one_step_is_the_restated_step, test_trajectory, test_restart_starts on all four
  (c) lambda^2 on the first three diagonal entries      the same three on all four
  (d) the clamp compares n2 with err_clamp              test_one_step_is_the_restated_step and test_trajectory on all four
  (e) ik_start drops the factor R from the index        test_restart_starts on all four
  (f) the second walk clamps to K.lb / K.ub             test_one_step_is_the_restated_step and test_trajectory on all four,
                                                        test_restart_starts on the tilted two, test_whole_rule on all but calibrated
Of these the suite before this module catches (b), (c), (d) and (e) nowhere.  It catches (a) on no tilted base, only on dumbbell, whose
stock base frames differ between the arms, by a solved share that collapses to 0 of 40 (Wine_Bottle: 37 of 40 as before); and (f)
through orc_joint_valid on returned states that lie on a limit itself (tests/test_pose_ik_host.py)."""
import numpy as np
import pytest

import arm_model_cases as M
import ik_vet_cases as V
import pose_ik_cases as K

MODELS = ("stock", "tilted", "calibrated", "calibrated_tilted")
OBJ = "Wine_Bottle"
RNG_SEED = 0x1CE
EPS = 1e-5  # ccmp_ik_opts' default


@pytest.fixture(scope="module")
def ik(ccmp_built):
    from closed_chain_motion_planner_amd import ik_options, pose_ik_ref

    return pose_ik_ref, ik_options


def _rows(orc, OP, opts, items, fk_problem=None):
    """restated_step at both difference step sizes over items (arm, pose, q7): fine (n,7), coarse (n,7), emax (n,)"""
    fine, coarse, emax = [], [], []
    for arm, pose, q in items:
        f, e = K.restated_step(orc, OP, arm, pose, q, opts, K.H_FINE, fk_problem)
        fine.append(f)
        coarse.append(K.restated_step(orc, OP, arm, pose, q, opts, K.H_COARSE, fk_problem)[0])
        emax.append(e)
    return np.array(fine), np.array(coarse), np.array(emax)


@pytest.mark.parametrize("model", MODELS)
def test_one_step_is_the_restated_step(ik, model):
    pose_ik_ref, ik_options = ik
    orc, OP, _, _, targets, seeds = K.sampled_case(OBJ, model)
    opts = ik_options(restarts=0, max_rounds=1)
    out = pose_ik_ref(K.model_problem(OBJ, model), targets, seeds, rng_seed=RNG_SEED, opts=opts, want_candidates=True)
    lo, hi = K.joint_box(OP)
    where = [(t, s, a) for t in range(len(targets)) for s in range(seeds.shape[1]) for a in (0, 1) if out["cand_rounds"][t, s, a, 0] != 0]
    items = [(a, targets[t], np.clip(seeds[t, s, 7 * a:7 * a + 7], lo, hi)) for t, s, a in where]
    got = np.array([out["cand_q"][t, s, a, 0] for t, s, a in where])
    fine, coarse, _ = _rows(orc, OP, opts, items)
    tol, spread = K.step_tolerance(fine, coarse)
    # the conditions, on the restatement alone
    norm = np.array([np.linalg.norm(K.restated_error(orc, OP, a, pose, q)) for a, pose, q in items])
    clamped = int((norm > opts.err_clamp).sum())
    on_limit = int(((fine == lo) | (fine == hi)).any(axis=1).sum())
    worst = float(np.abs(got - fine).max())
    print("%s: %d rows, reference spread %.3g, tolerance %.3g, library - restatement %.3g; error clamp active on %d, inactive on %d; %d rows end on a "
          "joint limit" % (model, len(where), spread, tol, worst, clamped, len(where) - clamped, on_limit))
    assert len(where) >= 300 and 0 < clamped < len(where) and on_limit >= 1
    assert worst <= tol, (worst, tol, [where[i] for i in np.flatnonzero(np.abs(got - fine).max(axis=1) > tol)[:8]])
    # the restatement sees the model: the stock arm at the same (q, target) steps elsewhere
    if model != "stock":
        stock = K.sampled_case(OBJ)[1]
        sel = np.array([model != "tilted" or a == 1 for _, _, a in where])
        other = _rows(orc, OP, opts, [it for it, k in zip(items, sel) if k], fk_problem=stock)[0]
        d = np.abs(other - fine[sel]).max(axis=1)
        print("%s: the stock arm's step differs by %.3g .. %.3g rad over %d rows" % (model, d.min(), d.max(), len(d)))
        assert (d > 1000.0 * tol).mean() >= 0.9


@pytest.mark.parametrize("model", MODELS)
def test_trajectory(ik, model):
    pose_ik_ref, ik_options = ik
    orc, OP, _, _, targets, seeds = K.sampled_case(OBJ, model)
    T, S, ROUNDS = 12, seeds.shape[1], 6
    targets, seeds = targets[:T], seeds[:T]
    P = K.model_problem(OBJ, model)
    runs = {k: pose_ik_ref(P, targets, seeds, rng_seed=RNG_SEED, opts=ik_options(restarts=0, max_rounds=k), want_candidates=True) for k in range(1, ROUNDS + 1)}
    opts = ik_options(restarts=0, max_rounds=ROUNDS)
    assert opts.eps == EPS
    lo, hi = K.joint_box(OP)
    last = runs[ROUNDS]["cand_rounds"][..., 0]
    assert ((last >= -1) & (last <= ROUNDS)).all() and (last == -1).any() and (last > 0).any()  # converged and unconverged records
    where = [(t, s, a) for t in range(T) for s in range(S) for a in (0, 1)]

    def iterate(k, t, s, a):  # the library's iterate k of a row that had not converged before it
        return np.clip(seeds[t, s, 7 * a:7 * a + 7], lo, hi) if k == 0 else runs[k]["cand_q"][t, s, a, 0]

    steps, emax_at = [], {}
    for t, s, a in where:
        r = int(last[t, s, a])
        n = ROUNDS if r < 0 else r  # steps taken
        for k in range(1, ROUNDS + 1):  # a shorter run's record is the longer one's, cut
            assert runs[k]["cand_rounds"][t, s, a, 0] == (r if 0 <= r <= k else -1), (t, s, a, k)
        steps += [((t, s, a, k), (a, targets[t], iterate(k - 1, t, s, a))) for k in range(1, n + 1)]
        emax_at[(t, s, a, n)] = float(np.abs(K.restated_error(orc, OP, a, targets[t], iterate(n, t, s, a))).max())
    fine, coarse, emax = _rows(orc, OP, opts, [it for _, it in steps])
    tol, spread = K.step_tolerance(fine, coarse)
    got = np.array([iterate(k, t, s, a) for (t, s, a, k), _ in steps])
    worst = float(np.abs(got - fine).max())
    for ((t, s, a, k), _), e in zip(steps, emax):
        emax_at[(t, s, a, k - 1)] = float(e)
    # rounds = r: below eps at iterate r, not before; never below: rounds = -1.  Rows within 1e-9 of eps at any iterate are left out
    left_out = 0
    for t, s, a in where:
        r = int(last[t, s, a])
        e = np.array([emax_at[(t, s, a, k)] for k in range((ROUNDS if r < 0 else r) + 1)])
        if (np.abs(e - EPS) < 1e-9).any():
            left_out += 1
            continue
        assert (e[:-1] >= EPS).all() and ((e[-1] < EPS) if r >= 0 else (e[-1] >= EPS)), (t, s, a, r, e)
    print("%s: %d steps of %d rows, reference spread %.3g, tolerance %.3g, library - restatement %.3g; records: %d converged within %d rounds, %d not; "
          "%d of %d rows left out (within 1e-9 of eps)" % (model, len(steps), len(where), spread, tol, worst, int((last >= 0).sum()), ROUNDS,
                                                           int((last < 0).sum()), left_out, len(where)))
    assert worst <= tol, (worst, tol)
    assert left_out <= 0.02 * len(where)


@pytest.mark.parametrize("model", MODELS)
def test_restart_starts(ik, model):
    pose_ik_ref, ik_options = ik
    orc, OP, _, _, targets, seeds = K.sampled_case(OBJ, model)
    T, S, R, FIRST = 4, seeds.shape[1], 3, 11
    targets, seeds = targets[:T], seeds[:T]
    opts = ik_options(restarts=R, max_rounds=1)
    P = K.model_problem(OBJ, model)
    out = pose_ik_ref(P, targets, seeds, rng_seed=RNG_SEED, first_index=FIRST, opts=opts, want_candidates=True)
    where = [(t, s, a, r) for t in range(T) for s in range(S) for a in (0, 1) for r in range(1, R + 1)]
    starts = {(t, s, r): K.restart_start(orc, OP, opts, RNG_SEED, FIRST, t, s, S, r) for t, s, _, r in where}
    assert len({tuple(v) for v in starts.values()}) == T * S * R  # every (t, s, r) its own draw
    assert (out["cand_rounds"][..., 1:] != 0).all()  # no restart starts on its target: every record is one step on
    fine, coarse, _ = _rows(orc, OP, opts, [(a, targets[t], starts[(t, s, r)][7 * a:7 * a + 7]) for t, s, a, r in where])
    tol, spread = K.step_tolerance(fine, coarse)
    got = np.array([out["cand_q"][t, s, a, r] for t, s, a, r in where])
    worst = float(np.abs(got - fine).max())
    print("%s: %d restart candidates, reference spread %.3g, tolerance %.3g, library - restatement %.3g" % (model, len(where), spread, tol, worst))
    assert worst <= tol, (worst, tol)
    other = pose_ik_ref(P, targets, seeds, rng_seed=RNG_SEED, first_index=0, opts=opts, want_candidates=True)
    assert (np.abs(other["cand_q"][..., 1:, :] - out["cand_q"][..., 1:, :]).max(axis=-1) > 1000.0 * tol).all()  # the restarts follow first_index
    assert np.array_equal(other["cand_q"][..., 0, :].view(np.uint64), out["cand_q"][..., 0, :].view(np.uint64))


@pytest.fixture(scope="module")
def solved(ik):
    """each model's own 40 targets through the whole rule, once"""
    pose_ik_ref = ik[0]
    out = {}

    def run(model):
        if model not in out:
            targets, seeds = K.sampled_case(OBJ, model)[4:]
            out[model] = pose_ik_ref(K.model_problem(OBJ, model), targets, seeds, rng_seed=RNG_SEED, want_candidates=True)
        return out[model]

    return run


@pytest.mark.parametrize("model", MODELS)
def test_whole_rule(solved, model):
    orc, OP, _, _, targets, seeds = K.sampled_case(OBJ, model)
    P, out = K.model_problem(OBJ, model), solved(model)
    assert np.allclose(P.t_o7_R[:], OP.t_o7_R[:], rtol=0, atol=1e-13) and np.allclose(P.t_o7_p[:], OP.t_o7_p[:], rtol=0, atol=1e-13)
    worst = 0.0
    for t in range(len(targets)):
        if not out["ok"][t]:
            assert np.isnan(out["q"][t]).all() and out["which"][t] == -1
            continue
        assert 0 <= out["which"][t] < seeds.shape[1]
        for arm in (0, 1):
            e = np.abs(K.restated_error(orc, OP, arm, targets[t], out["q"][t, 7 * arm:7 * arm + 7]))
            worst = max(worst, float(e.max()))
            assert (e < EPS + 1e-9).all(), (t, arm, e)
        assert orc.is_satisfied(OP, out["q"][t]) and orc.joint_valid(OP, out["q"][t]), t
    q, ok, which = K.select(out["cand_q"], out["cand_rounds"], seeds)
    assert np.array_equal(ok, out["ok"]) and np.array_equal(which, out["which"])
    assert np.array_equal(q.view(np.uint64), out["q"].view(np.uint64))
    rounds = out["cand_rounds"]
    took_restart = [t for t in np.flatnonzero(out["ok"]) if (rounds[t, out["which"][t], :, 0] < 0).any()]
    n_ok = int(out["ok"].sum())
    print("%s: %d of %d targets solved, %d by the first slot, %d winning slots took a restart; worst twist component %.3g"
          % (model, n_ok, len(targets), int((out["which"] == 0).sum()), len(took_restart), worst))
    assert len(took_restart) >= 1
    assert n_ok >= 0.75 * len(targets)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("model", ["tilted", "calibrated_tilted"])
def test_vetted_rule(solved, oracle_det, model):
    from closed_chain_motion_planner_amd import pose_ik_vetted_ref

    targets, seeds = K.sampled_case(OBJ, model)[4:]
    P, plain = K.model_problem(OBJ, model), solved(model)
    OP = oracle_det.problem_from_bytes(bytes(P))
    sc = M.default_scene_host(P)
    # the margin: the median of the oracle's clearance over the plain answers, so the scene keeps some and refuses some
    rows = np.flatnonzero(plain["ok"])
    clr = oracle_det.clearance_batch(OP, sc.spheres, sc.boxes, sc.allowed, plain["q"][rows])[0]
    margin = float(np.median(clr))
    kept, refused = int((clr > margin).sum()), int((~(clr > margin)).sum())
    assert kept > 0 and refused > 0
    out = pose_ik_vetted_ref(P, targets, seeds, sc.spheres, sc.boxes, sc.allowed, margin, rng_seed=RNG_SEED, want_candidates=True)
    assert np.array_equal(_bits(out["cand_q"]), _bits(plain["cand_q"])) and np.array_equal(out["cand_rounds"], plain["cand_rounds"])
    assert np.array_equal(out["cand_clear"] == -np.inf, out["cand_rounds"] < 0)
    for a in (0, 1):
        conv = out["cand_rounds"][:, :, a] >= 0
        want = oracle_det.clearance_batch(OP, V.sub_scene(sc.spheres, a), sc.boxes, sc.allowed, V.state_of(P, a, out["cand_q"][:, :, a][conv]))[0]
        assert np.array_equal(_bits(out["cand_clear"][:, :, a][conv]), _bits(want)), a
    q, ok, which, assembled = V.select_vetted(out["cand_q"], out["cand_rounds"], out["cand_clear"], out["slot_clear"], seeds, margin)
    assert np.array_equal(ok, out["ok"]) and np.array_equal(which, out["which"]) and np.array_equal(_bits(q), _bits(out["q"]))
    for t in range(len(targets)):
        for s in range(seeds.shape[1]):
            if assembled[t][s] is None:
                assert np.isnan(out["slot_clear"][t, s])
            else:
                assert _bits(out["slot_clear"][t, s]) == _bits(oracle_det.clearance(OP, sc.spheres, sc.boxes, sc.allowed, assembled[t][s])[0]), (t, s)
        assert _bits(out["clearance"][t]) == _bits(out["slot_clear"][t, which[t]] if ok[t] else np.nan)
    # a kept plain answer is the vetted answer
    keep = rows[clr > margin]
    assert np.array_equal(_bits(out["q"][keep]), _bits(plain["q"][keep])) and np.array_equal(out["which"][keep], plain["which"][keep])
    print("%s: margin %.6f (the oracle's median over %d plain answers): %d kept, %d refused; the vetted call solves %d of %d"
          % (model, margin, len(rows), kept, refused, int(out["ok"].sum()), len(targets)))
