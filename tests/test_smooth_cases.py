"""The case builders of tests/smooth_cases.py checked on the oracle alone (no device): each batch of tests/test_gpu_smooth_shapes.py holds
the shapes, stops and verdicts its test is about, so that no GPU run is spent finding one.  These are conditions on the restatement, not
measurements; the seeds in smooth_cases.py were chosen until the oracle met them.  The figures behind each are printed (pytest -s).
Wall time on one host core: 3.4 s for the module, all but 0.1 s of it the batches and their restatements (wide 0.9 s in FD mode and
0.6 s in analytic mode, long 0.6 s, straddle 0.4 s, identity 0.2 s)."""
import time

import numpy as np
import pytest

import arm_model_cases as A
import smooth_cases as S
from smooth_cases import BELOW, PROJECTED, REFUSED, Restatement, expect, same_f64
from test_gpu_parity import _oracle_problem

GUARD = -7.0


@pytest.fixture(scope="module", params=[0, 1], ids=["fd", "analytic"])
def wide(request, oracle_det):
    t = time.perf_counter()
    case = S.wide_batch(oracle_det, S.stock_problem(oracle_det, request.param))
    want = {ms: expect(case["R"], case["pj"], case["pl"], ms, case["min_change"], case["out_max_len"], GUARD) for ms in (3, 2)}
    print("wide batch, mode %d: built and restated twice in %.2f s" % (request.param, time.perf_counter() - t))
    return case, want


def test_wide_batch_shape(wide):
    case, _ = wide
    pj, pl = case["pj"], case["pl"]
    assert pj.shape == (70, 6, 14) and (case["max_steps"], case["out_max_len"]) == (3, 9)
    assert pl.tolist() == [S.WIDE_CYCLE[f % 10] for f in range(70)] and S.WIDE_CYCLE == (3, 5, 0, 4, 1, 3, 2, 6, 3, 4)
    for f in range(70):
        L = int(pl[f])
        assert np.isnan(pj[f, L:]).all()  # rows behind the length are NaN
        assert np.isfinite(pj[f, :L]).all() == (f != S.WIDE_NAN_PATH)
    bad = pj[S.WIDE_NAN_PATH, : pl[S.WIDE_NAN_PATH]]
    assert pl[S.WIDE_NAN_PATH] == 5 and np.isnan(bad[1:-1]).any() and np.isfinite(bad[[0, -1]]).all()  # an interior row


def test_wide_batch_outcomes(wide):
    case, wants = wide
    want, pl = wants[3], case["pl"]
    first, second = want["passes"] >= 1, want["passes"] >= 2
    total = want["stats"].sum(axis=0)
    print("stops at max_steps 3 %s, at 2 %s; active in pass 1 %d, in pass 2 %d; passes %s; stats %s, moved %d; min_change %.17g"
          % (np.bincount(want["stop"], minlength=5), np.bincount(wants[2]["stop"], minlength=5), first.sum(), second.sum(),
             np.bincount(want["passes"], minlength=3), total, want["moved"].sum(), case["min_change"]))
    # with a result of 9 vertices no path runs three passes, so stop 2 needs max_steps 2: the GPU test runs both
    assert set(want["stop"].tolist()) == {0, 1, 3, 4} and set(wants[2]["stop"].tolist()) == {0, 1, 2, 3, 4}
    assert want["stop"][S.WIDE_NAN_PATH] == 4 and (want["stop"] == 4).sum() == 1 and (want["stop"][pl < 3] == 0).all()
    assert first.sum() >= 40 and 17 <= second.sum() < first.sum() and not (second & ~first).any()
    assert set(want["passes"].tolist()) == {0, 1, 2}  # finished paths lie in both buffers
    assert min(total[PROJECTED], total[REFUSED], total[BELOW], want["moved"].sum()) >= 1
    assert (want["stop"] == 1).sum() >= 1
    # the capacity: 3 waypoints run two passes, 4 or 5 one, 6 none
    going = (want["stop"] == 3) | (want["stop"] == 2)
    assert (want["passes"][going & (pl == 3)] == 2).all() and (want["passes"][going & ((pl == 4) | (pl == 5))] == 1).all()
    assert (want["passes"][pl == 6] == 0).all() and (want["stop"][pl == 6] == 3).all()
    for a, b in ((want, wants[2]),):  # max_steps 2 changes the stop of the paths that ran two moving passes, nothing else
        assert all(np.array_equal(a[k], b[k]) for k in ("out_len", "passes", "moved", "stats")) and same_f64(a["joints"], b["joints"])
        assert ((a["stop"] != b["stop"]) == ((a["stop"] == 3) & (a["passes"] == 2))).all()


@pytest.fixture(scope="module")
def long_(oracle_det):
    t = time.perf_counter()
    P = S.stock_problem(oracle_det, 0)
    case = S.long_batch(oracle_det, P)
    want = expect(Restatement(oracle_det, P), case["pj"], case["pl"], case["max_steps"], case["min_change"], case["out_max_len"], GUARD)
    print("long batch: built and restated in %.2f s" % (time.perf_counter() - t))
    return case, want


def test_long_batch(long_):
    case, want = long_
    assert case["pl"].tolist() == [70, 33, 2] and case["pj"].shape == (3, 70, 14) and (case["max_steps"], case["out_max_len"]) == (2, 139)
    print("moved %s, stats %s" % (want["moved"], want["stats"].tolist()))
    assert want["stop"].tolist() == [3, 2, 0] and want["passes"].tolist() == [1, 2, 0] and want["out_len"].tolist() == [139, 129, 2]
    assert (want["moved"][:2] > 0).all() and want["moved"][2] == 0
    # distances summed: 69 and 32 going in, 138 and 128 coming out — 64 + 5, 2 x 64 + 10, half a chunk, two chunks exactly
    assert [int(n) - 1 for n in case["pl"][:2]] == [69, 32] and [int(n) - 1 for n in want["out_len"][:2]] == [138, 128]


def test_identity_batch(oracle_det):
    case = S.identity_batch()
    pj, pl = case["pj"], case["pl"]
    assert pl.tolist() == [0, 1, 2, 3, 64, 65, 66, 129, 130] and pj.shape == (9, 130, 14) and np.isfinite(pj).all()
    assert (case["max_steps"], case["out_max_len"]) == (0, 130)
    want = S.identity_expect(case, GUARD)
    assert want["stop"].tolist() == [0, 0, 0, 2, 2, 2, 2, 2, 2] and want["length_in"][:2].tolist() == [0.0, 0.0] and not np.signbit(want["length_in"][:2]).any()
    # the definition and the restatement of the loop agree (the restatement traverses nothing at max_steps 0)
    S.same_result(expect(Restatement(oracle_det, S.stock_problem(oracle_det, 0)), pj, pl, 0, 0.005, 130, GUARD), want, "identity")


def test_straddle_scene_case(oracle_det):
    c = A.host_constraint(0)
    c.problem.delta = S.stock_problem(oracle_det, 0).delta
    P = _oracle_problem(oracle_det, c)
    assert bytes(P) == bytes(S.stock_problem(oracle_det, 0))
    sc = A.default_scene_host(c.problem)
    case = S.straddle_scene_case(oracle_det, P, sc)
    rows, margin, i = case["pj"][0], case["margin"], S.STRADDLE_VERTEX
    facts = S.straddle_facts(oracle_det, P, sc, rows, margin)
    ok, clear_in, clear_out, clear_c = facts[i - 1]
    print("seed %#x, vertex %d, margin %.17g: clearance(m_%d) %.17g, clearance(m_%d) %.17g, clearance(c) %.17g"
          % (S.STRADDLE_SEED, i, margin, i - 1, clear_in, i, clear_out, clear_c))
    # an interior vertex that passes both tests, with its candidate clear, whose two midpoints lie on different sides of the margin
    assert ok and clear_c >= margin and (clear_in >= margin) != (clear_out >= margin)
    args = (case["pj"], case["pl"], case["max_steps"], case["min_change"], case["out_max_len"], 0.0)
    want = expect(S.scene_restatement(oracle_det, P, sc, margin), *args)
    assert want["moved"][0] >= 1 and want["stats"][0, REFUSED] >= 1  # accepted vertices with the scene, and the straddling one refused
    # the clearance of the "from" midpoint taken at m_i instead of m_{i-1} gives another result
    wrong = expect(S.scene_restatement(oracle_det, P, sc, margin, S.WrongMidpoint), *args)
    assert not same_f64(want["joints"], wrong["joints"])
    one = [expect(S.scene_restatement(oracle_det, P, sc, margin, cls), case["pj"], case["pl"], 1, case["min_change"], case["out_max_len"], 0.0)
           for cls in (Restatement, S.WrongMidpoint)]
    # in the first pass the straddling vertex (row 2 i of the subdivided path) stays where it was; read at m_i it moves
    assert same_f64(one[0]["joints"][0, 2 * i], rows[i]) and not same_f64(one[1]["joints"][0, 2 * i], rows[i])
    plain = expect(Restatement(oracle_det, P), *args)
    assert not same_f64(want["joints"], plain["joints"])
