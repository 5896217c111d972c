"""The batches of tests/test_gpu_setpoints.py contain what their tests are about — asserted here on the oracle and the plain-Python
restatement alone, no device, so a seed or a constant that stops producing the case fails on every machine and not only where the GPU suite
runs."""
import numpy as np
import pytest

import setpoint_cases as sc
from setpoint_cases import ACC, CLEARANCE, EMPTY, FULL, NONFINITE, OK, POINT, SPEED, UNORDERED


@pytest.fixture(scope="module")
def ref():
    return sc.reference()


def test_ragged_batch_has_every_size_and_status(ref):
    case, want = ref["ragged"]["case"], ref["ragged"]["want"]
    assert np.diff(case["path_first"]).tolist() == [0, 1, 2, 3, 17, 70, 5] + [3] * 5
    assert want["status"].tolist() == case["statuses"] == [EMPTY, POINT, OK, OK, OK, OK, OK, NONFINITE, NONFINITE, UNORDERED, UNORDERED, UNORDERED]
    assert np.diff(want["tick_first"]).tolist() == case["ticks"] == [0, 1, 2, 15, 257, 17, 16, 0, 0, 0, 0, 0]
    pf, t = case["path_first"], case["time"]
    assert np.isnan(case["rows"][pf[7]:pf[8]]).any() and np.isfinite(t[pf[7]:pf[8]]).all()  # the NaN coordinate
    assert np.isnan(t[pf[8]:pf[9]]).any() and np.isfinite(case["rows"][pf[8]:pf[9]]).all()  # the NaN stamp
    assert t[pf[9]] != 0.0 and (np.diff(t[pf[9]:pf[10]]) > 0).all()                          # t_0 != 0, otherwise ordered
    assert t[pf[10]] == 0.0 and (np.diff(t[pf[10]:pf[11]]) < 0).any()                        # a decreasing stamp
    d = np.diff(t[pf[11]:pf[12]])
    assert t[pf[11]] == 0.0 and (d >= 0).all() and (d == 0).any()                            # a repeated stamp on rows that differ
    # N = 2: the period is longer than the duration
    assert t[pf[3] - 1] < case["period"]
    # the 70-row path: a period of several row intervals, so consecutive interior ticks skip rows
    ks = want["brackets"][5]
    assert len(ks) == 15 and min(np.diff(ks)) >= 2
    # the 17-row path at 257 ticks: many ticks per bracket, every bracket met
    assert sorted(set(want["brackets"][4])) == list(range(1, 17))
    # the rows are on the manifold, the setpoints between them are not projected: some are off it, none by much
    assert all(ref["O"].is_satisfied(ref["P"], x) for x in case["run"]) and np.isfinite(want["f"]).all() and (want["f"] >= 0).all()
    assert want["counts"][:, 1].sum() == 0 and np.isnan(want["clearance"]).all()
    assert (want["peak_tick"][:, CLEARANCE] == -1).all() and np.isinf(want["peak"][:, CLEARANCE]).all()
    # a tangent without the sign test would differ: joint slopes change sign inside the 70-row path
    r, tt = case["rows"][pf[5]:pf[6]], t[pf[5]:pf[6]]
    m = np.diff(r, axis=0) / np.diff(tt)[:, None]
    assert ((m[:-1] * m[1:]) < 0).sum() >= 5
    assert not sc.same_f64(sc.tangents_py(r, tt), np.nan_to_num(sc.tangents_py(r, tt, sign_test=False)))
    # the audit measures something: moving paths have peaks at interior ticks, the stretch follows them
    for p in (3, 4, 5, 6):
        assert want["peak"][p, SPEED] > 0 and want["peak"][p, ACC] > 0 and 0 < want["peak_tick"][p, SPEED] < case["ticks"][p] - 1
        assert want["stretch"][p] == max(1.0, want["peak"][p, SPEED], np.sqrt(want["peak"][p, ACC]))
    assert want["stretch"][0] == 1.0 and want["stretch"][1] == 1.0 and want["peak_tick"][1].tolist() == [0, -1, 0, 0, -1]


def test_on_the_stamp_has_ticks_that_equal_stamps(ref):
    case, want = ref["on_the_stamp"]["case"], ref["on_the_stamp"]["want"]
    pf, t, tf = case["path_first"], case["time"], want["tick_first"]
    assert want["status"].tolist() == [OK, OK] and np.diff(tf).tolist() == [33, 45]
    for p in (0, 1):
        stamps, tau = t[pf[p]:pf[p + 1]].tolist(), want["tau"][tf[p]:tf[p + 1]]
        assert all(v * 2 ** 7 == int(v * 2 ** 7) for v in stamps)
        interior = tau[1:-1]
        on = [j + 1 for j, v in enumerate(interior) if v in stamps]
        assert len(on) >= 6 and (p == 1 or on == list(range(4, 32, 4)))  # path 0: every fourth tick
        exact = []
        for j in on:  # `>=`: the interval that ENDS at the stamp; `>` would take the next one
            k = want["brackets"][p][j - 1]
            assert stamps[k] == tau[j] and sc.bracket_py(stamps, float(tau[j]), strict=True) == k + 1
            exact.append(sc.same_f64(want["q"][tf[p] + j], case["rows"][pf[p] + k]))  # u == 1: a + (b - a), the row itself only while b - a is exact
        # path 0 (geodesic rows 0.05 apart): the row from either side; path 1 (random rows): the rounding shows, so `>` differs in bits
        assert all(exact) if p == 0 else not all(exact)
    wrong = sc.setpoints_py(case["rows"], pf, t, sc.PANDA_VMAX, sc.PANDA_AMAX, case["period"], mutate=("bracket",))
    assert sc.same_f64(wrong["q"][:tf[1]], want["q"][:tf[1]]) and not sc.same_f64(wrong["q"][tf[1]:], want["q"][tf[1]:])
    assert (np.array([v * 2.0 ** 9 for v in want["tau"]]) % 1 == 0).all()  # every product j * period is exact


def test_still_batch_ties_on_every_tick(ref):
    case, want = ref["still"]["case"], ref["still"]["want"]
    tf = want["tick_first"]
    assert want["status"].tolist() == [OK, OK] and np.diff(tf).tolist() == [sc.count_py(0.016, 0.001), sc.count_py(0.017, 0.001)]
    q0 = want["q"][tf[0]:tf[1]]
    assert (sc.bits(q0) == sc.bits(q0[0])).all() and (want["qd"][tf[0]:tf[1]] == 0.0).all()
    f0 = want["f"][tf[0]:tf[1]]
    assert (sc.bits(f0) == sc.bits(f0[0])).all()
    assert want["peak_tick"][0].tolist() == [0, 0, 0, 0, -1] and want["peak"][0, :2].tolist() == [0.0, 0.0] and want["stretch"][0] == 1.0
    t = case["time"][case["path_first"][1]:]
    assert (np.diff(t) == 0).sum() == 2 and want["peak"][1, SPEED] > 0  # repeated stamps on repeated rows, and the path moves
    assert all(t[k] > t[k - 1] for k in want["brackets"][1])  # a zero-width interval is never a bracket


def test_full_batch_refuses_one_path(ref):
    case, want = ref["full"]["case"], ref["full"]["want"]
    assert case["max_ticks"] == 257 - 1 and want["status"].tolist() == [OK, FULL, OK] and np.diff(want["tick_first"]).tolist() == case["ticks"]
    whole = ref["ragged"]["want"]
    for mine, theirs in ((0, 3), (2, 6)):  # the others are untouched: the ragged batch's results
        a, b = want["tick_first"][mine], want["tick_first"][mine + 1]
        c, d = whole["tick_first"][theirs], whole["tick_first"][theirs + 1]
        assert sc.same_f64(want["q"][a:b], whole["q"][c:d]) and sc.same_f64(want["peak"][mine], whole["peak"][theirs])
    assert want["peak_tick"][1].tolist() == [-1] * 5 and want["stretch"][1] == 1.0


def test_scene_minimum_lies_between_two_rows(ref):
    case, want = ref["scene"]["case"], ref["scene"]["want"]
    clr, tau, t = want["clearance"], want["tau"], case["time"]
    j = int(want["peak_tick"][0, CLEARANCE])
    assert want["status"].tolist() == [OK] and np.isfinite(clr).all() and clr[j] == clr.min() == want["peak"][0, CLEARANCE]
    assert t[0] < tau[j] < t[1] and tau[j] not in t.tolist()  # strictly between rows 0 and 1
    assert clr[j] < min(case["at_rows"])  # smaller than at every row
    assert clr[j] < case["margin"] < min(case["at_rows"])  # the rows are free under the margin, the motion between them is not
    n_below = int(want["counts"][0, 1])
    assert 0 < n_below < want["ticks"] and n_below == int((clr < case["margin"]).sum())
