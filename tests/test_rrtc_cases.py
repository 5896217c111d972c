"""The plain-Python restatement of the RRT-Connect rule (tests/rrtc_cases.py) checked by itself: hand-worked picks, the commit's total
order, the best gap's strict fold and the solution test.  No library beyond ccmp_joint_distance (the arc's steps), no device."""
import numpy as np

import rrtc_cases as R


def _rows(steps, ms=4):
    return R.line_list(steps, ms)


def test_the_arc_keeps_a_row_that_lands_on_the_range(ccmp_built):
    rows = _rows([0.25, 0.25, 0.25])
    assert R.arc(rows, 0.5) == (2, 0.5, False)
    assert R.arc(rows, 0.4999999999999999)[0] == 1
    assert R.arc(rows, 0.1)[0] == 0 and R.arc(rows[:1], 0.5) == (0, 0.0, False)
    bad = rows.copy()
    bad[1, 3] = np.nan
    assert R.arc(bad, 0.5)[2]


def test_extend_by_hand(ccmp_built):
    rows = _rows([0.25, 0.25, 0.25])
    # d <= range: ok decides, then the cut
    assert R.extend(rows, 2, 4, 1, 0.5, 0.5) == (R.REACHED, -1)
    assert R.extend(rows, 2, 4, 0, 0.5, 0.5) == (R.TRAPPED, -1)
    assert R.extend(rows, 2, 4, 2, 0.25, 0.5) == (R.UNSETTLED, -1)
    assert R.extend(rows, 5, 4, 0, 0.25, 0.5) == (R.UNSETTLED, -1)
    # d > range: the clip
    assert R.extend(rows, 4, 4, 0, 2.0, 0.5) == (R.ADVANCED, 2)
    assert R.extend(rows, 4, 4, 1, 2.0, 0.6) == (R.ADVANCED, 2)
    assert R.extend(rows, 1, 4, 0, 2.0, 0.5) == (R.TRAPPED, -1)
    assert R.extend(rows, 1, 4, 2, 2.0, 0.5) == (R.TRAPPED, -1)  # only `from` is listed: trapped comes first
    assert R.extend(rows, 4, 4, 0, 2.0, 0.1) == (R.ADVANCED, 1)  # at least one step of progress
    assert R.extend(rows, 5, 4, 0, 2.0, 0.75) == (R.UNSETTLED, -1)  # the arc was not used up inside a cut list
    assert R.extend(rows, 5, 4, 0, 2.0, 0.5) == (R.ADVANCED, 2)  # a cut list whose clip lies inside it
    assert R.extend(rows, 2, 4, 2, 2.0, 0.1) == (R.ADVANCED, 1)  # suspended, but the first step already went beyond the range
    assert R.extend(rows, 3, 4, 2, 2.0, 0.75) == (R.UNSETTLED, -1)
    assert R.extend(rows, 3, 4, 0, float("nan"), 0.5) == (R.TRAPPED, -1)
    assert R.extend(rows, 3, 4, 1, 0.25, 0.5, use=0) == (R.NONE, -1) and R.extend(rows, 3, 4, 1, 0.25, 0.5, use=2) == (R.TRAPPED, -1)
    assert R.extend(rows, 0, 4, 1, 0.25, 0.5) == (R.TRAPPED, -1)


def test_connect_by_hand(ccmp_built):
    rows = _rows([0.25, 0.25, 0.25])
    v = rows[2].copy()
    v[0] += 0.125
    assert R.connect(rows, 3, 4, 1, v) == (R.C_JOINED, -1, 0.125)
    assert R.connect(rows, 3, 4, 0, v) == (R.C_ADDED, 2, 0.125)
    assert R.connect(rows, 5, 4, 0, v)[:2] == (R.C_ADDED, 3) and R.connect(rows, 3, 4, 2, v)[:2] == (R.C_ADDED, 2)
    assert R.connect(rows, 1, 4, 0, v)[:2] == (R.C_NOTHING, -1) and R.connect(rows, 1, 4, 0, v)[2] == 0.625
    o, r, g = R.connect(rows, 0, 4, 1, v)
    assert (o, r) == (R.C_NOTHING, -1) and g != g
    assert R.connect(rows, 3, 4, 1, v, use=0)[0] == R.NONE and R.connect(rows, 3, 4, 1, v, use=2)[0] == R.C_NOTHING


def _picks(oa, ob, gaps):
    W = len(oa)
    pa = {"outcome": np.array(oa, dtype=np.int32), "row": np.arange(W)[:, None] + np.zeros((W, 14))}
    pb = {"outcome": np.array(ob, dtype=np.int32), "row": 100.0 + np.arange(W)[:, None] + np.zeros((W, 14)), "gap": np.array(gaps, dtype=np.float64)}
    return pa, pb


def test_commit_takes_indices_in_the_stated_total_order(ccmp_built):
    """step 2's vertices in ascending sample order, then step 3's in ascending sample order; the edges likewise"""
    oa = [R.ADVANCED, R.TRAPPED, R.REACHED, R.NONE, R.ADVANCED, R.UNSETTLED]
    ob = [R.C_ADDED, R.NONE, R.C_JOINED, R.NONE, R.C_NOTHING, R.NONE]
    nan = float("nan")
    pa, pb = _picks(oa, ob, [0.5, nan, 0.25, nan, 0.25, nan])
    idx_a, idx_b = np.array([3, 1, 4, -1, 0, 2]), np.array([7, 0, 8, 0, 9, 0])
    use = np.array([1, 1, 1, 0, 1, 1], dtype=np.uint8)
    s0 = R.new_state([0], [5], first_index=10)
    s, rows, uv = R.commit(s0, 20, True, use, pa, idx_a, pb, idx_b)
    assert rows[:, 0].tolist() == [0.0, 2.0, 4.0, 100.0]  # A's rows of samples 0, 2, 4, then B's row of sample 0
    assert uv.tolist() == [[3, 20], [-1, -1], [4, 21], [-1, -1], [0, 22], [-1, -1], [7, 23], [-1, -1], [8, 21], [-1, -1], [-1, -1], [-1, -1]]
    c = s["counters"]
    assert (c["samples"], c["projected"], c["trapped"], c["advanced"], c["reached"], c["unsettled"]) == (6, 5, 1, 2, 1, 1)
    assert (c["connect_reached"], c["connect_added"], c["connect_nothing"], c["vertices"], c["edges"]) == (1, 1, 1, 4, 5)
    assert s["next_index"] == 16 and s0["next_index"] == 10
    # the smallest gap, strict: sample 2 (0.25) wins over sample 4 (the same gap, later); A is the start side
    assert (s["best_gap"], s["best_a"], s["best_b"]) == (0.25, 21, 8)
    s2, _, _ = R.commit(s, 24, False, use, pa, idx_a, pb, idx_b)
    assert (s2["best_gap"], s2["best_a"], s2["best_b"]) == (0.25, 21, 8)  # an equal gap later does not replace it
    pb["gap"][0] = 0.125
    s3, _, _ = R.commit(s, 24, False, use, pa, idx_a, pb, idx_b)
    assert (s3["best_gap"], s3["best_a"], s3["best_b"]) == (0.125, 27, 24)  # A is the goal side: the pair is stored start side first


def test_full_and_the_solution_test(ccmp_built):
    assert not R.full(10, 5, 20) and R.full(11, 5, 20)
    s = R.new_state([0, 3], [5, 6])
    labels = np.array([0, 1, 2, 3, 4, 3, 0], dtype=np.int32)
    got = R.connected(labels, s)
    assert (got["status"], got["solved_start"], got["solved_goal"]) == (R.SOLVED, 0, 6)  # start-major: (0, 6) comes before (3, 5)
    assert R.connected(labels[:6], s)["solved_start"] == 3  # vertex 6 is outside: never a match
    assert R.connected(np.arange(7, dtype=np.int32), s)["status"] == R.OPEN
    assert R.connected(np.arange(7, dtype=np.int32), got) == got  # SOLVED stays


def test_the_synthetic_cases_reach_every_outcome(ccmp_built):
    cases = R.synthetic_cases()
    states, ns, ok, to, d = R.stack_cases(cases)
    seen = set()
    for (name, rows, n, k, dd, rng) in cases:
        seen.add(R.extend(rows, n, rows.shape[0], k, dd, rng)[0])
    assert seen == {R.TRAPPED, R.ADVANCED, R.REACHED, R.UNSETTLED}
    assert {c[2] for c in cases} >= {0, 1, 2, 3, 4, 5} and {c[3] for c in cases} == {0, 1, 2}
