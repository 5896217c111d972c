"""tests/plan_cases.py checked on its own: the restatement of the planner loop's scalar rule against hand-worked values, and its carry
rule against the logic of `Roadmap.closest_from_goal` (run on a stand-in store that returns prepared `closest` arrays: no device)."""
import numpy as np
import pytest

import plan_cases as P


def _fake_roadmap(idx, dist, fd):
    from closed_chain_motion_planner_amd import Roadmap

    rm = Roadmap.__new__(Roadmap)
    rm._h = None
    rm.read = lambda first, count, host=False: (np.zeros((1, 14)), np.zeros((1, 8)))
    rm.closest = lambda froms, pose: (np.asarray(idx, dtype=np.int32), np.asarray(dist, dtype=np.float64), np.asarray(fd, dtype=np.float64))
    return rm


@pytest.mark.parametrize("seed", range(40))
def test_carry_equals_the_mirrors_closest_from_goal(seed, ccmp_built):
    rng = np.random.default_rng(seed)
    F, size = int(rng.integers(1, 9)), 50
    froms = rng.integers(0, size, F).tolist()
    fd = rng.uniform(0.0, 2.0, F)
    dist = np.where(rng.random(F) < 0.5, fd * rng.uniform(0.2, 1.0, F), fd)  # the best of a component is never farther than its from
    idx = np.where(rng.random(F) < 0.2, -1, rng.integers(0, size, F)).astype(np.int32)
    dist = np.where(idx < 0, np.inf, dist)
    if seed % 5 == 0:
        fd[rng.integers(0, F)] = np.nan
    want = _fake_roadmap(idx, dist, fd).closest_from_goal(froms, 0)
    got = P.carry(froms, idx, dist, fd, size)
    assert got[0] == want[0] and np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes()


def test_carry_last_from_wins_even_when_it_is_worse():
    # from 3's component holds a vertex at 0.2; from 7 is at 0.9 and alone: closest is 7, closestVal stays 0.2 (the reference's behaviour)
    assert P.carry([3, 7], [5, 7], [0.2, 0.9], [0.5, 0.9], 10) == (7, 0.2)
    assert P.carry([7, 3], [7, 5], [0.9, 0.2], [0.9, 0.5], 10) == (5, 0.2)
    assert P.carry([], [], [], [], 10) == (-1, float("inf"))
    assert P.carry([12], [1], [0.1], [0.3], 10) == (-1, float("inf"))  # a from outside the store is skipped


def test_gate_full_prefix_connected_push():
    assert not P.gate(7, 4) and P.gate(8, 4)
    assert not P.full(10, 2, 5, 10 + 12 + 11) and P.full(10, 2, 5, 10 + 12 + 10)
    assert P.prefix([1] * 9, [1] * 9)[1] == 9 and P.prefix([0] + [1] * 8, [1] * 9)[1] == 0
    ok, n = P.prefix([1, 1, 1, 1, 0, 1, 1, 1, 1], [1] * 9)
    assert n == 4 and ok.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 0]
    s = P.new_state(np.zeros(8), 1.0)
    s["starts"], s["goals"] = [0, 4], [1, 5]
    lab = np.array([0, 1, 2, 3, 4, 4], dtype=np.int32)
    got = P.connected(lab, s)
    assert (got["status"], got["solved_start"], got["solved_goal"]) == (P.SOLVED, 4, 5) and s["status"] == P.OPEN
    for v in range(9):
        P.push(s, 1, 10 + v)
    assert len(s["goals"]) == 8 and s["counters"]["goal_pushes"] == 6 and s["counters"]["push_refused"] == 3
    P.push(s, 0, -1)
    assert s["starts"] == [0, 4]


def test_check_updates_only_what_fires():
    s = P.new_state(np.zeros(8), 1.0)
    s["starts"], s["goals"], s["size_at_check"] = [0], [1], 2
    a, b = ([2], [0.5], [1.0]), ([1], [1.0], [1.0])
    same, trig = P.check(s, 5, a, b)
    assert trig == [0, 0, 0, -1] and P.state_bits(same) == P.state_bits(s)
    got, trig = P.check(s, 6, a, b, np.arange(48.0).reshape(6, 8))
    assert trig == [1, 1, 0, 2] and got["nearest"] == 2 and got["prev_from_goal"] == 0.5 and got["prev_from_start"] == 1.0 and got["sprevious"] == 1
    assert got["size_at_check"] == 6 and got["next_index"] == 11 and got["nearest_pose"] == list(np.arange(16.0, 24.0)) and got["counters"]["checks"] == 1
