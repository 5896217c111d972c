"""ccmp_plan_check_ref / ccmp_plan_prefix_ref / ccmp_plan_connected_ref (csrc/ccmp_plan.h compiled for the host: the kernels' text)
against the plain-Python restatement of tests/plan_cases.py, bit for bit, on the rule's edges — and the three mutations of the rule
(`<` to `<=`, the gate's 3 to 4, the first pair to the last), each caught by a named case.  No device."""
import copy

import numpy as np
import pytest

import plan_cases as P

pytestmark = pytest.mark.usefixtures("ccmp_built")
POSES = np.arange(40 * 8, dtype=np.float64).reshape(40, 8) / 7.0


def _state(starts=(0,), goals=(1,), prev_goal=1.0, prev_start=1.0, size_at_check=2, next_index=5):
    s = P.new_state(np.linspace(0.1, 0.8, 8), 1.0, next_index)
    s.update(starts=list(starts), goals=list(goals), prev_from_goal=prev_goal, prev_from_start=prev_start, size_at_check=size_at_check, nearest=starts[0] if starts else -1,
             sprevious=goals[0] if goals else -1)
    return s


def _both(state, size, a, b, poses=POSES):
    from closed_chain_motion_planner_amd import plan_check_ref

    sp = poses[:size]
    want = P.check(state, size, a, b, sp)
    got = plan_check_ref(state, size, a, b, sp)
    assert got[1] == want[1] and P.state_bits(got[0]) == P.state_bits(want[0]), (got, want)
    return got


def _arr(idx, dist, fd):
    return np.array(idx, dtype=np.int32), np.array(dist, dtype=np.float64), np.array(fd, dtype=np.float64)


QUIET = _arr([1], [1.0], [1.0])  # a side that cannot fire against prev = 1.0


def test_gate_at_three_and_four():
    a = _arr([2], [0.5], [1.0])
    s = _state(size_at_check=10)
    _, trig = _both(s, 13, a, QUIET)
    assert trig[0] == 0  # size == size_at_check + 3: no check
    got, trig = _both(s, 14, a, QUIET)
    assert trig[:2] == [1, 1] and got["size_at_check"] == 14 and got["next_index"] == 16


def test_threshold_is_strict_to_the_ulp():
    prev = 0.7368421052631579
    edge = prev - 0.1  # as the rule computes it
    s = _state(prev_goal=prev, prev_start=prev)
    got, trig = _both(s, 10, _arr([2], [edge], [1.0]), _arr([3], [edge], [1.0]))
    assert trig[1:3] == [0, 0] and got["prev_from_goal"] == prev and got["nearest"] == 0  # exactly at prev - 0.1: no trigger
    below = np.nextafter(edge, -np.inf)
    got, trig = _both(s, 10, _arr([2], [below], [1.0]), _arr([3], [below], [1.0]))
    assert trig[1:] == [1, 1, 2] and got["prev_from_goal"] == below and got["prev_from_start"] == below and got["sprevious"] == 3


@pytest.mark.parametrize("d", [np.nan, np.inf], ids=["nan", "inf"])
def test_nan_and_inf_distances_never_fire(d):
    got, trig = _both(_state(), 10, _arr([2], [d], [d]), _arr([3], [d], [d]))
    assert trig == [1, 0, 0, -1] and got["prev_from_goal"] == 1.0 and got["counters"]["checks"] == 1


def test_idx_minus_one_falls_back_to_the_from():
    got, trig = _both(_state(starts=(4,)), 10, _arr([-1], [np.inf], [0.3]), QUIET)
    assert trig == [1, 1, 0, 4] and got["nearest"] == 4 and got["prev_from_goal"] == 0.3
    assert got["nearest_pose"] == POSES[4].tolist()


def test_index_outside_the_store_is_no_candidate():
    got, trig = _both(_state(starts=(4,)), 10, _arr([25], [0.1], [0.3]), QUIET)
    assert trig[3] == 4 and got["prev_from_goal"] == 0.3
    _, trig = _both(_state(starts=(30,)), 10, _arr([2], [0.1], [0.3]), QUIET)
    assert trig[1] == 0


@pytest.mark.parametrize("F", [1, 2, 8])
def test_carry_across_froms(F):
    rng = np.random.default_rng(F)
    starts = list(range(F))
    fd = rng.uniform(0.3, 0.8, F)
    a = _arr(rng.integers(10, 20, F), fd * 0.5, fd)
    got, trig = _both(_state(starts=starts, goals=(9,)), 30, a, _arr([9], [1.0], [1.0]))
    assert trig[1] == 1 and got["prev_from_goal"] == P.carry(starts, *a, 30)[1]


def test_a_later_from_that_worsens_closest_still_wins():
    # from 0's component reaches 0.2 at vertex 5; from 1 stands alone at 0.6: closest is 1 ("last from wins"), its value 0.2
    got, trig = _both(_state(starts=(0, 1), goals=(9,)), 30, _arr([5, 1], [0.2, 0.6], [0.5, 0.6]), _arr([9], [1.0], [1.0]))
    assert trig[3] == 1 and got["nearest"] == 1 and got["prev_from_goal"] == 0.2


def test_lists_at_one_and_at_the_cap():
    fire = _arr([20] * 8, [0.1] * 8, [0.9] * 8)
    one = tuple(a[:1] for a in fire)
    got, trig = _both(_state(starts=(0,), goals=(1,)), 30, one, one)
    assert trig[1:3] == [1, 1] and got["counters"]["push_refused"] == 0
    s = _state(starts=tuple(range(8)), goals=tuple(range(8, 16)))
    got, trig = _both(s, 30, fire, fire)
    assert trig[1:3] == [1, 1] and got["counters"]["push_refused"] == 2  # both sides fire, neither may push: refused and counted


def test_no_goals_nothing_fires():
    from closed_chain_motion_planner_amd import plan_check_ref

    s = _state(goals=())
    got, trig = plan_check_ref(s, 10, _arr([2], [0.1], [0.3]), None, POSES[:10])
    want = P.check(s, 10, _arr([2], [0.1], [0.3]), ([], [], []))
    assert trig == want[1] == [1, 0, 0, -1] and P.state_bits(got) == P.state_bits(want[0]) and got["size_at_check"] == 10


PREFIXES = {0: [0, 1, 1, 1, 1, 1, 1, 1, 1], 1: [1, 0, 1, 1, 1, 1, 1, 1, 1], 4: [1, 1, 1, 1, 0, 1, 1, 1, 1], 9: [1] * 9}


@pytest.mark.parametrize("n", sorted(PREFIXES))
@pytest.mark.parametrize("via", ["valid", "ik_ok"])
def test_prefix_lengths(n, via):
    from closed_chain_motion_planner_amd import plan_prefix_ref

    flags, ones = np.array(PREFIXES[n], dtype=np.uint8), np.ones(9, dtype=np.uint8)
    args = (flags, ones) if via == "valid" else (ones, flags)
    got, want = plan_prefix_ref(*args), P.prefix(*args)
    assert got[1] == want[1] == n and got[0].tolist() == want[0].tolist()
    assert not got[0][n:].any()  # a valid pose after the first invalid one is not kept


def test_prefix_needs_both_flags():
    from closed_chain_motion_planner_amd import plan_prefix_ref

    v, k = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1], dtype=np.uint8), np.array([1, 0, 1, 1, 1, 1, 1, 1, 1], dtype=np.uint8)
    assert plan_prefix_ref(v, k)[1] == P.prefix(v, k)[1] == 1


def _connected(labels, s):
    from closed_chain_motion_planner_amd import plan_connected_ref

    lab = np.array(labels, dtype=np.int32)
    got, want = plan_connected_ref(lab, s), P.connected(lab, s)
    assert P.state_bits(got) == P.state_bits(want)
    return got


def test_connected_only_the_last_pair():
    s = _state(starts=(0, 1, 2), goals=(3, 4))
    got = _connected([0, 1, 2, 3, 2], s)
    assert (got["status"], got["solved_start"], got["solved_goal"]) == (P.SOLVED, 2, 4)
    assert _connected([0, 1, 2, 3, 4], s)["status"] == P.OPEN


def test_connected_first_pair_in_start_major_order_wins():
    s = _state(starts=(0, 1), goals=(2, 3))
    got = _connected([0, 0, 0, 0], s)  # all four pairs match
    assert (got["solved_start"], got["solved_goal"]) == (0, 2)
    got = _connected([0, 1, 1, 0], s)  # (0, 3) and (1, 2): start-major order puts (0, 3) first
    assert (got["solved_start"], got["solved_goal"]) == (0, 3)
    assert _connected([0, 0], s)["status"] == P.OPEN  # lists that point outside the labels never match


# ---- the mutations: each variant of the restatement must DIFFER from the library on the named case ------------------------------------
def _mutant_check(state, size, a, b, strict=True, gate_add=3):
    s = copy.deepcopy(state)
    if not size > s["size_at_check"] + gate_add:
        return s, [0, 0, 0, -1]
    c, d = P.carry(s["starts"], *a, size)
    fired = d < s["prev_from_goal"] - 0.1 if strict else d <= s["prev_from_goal"] - 0.1
    return s, [1, int(fired), 0, c if fired else -1]


def test_mutation_less_equal_is_caught_by_the_ulp_case():
    from closed_chain_motion_planner_amd import plan_check_ref

    prev = 0.7368421052631579
    s, a = _state(prev_goal=prev), _arr([2], [prev - 0.1], [1.0])
    assert plan_check_ref(s, 10, a, QUIET)[1][1] == 0 and _mutant_check(s, 10, a, QUIET, strict=False)[1][1] == 1


def test_mutation_gate_plus_four_is_caught_by_the_gate_case():
    from closed_chain_motion_planner_amd import plan_check_ref

    s, a = _state(size_at_check=10), _arr([2], [0.5], [1.0])
    assert plan_check_ref(s, 14, a, QUIET)[1][0] == 1 and _mutant_check(s, 14, a, QUIET, gate_add=4)[1][0] == 0


def test_mutation_last_pair_is_caught_by_the_several_pairs_case():
    from closed_chain_motion_planner_amd import plan_connected_ref

    s = _state(starts=(0, 1), goals=(2, 3))
    got = plan_connected_ref(np.zeros(4, dtype=np.int32), s)
    last = [(a, b) for a in s["starts"] for b in s["goals"]][-1]
    assert (got["solved_start"], got["solved_goal"]) == (0, 2) != last
