"""What the batches of tests/jerk_cases.py contain, asserted on the restatement alone: no library, no device.  A batch that stopped holding
what it was built for would let the GPU tests pass for the wrong reason."""
import numpy as np
import pytest

import jerk_cases as jc
from jerk_cases import CASE_TILE, EMPTY, FULL, NAMES, NONFINITE, OK, POINT, UNORDERED, WINDOW


@pytest.fixture(scope="module")
def ref():
    return jc.reference()


def test_the_ragged_batch_holds_every_status_and_every_tile_edge(ref):
    case, want = ref["case"], ref[0]
    st = dict(zip(NAMES, want["status"].tolist()))
    W = dict(zip(NAMES, want["window"].tolist()))
    passes = dict(zip(NAMES, want["passes"].tolist()))
    M = dict(zip(NAMES, np.diff(want["tick_first"]).tolist()))
    assert (st["empty"], st["point"], st["non_finite"], st["unordered"]) == (EMPTY, POINT, NONFINITE, UNORDERED)
    assert (M["empty"], M["point"], M["non_finite"], M["unordered"]) == (0, 1, 0, 0) and W["point"] == 0
    # n = 1: every qd zero, M = 1 + W
    assert st["one_interval"] == OK and M["one_interval"] == 1 + W["one_interval"] and want["traces"][NAMES.index("one_interval")] == [(1, 0.0)]
    # the window is longer than the motion, and max_window does not reach the limit
    assert st["short"] == WINDOW and W["short"] == case["max_window"] and M["short"] - W["short"] == 3 < W["short"] and want["peak"][NAMES.index("short"), jc.JERK] > 1.0
    assert (M["m_less"], M["m_tile"], M["m_more"], M["m_two"]) == (CASE_TILE - 1, CASE_TILE, CASE_TILE + 1, 2 * CASE_TILE + 1)
    pf = case["path_first"]
    assert [int(pf[NAMES.index(n) + 1] - pf[NAMES.index(n)]) for n in ("m_less", "m_tile", "m_more", "m_two")] == [3, 17, 70, 17]
    # FULL before any measurement, and FULL only after the window grew
    assert st["full"] == FULL and passes["full"] == 0 and W["full"] == 1 and M["full"] == 0
    assert st["full_after"] == FULL and passes["full_after"] == 1 and W["full_after"] > 1 and M["full_after"] == 0
    assert ref[1]["status"][NAMES.index("full_after")] == WINDOW and np.diff(ref[1]["tick_first"])[NAMES.index("full_after")] == case["max_ticks"]
    # paths of one launch that end on different windows after different numbers of passes
    done = [(W[n], passes[n]) for n in NAMES if st[n] == OK]
    assert len({w for w, _ in done}) >= 4 and len({p for _, p in done}) >= 3, done
    assert max(W[n] for n in NAMES if st[n] == OK) == case["max_window"]  # an OK at max_window itself
    # windows wider than a tile exist for the small tile lengths the tests force
    assert max(W.values()) > 2


def test_the_fixed_windows_differ_and_one_is_no_power_of_two(ref):
    assert jc.FIXED_WINDOWS == (1, 2, 3, ref["case"]["max_window"])
    for w in jc.FIXED_WINDOWS:
        want = ref[w]
        ran = np.isin(want["status"], (OK, WINDOW))
        assert ran.sum() >= 9 and (want["window"][ran] == w).all() and (want["passes"] == 0).all()
        assert {OK, WINDOW} <= set(want["status"].tolist())


def test_the_scene_case_cuts_its_corner(ref):
    want = ref["scene"]["want"]
    assert want["status"].tolist() == [OK] and want["window"][0] > 1 and want["passes"][0] >= 1
    assert want["counts"][0][0] > 0 and want["counts"][0][1] > 0  # ticks off the manifold's tolerance and below the margin: the audit has something to say
    assert 0 < want["peak_tick"][0][jc.CLEARANCE] < want["ticks"] - 1 and np.isfinite(want["clearance"]).all()


def test_next_window_grows_whatever_it_is_given():
    for W in (1, 2, 5, 63):
        for P in (0.0, 0.5, 1.0, 1.0 + 2.0 ** -52, 1.5, 7.3, 1e300, float("inf")):
            for aim in (0.5, 0.95, 1.0):
                nxt = jc.next_window_py(W, P, aim, 64)
                assert W < nxt <= 64
    assert jc.next_window_py(3, 0.9, 0.95, 64) == 4 and jc.next_window_py(3, 0.9, 0.95, 64, plus_one=False) == 3
    assert jc.next_window_py(1, 3.43, 0.95, 64) == 4 and jc.next_window_py(4, 1.3, 0.95, 64) == 6 and jc.next_window_py(5, 100.0, 0.95, 64) == 64
