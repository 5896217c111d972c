"""Jerk-bounded setpoints on the host (ccmp_jerk_setpoints_ref, ccmp_jerk_next_window_ref: csrc/ccmp_jerk.h compiled for the host) against the
plain-Python restatement of tests/jerk_cases.py, bit for bit, and what the rule guarantees by construction, each with a margin derived
where it is used.  No device.

Mutations tried against the rule.  They are made in the RESTATEMENT (jerk_cases.jerk_py(..., mutate=...)), not in the library's sources:
test_mutations_are_caught asserts, for each, where the wrong rule stops agreeing with the library — the same comparison that
test_ref_matches_the_restatement makes with the right rule, so a library carrying the mutation would turn that case red:
  * "running": a sum carried from tick to tick          -> q and qd of "five" (W = 5) differ in their last bits
  * "divide_first": every term divided by W, then summed -> "three" under the fixed window 3 (under W = 2 halving is exact and nothing shows)
  * "left": the jerk attributed to the left tick          -> the jerk peak's tick of every measured path is one too small
  * "ends": the end ticks computed as means               -> tick 0 of "three" under the fixed window 3: fl(fl(r + r) + r) / 3 is not r
  * "no_plus_one": W + 1 dropped from the update          -> inside the search P > 1 and aim <= 1 make ceil(W P / aim) >= W + 1 by themselves
        (fl(W P) > W because W P - W >= W 2^-52 is at least a whole spacing at W, and dividing by aim <= 1 cannot lower it), so no path can
        tell; the update itself is compared through ccmp_jerk_next_window_ref at P <= 1, where only the W + 1 term makes it grow.
"""
import numpy as np
import pytest

import jerk_cases as jc
import setpoint_cases as sc
from conftest import load_path_rows
from jerk_cases import NAMES, OK, PANDA_AMAX, PANDA_JMAX, PANDA_VMAX, WINDOW

U = 2.0 ** -52  # twice the unit roundoff of a double: what one rounded operation can be off by, relative, with room to spare


@pytest.fixture(scope="module")
def ref(ccmp_built):
    return jc.reference()


def _lib_jerk(case, window=0, **over):
    from closed_chain_motion_planner_amd import jerk_setpoints_ref

    return jerk_setpoints_ref(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, case["jmax"], window=window, **dict(jc.options(case), **over))


@pytest.fixture(scope="module")
def got(ref):
    """the library's answers for the ragged batch, computed once: {window: result}"""
    return {w: _lib_jerk(ref["case"], w) for w in (0,) + jc.FIXED_WINDOWS}


def _paths(res):
    tf = res["tick_first"]
    return [(f, int(tf[f]), int(tf[f + 1])) for f in range(len(tf) - 1) if res["status"][f] in (OK, WINDOW)]


def test_ref_matches_the_restatement(ref, got):
    for w, res in got.items():
        jc.same_jerk(res, jc.host_part(ref[w]), "window %d" % w)
    scene = ref["scene"]
    jc.same_jerk(_lib_jerk(scene), jc.host_part(scene["want"]), "scene case")


def test_window_one_is_the_setpoints_rule_on_the_grid(ref, got):
    """window = 1: q and qd bit-identical to ccmp_setpoints_ref and M = N; tau identical except the last entry, fl(n period) against D"""
    from closed_chain_motion_planner_amd import setpoints_ref

    case, one = ref["case"], got[1]
    sp = setpoints_ref(case["rows"], case["path_first"], case["time"], PANDA_VMAX, PANDA_AMAX, period=case["period"], max_ticks=case["max_ticks"])
    assert np.array_equal(sp["tick_first"], one["tick_first"]) and len(_paths(one)) >= 9
    assert sc.same_f64(sp["q"], one["q"]) and sc.same_f64(sp["qd"], one["qd"])
    last = np.zeros(one["ticks"], dtype=bool)
    for f, a, b in _paths(one):
        last[b - 1] = True
        D = case["time"][case["path_first"][f + 1] - 1]
        assert sp["tau"][b - 1] == D and one["tau"][b - 1] == float(b - 1 - a) * case["period"] and one["tau"][b - 1] >= D
    assert sc.same_f64(sp["tau"][~last], one["tau"][~last])
    ok = np.isin(one["status"], (OK, WINDOW))
    assert np.array_equal(sp["status"][~ok], one["status"][~ok]) and (sp["status"][ok] == sc.OK).all()


def test_ends_are_copies_and_every_tick_lies_in_the_hull_of_its_window(ref, got):
    case = ref["case"]
    pf = case["path_first"]
    for w, res in got.items():
        base = got[1]
        for f, a, b in _paths(res):
            W, M = int(res["window"][f]), b - a
            r = case["rows"][pf[f]:pf[f + 1]]
            assert np.array_equal(sc.bits(res["q"][a]), sc.bits(r[0])) and np.array_equal(sc.bits(res["q"][b - 1]), sc.bits(r[-1]))
            zero = sc.bits(np.zeros(14))
            assert np.array_equal(sc.bits(res["qd"][a]), zero) and np.array_equal(sc.bits(res["qd"][b - 1]), zero) and sc.bits(res["tau"][a:a + 1])[0] == 0
            # the inputs are the path's W = 1 ticks, held at both ends
            xa, xb = int(base["tick_first"][f]), int(base["tick_first"][f + 1])
            n = xb - xa - 1
            assert M == n + W
            x = base["q"][xa:xb]
            for j in range(M):
                win = x[np.clip(np.arange(j - W + 1, j + 1), 0, n)]
                # W - 1 additions and one division, each rounded once: the mean is off by at most W 2^-53 times the largest partial sum / W,
                # and no partial sum exceeds W max|x|.  U = 2^-52 leaves a factor two to spare.
                margin = W * U * np.abs(win).max(axis=0)
                assert (res["q"][a + j] >= win.min(axis=0) - margin).all() and (res["q"][a + j] <= win.max(axis=0) + margin).all(), (w, f, j)


def _accel_peaks(res, f, a, b, period):
    """A_c in rad/s^2 of path f of a window-1 result: max_j |qd_{j+1}[c] - qd_j[c]| / period"""
    return np.abs(np.diff(res["qd"][a:b], axis=0)).max(axis=0) / period


def test_speed_and_acceleration_peaks_do_not_rise_and_the_jerk_bound_holds(ref, got):
    case = ref["case"]
    p, base = case["period"], got[1]
    jmax, amax = np.array(case["jmax"]), np.array(PANDA_AMAX)
    premise_met = 0
    for w, res in got.items():
        for f, a, b in _paths(res):
            if base["status"][f] not in (OK, WINDOW):
                continue  # (a path that is FULL at one window has no figures at it)
            W, M = int(res["window"][f]), b - a
            xa, xb = int(base["tick_first"][f]), int(base["tick_first"][f + 1])
            vmax_abs = np.abs(base["qd"][xa:xb]).max()
            # a tick width is a difference of two products fl(j period), each within half a spacing of j period <= M period: relative to
            # the period every width is within M 2^-52 of it; quotients and differences add a few roundings of their own
            rel = 1.0 + (2 * M + 8) * U
            # a filtered velocity is off by at most W 2^-53 max|v| (as the positions above); a difference of two by twice that
            dv = W * U * vmax_abs
            assert res["peak"][f, jc.SPEED] <= base["peak"][f, jc.SPEED] * rel + dv / min(PANDA_VMAX), (w, f)
            assert res["peak"][f, jc.ACC] <= base["peak"][f, jc.ACC] * rel + 2.0 * dv / (p * amax.min()), (w, f)
            # the bound: qd_{j+1} - qd_j = (v_{j+1} - v_{j+1-W}) / W telescopes, so a_{j+1} - a_j is a difference of two unfiltered
            # accelerations over W: at most 2 A_c / W, and the jerk 2 A_c / (W period); a second difference of three filtered
            # velocities carries four times their error, over period^2
            A = _accel_peaks(base, f, xa, xb, p)
            bound = (2.0 * A / (W * p * jmax)).max() * rel + 4.0 * dv / (p * p * jmax.min())
            assert res["peak"][f, jc.JERK] <= bound, (w, f, res["peak"][f, jc.JERK], bound)
            if w == 0:  # the search ends in OK whenever W* <= max_window, with that margin to spare
                at_max = (2.0 * A / (case["max_window"] * p * jmax)).max() * rel + 4.0 * case["max_window"] * U * vmax_abs / (p * p * jmax.min())
                if at_max <= 1.0:
                    premise_met += res["window"][f] > 1
                    assert res["status"][f] == OK and res["peak"][f, jc.JERK] <= 1.0, f
    assert premise_met >= 1  # (the batch holds a path whose window grew and whose W* is within max_window: the implication was put to use)


@pytest.mark.parametrize("obj", ["Wine_Bottle", "dumbbell"])
def test_recorded_paths_get_a_window_at_one_millisecond(ccmp_built, obj):
    """stamped by timestamps_ref (beta 0.5, the Panda's limits), 1 ms: the unfiltered jerk ratio exceeds 1, the chosen window passes within
    three growths; the figures are printed (profiles/jerk.md records them), not hard-coded"""
    from closed_chain_motion_planner_amd import jerk_setpoints_ref, timestamps_ref

    g = load_path_rows(obj)
    first = np.array([0, len(g)], dtype=np.int32)
    t = timestamps_ref(g, first, PANDA_VMAX, PANDA_AMAX, 0.5)["time"]
    plain = jerk_setpoints_ref(g, first, t, PANDA_VMAX, PANDA_AMAX, PANDA_JMAX, window=1)
    chosen = jerk_setpoints_ref(g, first, t, PANDA_VMAX, PANDA_AMAX, PANDA_JMAX)
    print("%s at 1 ms: window %d after %d passes, %d -> %d ticks, speed / acceleration / jerk ratios %s -> %s" % (
        obj, chosen["window"][0], chosen["passes"][0], plain["ticks"], chosen["ticks"], plain["peak"][0].tolist(), chosen["peak"][0].tolist()))
    assert plain["status"].tolist() == [WINDOW] and plain["peak"][0, jc.JERK] > 1.0
    assert chosen["status"].tolist() == [OK] and chosen["passes"][0] <= 3 and chosen["peak"][0, jc.JERK] <= 1.0 and chosen["window"][0] > 1
    assert chosen["ticks"] == plain["ticks"] + chosen["window"][0] - 1
    assert (chosen["peak"][0, :2] <= plain["peak"][0, :2] * (1.0 + 1e-9)).all()  # (the derived margin is the batch test's; this is a plausibility check)


def test_mutations_are_caught(ref):
    case = ref["case"]

    def agrees(name, m, window=0):
        one = jc.one_path(case, name)
        try:
            jc.same_jerk(_lib_jerk(one, window), jc.host_part(jc.jerk_py(one["rows"], one["path_first"], one["time"], PANDA_VMAX, PANDA_AMAX, one["jmax"], window=window,
                                                                         mutate=(m,), **jc.options(one))))
            return True
        except AssertionError:
            return False

    assert agrees("five", "") and agrees("three", "", 3)  # the comparison itself, with the right rule
    assert not agrees("five", "running") and not agrees("three", "running", 3)
    assert not agrees("three", "divide_first", 3) and agrees("three", "divide_first", 2)
    assert not agrees("five", "left") and not agrees("three", "left") and not agrees("stiff", "left")
    assert not agrees("three", "ends", 3) and agrees("three", "ends", 1)
    assert agrees("five", "no_plus_one") and agrees("stiff", "no_plus_one")  # unreachable inside the search (the module's docstring) ...


def test_next_window_is_the_rule_and_grows_unconditionally(ccmp_built):
    """... so the update is compared on its own, P <= 1 included: only the W + 1 term makes it grow there"""
    from closed_chain_motion_planner_amd import CcmpError, jerk_next_window_ref

    dropped = 0
    for W in (1, 2, 3, 5, 17, 63):
        for P in (0.0, 0.3, 0.9, 1.0, 1.0 + 2.0 ** -52, 1.35, 3.43, 5.74, 40.0, 1e308, float("inf")):
            for aim in (0.25, 0.95, 1.0):
                nxt = jerk_next_window_ref(W, P, aim, 64)
                assert nxt == jc.next_window_py(W, P, aim, 64) and W < nxt <= 64, (W, P, aim)
                dropped += nxt != jc.next_window_py(W, P, aim, 64, plus_one=False)
    assert dropped > 0
    for bad in ((0, 2.0, 0.95, 64), (64, 2.0, 0.95, 64), (1, float("nan"), 0.95, 64), (1, 2.0, 0.0, 64), (1, 2.0, 1.5, 64), (1, 2.0, 0.95, 257)):
        with pytest.raises(CcmpError):
            jerk_next_window_ref(*bad)


def test_a_single_path_answers_as_it_does_in_the_batch(ref, got):
    """a path's answer does not depend on its batch neighbours"""
    case, res = ref["case"], got[0]
    for name in ("stiff", "m_more", "full_after", "short"):
        f = NAMES.index(name)
        alone = _lib_jerk(jc.one_path(case, name))
        a, b = int(res["tick_first"][f]), int(res["tick_first"][f + 1])
        assert (alone["status"][0], alone["window"][0], alone["passes"][0]) == (res["status"][f], res["window"][f], res["passes"][f]), name
        assert sc.same_f64(alone["q"], res["q"][a:b]) and sc.same_f64(alone["qd"], res["qd"][a:b]) and sc.same_f64(alone["peak"][0], res["peak"][f]), name
