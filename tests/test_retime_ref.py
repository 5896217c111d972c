"""The host-only forms of the resample and time-stamp rule (ccmp_path_timestamps_ref, ccmp_arc_bracket_ref, ccmp_resample_targets_ref: the
text of csrc/ccmp_retime.h compiled for the host, no device) bit for bit against the plain-Python restatement of tests/retime_cases.py, on
every batch of that module and on the reference's two recorded path files; then the properties the rule guarantees by construction, and
every argument error.

Mutation check (each made in the sources, the library rebuilt, this file run; the unmutated sources turn every test green again):
  * csrc/ccmp_dense.h (arc_bracket), the bracket's bisection with `s[mid] > h` instead of `>=`
        -> test_arc_bracket_matches_the_linear_scan (the targets that ARE a dense arc) and test_argument_errors (its two spot values) red
  * csrc/ccmp_retime.h, h_j as (j * T) / (N - 1) instead of (j / (N - 1)) * T
        -> test_targets_match red
  * csrc/ccmp_retime.cpp, the envelope's loop started at +inf instead of at its k = i term x_i
        -> every test_timestamps_match case and test_properties (y <= x) red
"""
import ctypes as C

import numpy as np
import pytest

import retime_cases as rc
from conftest import load_path_rows
from retime_cases import EMPTY, NONFINITE, OK, PANDA_AMAX, PANDA_VMAX

EINVAL, ENODEV = -1, -5
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def ref(ccmp_built):
    return rc.reference(1)


def _batches(ref):
    rows, first = ref["ragged"]["rows"]
    yield "ragged", rows, first
    for name in ("wide", "long"):
        yield name, ref[name]["want"]["joints"], ref[name]["want"]["path_first"]
    yield "fallback", ref["fallback"]["case"]["want"]["joints"], ref["fallback"]["case"]["want"]["path_first"]
    yield ("still",) + rc.still_rows()
    for obj in ("Wine_Bottle", "dumbbell"):
        g = load_path_rows(obj)
        yield "golden-" + obj, g, np.array([0, len(g)], dtype=np.int32)
    # an empty path in front, between and behind, and a path with a NaN and one with an infinity
    rows = np.vstack([rows[first[4]:first[5]], rows[first[3]:first[4]], rows[first[4]:first[5]], rows[first[2]:first[3]]])
    rows[17 + 1, 3], rows[17 + 3 + 5, 0] = np.nan, np.inf
    yield "statuses", rows, np.array([0, 0, 17, 20, 20, 37, 39, 39], dtype=np.int32)


@pytest.mark.parametrize("name", ["ragged", "wide", "long", "fallback", "still", "golden-Wine_Bottle", "golden-dumbbell", "statuses"])
@pytest.mark.parametrize("beta", [0.5, 0.2])
def test_timestamps_match(ref, name, beta):
    from closed_chain_motion_planner_amd import timestamps_ref

    rows, first = next((r, f) for n, r, f in _batches(ref) if n == name)
    want = rc.timestamps_py(rows, first, PANDA_VMAX, PANDA_AMAX, beta)
    got = timestamps_ref(rows, first, PANDA_VMAX, PANDA_AMAX, beta)  # (its outputs start as NaN: rows the rule does not write stay so)
    rc.same_stamps(got, want, (name, beta))
    if name == "statuses":
        assert want["status"].tolist() == [EMPTY, OK, NONFINITE, EMPTY, NONFINITE, OK, EMPTY] and np.isnan(got["time"][17:20]).all()
        assert np.isnan(got["duration"][2]) and got["duration"][0] == 0.0


def test_properties(ref):
    """what the rule guarantees by construction, with the margins of its own roundings.
    Slope: if k attains y_i = fl(x_k + fl(g m)), m = |i - k|, then y_{i+1} <= fl(x_k + fl(g (m + 1))).  The four roundings are each RELATIVE
    TO THEIR TERM, which is up to m times g, not to g: with u = 2^-53, y_{i+1} - y_i <= g + 2u (x_k + g m) + 2u (x_k + g (m + 1)) = g (1 + 2u) +
    4u min(y_i, y_{i+1}).  The margin g (1 + 4 * 2^-52) alone holds only while the attaining k is next to i; it missed the rounding of the
    product g m and of the sum at large m (on the 65-row path y = g m up to m = 32: 6 ulp of g), so the assertion adds 4 * 2^-52 min(y_i, y_{i+1})
    — twice the derived 4u, the same factor of slack as the margin on g — and nothing else.
    Speed: |d| / dt = |d| (sqrt(y_i) + sqrt(y_{i+1})) / 2 against vmax = |d| V carries the quotient vmax / |d|, the square, two roots, the sum,
    the quotient 2 / sum and the test's own division and product: 8 roundings of at most one ulp, some entering twice: 16 * 2^-52 holds"""
    from closed_chain_motion_planner_amd import timestamps_ref

    moved = 0
    for name, rows, first in _batches(ref):
        got = timestamps_ref(rows, first, PANDA_VMAX, PANDA_AMAX, 0.5)
        want = rc.timestamps_py(rows, first, PANDA_VMAX, PANDA_AMAX, 0.5)
        for f in range(len(first) - 1):
            a, b = int(first[f]), int(first[f + 1])
            if got["status"][f] != OK or b - a < 2:
                continue
            x, y, t, g = got["ceiling"][a:b], got["envelope"][a:b], got["time"][a:b], want["g"][f]
            assert (y <= x).all(), (name, f)
            if np.isfinite(g) and b - a >= 3:
                assert (np.abs(np.diff(y)) <= g * (1 + 4 * ULP) + 4 * ULP * np.minimum(y[:-1], y[1:])).all(), (name, f, np.abs(np.diff(y)).max() / g - 1)
            d, dt = np.abs(np.diff(rows[a:b], axis=0)), np.diff(t)
            for i in range(b - a - 1):
                if d[i].any():
                    assert dt[i] > 0.0 and t[i + 1] > t[i], (name, f, i)  # times strictly increase wherever a row moved
                    assert (d[i] / dt[i] <= np.array(PANDA_VMAX) * (1 + 16 * ULP)).all(), (name, f, i, (d[i] / dt[i] / np.array(PANDA_VMAX)).max() - 1)
                    moved += 1
            assert t[0] == 0.0 and got["duration"][f] == t[-1]
    assert moved > 1000


def test_arc_bracket_matches_the_linear_scan(ref):
    from closed_chain_motion_planner_amd import arc_bracket_ref

    seen = {True: 0, False: 0}
    exact = 0
    for name in ("ragged", "wide", "long"):
        d = ref[name]["dense"]
        for f in range(len(d["path_first"]) - 1):
            s = d["arc"][d["path_first"][f]:d["path_first"][f + 1]]
            if len(s) < 2 or not s[-1] > 0.0:
                continue
            hs = [rc.target_py(j, 19, float(s[-1])) for j in range(1, 18)] + [float(v) for v in s if v > 0.0] + [float(np.nextafter(v, 0.0)) for v in s if v > 0.0]
            for h in hs:
                want = rc.bracket_py(s, h)
                assert arc_bracket_ref(s, h) == want, (name, f, h, arc_bracket_ref(s, h), want)
                assert s[want[0]] > s[want[0] - 1]  # a +0.0 step (a duplicated row) is never the bracket
                seen[want[2]] += 1
                exact += h in s
    assert seen[True] > 100 and seen[False] > 100 and exact > 100


def test_targets_match():
    from closed_chain_motion_planner_amd import resample_targets_ref

    for t in rc.targets() + [(float(T), n, 0.0, 65536) for T in (0.1, 1.7320508075688772, 3.0, 1e-310) for n in (3, 7, 65, 130, 1000)]:
        N, h = resample_targets_ref(*t)
        want = rc.targets_py(*t)
        assert N == want[0] and rc.same_f64(h, np.array(want[1])), (t, N, want[0])


def test_argument_errors(ref):
    from closed_chain_motion_planner_amd import CcmpError, arc_bracket_ref, resample_targets_ref, timestamps_ref
    from closed_chain_motion_planner_amd import _lib

    rows, first = ref["ragged"]["rows"]

    def refused(fn, *a, **k):
        with pytest.raises(CcmpError) as e:
            fn(*a, **k)
        assert e.value.code == EINVAL, (a, k)

    nan, inf = float("nan"), float("inf")
    for bad in (0.0, -1.0, nan, inf):  # a limit that is not finite and positive
        for which in (0, 13):
            v, a = list(PANDA_VMAX), list(PANDA_AMAX)
            v[which] = bad
            refused(timestamps_ref, rows, first, v, PANDA_AMAX)
            a[which] = bad
            refused(timestamps_ref, rows, first, PANDA_VMAX, a)
    for beta in (0.0, 1.0, -0.5, 1.5, nan):
        refused(timestamps_ref, rows, first, PANDA_VMAX, PANDA_AMAX, beta)
    for pf in ([-1, 3], [0, 3, 2], [0, len(rows) + 1]):  # negative, decreasing, beyond the rows
        refused(timestamps_ref, rows, np.array(pf, dtype=np.int32), PANDA_VMAX, PANDA_AMAX)
    empty = timestamps_ref(rows[:0], np.array([0], dtype=np.int32), PANDA_VMAX, PANDA_AMAX)  # F == 0
    assert len(empty["time"]) == 0 and len(empty["duration"]) == 0
    s = np.array([0.0, 0.5, 0.5, 1.0])
    for h in (0.0, -0.1, nan, 1.0000000000000002):
        refused(arc_bracket_ref, s, h)
    refused(arc_bracket_ref, s[:1], 0.1)
    assert arc_bracket_ref(s, 0.5) == (1, 1.0, False) and arc_bracket_ref(s, 0.75) == (3, 0.5, True)
    for t in ((1.0, 1, 0.25, 65536), (1.0, -2, 0.25, 65536), (1.0, 0, 0.0, 65536), (1.0, 0, -0.25, 65536), (1.0, 0, nan, 65536), (1.0, 5, 0.25, 1), (1.0, 0, 0.25, 0)):
        refused(resample_targets_ref, *t)
    # without a context: no device here -> CCMP_ENODEV, a device -> CCMP_EINVAL; either way before anything else is looked at
    L = _lib.lib()
    out = C.c_void_p(1)
    rc_null = L.ccmp_path_resample(None, None, None, None, C.byref(out), None)
    assert rc_null in (ENODEV, EINVAL) and not out.value
    assert L.ccmp_path_timestamps(None, None, None, 0, 0, None, None, 0.5, None, None, None, None, None, None) in (ENODEV, EINVAL)
    assert L.ccmp_path_timestamps_host(None, None, None, 0, 0, None, None, 0.5, None, None, None, None, None) in (ENODEV, EINVAL)
    o = _lib.CcmpResampleOpts()
    L.ccmp_resample_opts_default(None, C.byref(o))
    assert (o.count, o.spacing, o.max_rows) == (0, 0.0, 65536)
