"""What the batch of tests/fit_cases.py is meant to contain, asserted on the restatement alone (no library, no device): the GPU test compares
bits on this batch, and a batch that has lost an edge compares nothing there."""
import numpy as np
import pytest

import fit_cases as fc
import setpoint_cases as sc
from fit_cases import EMPTY, FITTED, FULL, NAMES, NONFINITE, PASSES, POINT, UNORDERED


@pytest.fixture(scope="module")
def ref():
    return fc.reference()


def _path(ref, name):
    case, want = ref["case"], ref["want"]
    f = NAMES.index(name)
    a, b = int(case["path_first"][f]), int(case["path_first"][f + 1])
    return dict(f=f, rows=case["rows"][a:b], time=case["time"][a:b], out=want["time"][a:b], status=int(want["status"][f]), passes=int(want["passes"][f]),
                peak=want["peak"][f], trace=want["traces"][f], factor=want["factor"][a:b])


def test_every_status_is_there(ref):
    st = {n: _path(ref, n)["status"] for n in NAMES}
    assert (st["empty"], st["point"], st["non_finite"], st["unordered"], st["full_after"]) == (EMPTY, POINT, NONFINITE, UNORDERED, FULL)
    assert all(st[n] == FITTED for n in ("two", "three", "seventeen", "repeats", "within", "slow_start"))
    assert PASSES in st.values()
    # the bad paths stand between the others
    order = [st[n] in (FITTED, PASSES, FULL) for n in NAMES]
    assert order[0] and order[-1] and not all(order[1:-1])
    assert [len(_path(ref, n)["rows"]) for n in ("two", "three", "seventeen", "seventy")] == [2, 3, 17, 70]


def test_two_rows_have_one_bracket(ref):
    p = _path(ref, "two")
    assert p["trace"] and all(set(k) == {1} for _, _, k in p["trace"])


def test_repeated_rows_keep_intervals_of_no_width(ref):
    p = _path(ref, "repeats")
    h_in, h_out = np.diff(p["time"]), np.diff(p["out"])
    assert (h_in == 0.0).sum() == 2 and h_in[-1] == 0.0 and h_in[1] == 0.0
    assert np.array_equal(h_in == 0.0, h_out == 0.0) and p["passes"] >= 1
    assert p["factor"][2] == 1.0 and p["factor"][-1] == 1.0
    # a tick interval spans the interval of no width: it owns an acceleration, and no tick
    S, A, k = p["trace"][0]
    assert S[2] == 0.0 and A[2] > 0.0 and 2 not in k


def test_the_tight_path_feeds_one_acceleration_to_many_intervals(ref):
    p = _path(ref, "tight")
    S, A, k = p["trace"][0]
    assert max(np.diff(k)) >= 2  # a tick interval spanning three row intervals or more
    empty = [i for i in range(1, len(S)) if i not in k]
    assert len(empty) >= 3 and all(S[i] == 0.0 for i in empty) and any(A[i] > 0.0 for i in empty)
    assert k[0] == k[1] > 1  # where k_0 = k_1 and k_0 = 1 part


def test_within_the_limits_means_untouched(ref):
    p = _path(ref, "within")
    assert p["status"] == FITTED and p["passes"] == 0 and sc.same_f64(p["out"], p["time"]) and (p["factor"] == 1.0).all()
    assert 0.0 < p["peak"][0] <= 1.0 and 0.0 < p["peak"][1] <= 1.0


def test_full_arises_after_the_first_dilation(ref):
    p = _path(ref, "full_after")
    assert p["status"] == FULL and p["passes"] == 1 and len(p["trace"]) == 1
    assert sc.status_py(p["rows"], p["time"], fc.BATCH_PERIOD, fc.BATCH_MAX_TICKS)[0] == sc.OK
    assert sc.status_py(p["rows"], p["out"], fc.BATCH_PERIOD, fc.BATCH_MAX_TICKS)[0] == FULL
    assert p["peak"][1] > 1.0  # the last measurement made, not zero


def test_paths_finish_in_different_passes(ref):
    done = {n: _path(ref, n)["passes"] for n in NAMES if _path(ref, n)["status"] == FITTED}
    assert len(set(done.values())) >= 3 and min(done.values()) == 0, done
    p = _path(ref, "seventy")
    assert p["status"] == PASSES and p["passes"] == fc.BATCH_MAX_PASSES


def test_boundaries_fall_inside_blocks_and_wavefronts(ref):
    """sixteen lanes per tick interval: four intervals per wavefront, sixteen per block of 256"""
    counts = [len(p[0][2]) - 1 if p else 0 for p in ref["want"]["traces"]]  # tick intervals of the first measurement
    first = np.cumsum([0] + counts)
    assert first[-1] > 16 * 8
    inner = [int(v) for v in first[1:-1]]
    assert any(v % 16 for v in inner) and any(v % 4 for v in inner)


def test_the_reordered_batch_is_the_same_paths(ref):
    case = ref["case"]
    other, order = fc.reordered(case)
    pf, qf = case["path_first"], other["path_first"]
    assert len(qf) == len(pf) + 1 and sorted(order) == list(range(len(pf) - 1))
    for i, f in enumerate(order):
        assert np.array_equal(other["rows"][qf[i + 1]:qf[i + 2]], case["rows"][pf[f]:pf[f + 1]], equal_nan=True)
        assert np.array_equal(other["time"][qf[i + 1]:qf[i + 2]], case["time"][pf[f]:pf[f + 1]], equal_nan=True)
    assert qf[1] == 3 and [int(qf[i + 1]) for i, f in enumerate(order)] != [int(pf[f]) for f in order]
