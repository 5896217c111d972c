"""The batches of tests/test_gpu_retime.py contain what their tests are about — asserted here on the oracle alone, no device, so a seed or a
constant that stops producing the case fails on every machine and not only where the GPU suite runs.  The seeds of tests/retime_cases.py were
chosen here: every chain is traversable in both Jacobian modes, and in every batch but the fallback case at least 90 % of the interior output
rows are PROJECTED on the oracle — otherwise the GPU comparison could pass on fallbacks alone."""
import numpy as np
import pytest

import retime_cases as rc
from retime_cases import BROKEN, COPIED, EMPTY, FALLBACK, FULL, NONFINITE, OK, POINT


@pytest.fixture(scope="module", params=[0, 1], ids=["fd", "analytic"])
def ref(request):
    return rc.reference(request.param)


def test_ragged_batch_has_every_size(ref):
    r = ref["ragged"]
    assert r["case"]["pl"].tolist() == list(rc.RAGGED_LENS) and r["case"]["counts"] == (2, 3, 17, 64, 65)
    for count, want in r["want"].items():
        assert want["status"].tolist() == [EMPTY, POINT, OK, OK, OK, OK, OK]
        assert np.diff(want["path_first"]).tolist() == [0, 1] + [count] * 5
        assert (want["kind"][want["path_first"][:-1][1:]] == COPIED).all() and rc.interior_projected_share(want) >= 0.9
    rows, first = r["rows"]
    assert np.diff(first).tolist() == list(rc.RAGGED_SIZES) and np.isfinite(rows).all()
    # both layouts of the same waypoints: duplicated rows, the same arcs at the rows both have
    ref_rows, dis_rows = np.diff(r["dense"]["path_first"]), np.diff(r["distinct"]["path_first"])
    assert (ref_rows[2:] > dis_rows[2:]).all() and rc.same_f64(r["dense"]["length"], r["distinct"]["length"])


def test_wide_batch_has_every_status(ref):
    w = ref["wide"]
    case, want, dense = w["case"], w["want"], w["dense"]
    st = want["status"]
    assert len(st) == rc.WIDE_F == 70 and len(want["joints"]) > 16 * 4  # more paths than a 256-lane block holds rows, and more rows than four blocks hold
    assert (st[rc.WIDE_BROKEN], st[rc.WIDE_POINT], st[rc.WIDE_NONFINITE], st[rc.WIDE_FULL]) == (BROKEN, POINT, NONFINITE, FULL)
    assert sorted(np.flatnonzero(st != OK).tolist()) == sorted([rc.WIDE_BROKEN, rc.WIDE_POINT, rc.WIDE_NONFINITE, rc.WIDE_FULL])
    assert (dense["seg_ok"][rc.WIDE_BROKEN][dense["seg_first"][rc.WIDE_BROKEN] >= 0] == 0).any()
    assert (dense["seg_first"][rc.WIDE_NONFINITE] < 0).all() and np.isnan(dense["rows"][dense["path_first"][rc.WIDE_NONFINITE]]).any()
    assert dense["length"][rc.WIDE_POINT] == 0.0 and np.diff(dense["path_first"])[rc.WIDE_POINT] == 3
    n = np.diff(want["path_first"])
    assert n[rc.WIDE_POINT] == 1 and n[rc.WIDE_BROKEN] == n[rc.WIDE_NONFINITE] == n[rc.WIDE_FULL] == 0
    assert n.max() == case["max_rows"] and rc.count_py(float(dense["length"][rc.WIDE_FULL]), 0, case["spacing"]) > case["max_rows"]
    assert len(set(n[st == OK].tolist())) >= 4  # spacing mode: the row count follows the length
    assert rc.interior_projected_share(want) >= 0.9


def test_long_path_spans_three_chunks(ref):
    want = ref["long"]["want"]
    assert want["status"].tolist() == [OK] and len(want["joints"]) == 130 and (130 - 1) // 64 == 2 and (130 - 1) % 64 == 1
    assert rc.interior_projected_share(want) >= 0.9 and (np.diff(want["arc"]) > 0).all()


def test_fallback_case_falls_back_both_ways(ref):
    want = ref["fallback"]["case"]["want"]  # (the builder asserts the two `lower` outcomes)
    assert (want["kind"][1:-1] == FALLBACK).all() and want["kind"][[0, -1]].tolist() == [COPIED, COPIED]
    dense_rows = {r.tobytes() for r in rc.Restatement(ref["O"], ref["P"]).dense(ref["fallback"]["case"]["pj"], ref["fallback"]["case"]["pl"])["rows"]}
    assert all(r.tobytes() in dense_rows for r in want["joints"])  # every row is a dense row


def test_still_rows_make_infinite_ceilings():
    rows, first = rc.still_rows()
    want = rc.timestamps_py(rows, first, rc.PANDA_VMAX, rc.PANDA_AMAX)
    assert np.diff(first).tolist() == [5, 3, 2, 3, 3, 1] and (want["status"] == OK).all()
    assert want["g"][1] == rc.INF and want["g"][2] == rc.INF and np.isfinite(want["g"][0])
    assert np.isinf(want["ceiling"][first[1] + 1]) and np.isinf(want["envelope"][first[1] + 1])  # a a a: nothing bounds the middle row
    assert want["duration"][1] == 0.0 and want["duration"][2] == 0.0 and want["duration"][5] == 0.0 and want["duration"][0] > 0.0
    assert np.isfinite(want["time"]).all()


def test_targets_cover_the_arithmetic():
    got = [rc.targets_py(*t)[0] for t in rc.targets()]
    assert got == [2, 17, 65, 0, 9, 8, 9, 2, 2, 9, 0, 1, 1, 1, 0, 0, 4], got
