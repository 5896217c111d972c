"""Dense solution paths without a device: the joining rule reproduces the reference's recorded <obj>_path.txt as a whole on the det
oracle, and the host-only forms of the rule (ccmp_dense_layout_ref, ccmp_dense_arc_ref) equal the plain-Python restatement of
tests/dense_path_cases.py."""
import numpy as np
import pytest

from dense_path_cases import RECORDED, arc_py, bits, distinct_of_reference, join, layout_py, recorded_case


@pytest.fixture(scope="module")
def api(ccmp_built):
    import closed_chain_motion_planner_amd as pkg

    return pkg


@pytest.mark.parametrize("obj", sorted(RECORDED))
def test_the_rule_reproduces_the_recorded_file_as_a_whole(oracle_det, obj):
    rec = RECORDED[obj]
    P, pj, pl, segs, file_rows = recorded_case(oracle_det, obj)
    ref = join(pj, pl, pj.shape[1], segs)
    assert ref["rows"].shape == (rec["rows"], 14) == file_rows.shape
    for a, b in rec["duplicates"]:
        assert np.array_equal(bits(ref["rows"][a]), bits(ref["rows"][b])), (a, b)
    worst = float(np.abs(ref["rows"] - file_rows).max())
    print("%s: whole file reproduced, max |dq| = %.3e rad" % (obj, worst))
    assert worst <= rec["bound"], worst
    if obj == "Wine_Bottle":
        assert ref["seg_ok"][0].tolist() == [1, 0, 1, 1]  # segment 1 stops short of its target: part of the contract, not an error
        last = ref["rows"][ref["seg_first"][0, 2] - 2]
        assert oracle_det.distance(last, pj[0][2]) > P.delta
    dis = join(pj, pl, pj.shape[1], segs, distinct=True)
    assert len(dis["rows"]) == rec["distinct_rows"]
    keep = distinct_of_reference(ref)
    assert len(keep) == rec["distinct_rows"] and np.array_equal(bits(dis["rows"]), bits(ref["rows"][keep]))
    assert np.array_equal(dis["seg_ok"], ref["seg_ok"]) and np.array_equal(dis["seg_newton"], ref["seg_newton"])


def _ragged(rng, F, max_len):
    path_len = rng.integers(0, max_len + 1, size=F).astype(np.int32)
    path_len[:4] = [0, 1, 2, max_len]
    seg_states = rng.integers(1, 9, size=(F, max_len - 1)).astype(np.int32)
    seg_states[rng.random(seg_states.shape) < 0.3] = 1  # n = 1: a segment that is its starting state alone
    seg_states[2, 0] = 1
    return path_len, seg_states


@pytest.mark.parametrize("distinct", [False, True])
def test_layout_ref_equals_the_restatement(api, distinct):
    rng = np.random.default_rng(5)
    for F, max_len in ((11, 6), (4, 2), (7, 1), (64, 24)):
        if max_len >= 2:
            path_len, seg_states = _ragged(rng, F, max_len)
        else:
            path_len, seg_states = rng.integers(0, 2, size=F).astype(np.int32), np.zeros((F, 0), dtype=np.int32)
        pf, sf, rows = api.dense_layout_ref(path_len, max_len, seg_states, distinct=distinct)
        wpf, wsf, wrows = layout_py(path_len, max_len, seg_states, distinct)
        assert rows == wrows and np.array_equal(pf, wpf) and np.array_equal(sf, wsf), (F, max_len)
        # the rule's counts: sum (1 + n_i) + 1, or sum n_i + 1
        for f in range(F):
            L = int(path_len[f])
            n = int(seg_states[f, : max(L - 1, 0)].sum())
            assert pf[f + 1] - pf[f] == (0 if L == 0 else n + 1 + (0 if distinct else L - 1))
    pf, sf, rows = api.dense_layout_ref(np.zeros(0, np.int32), 5, None, distinct=distinct)
    assert rows == 0 and pf.tolist() == [0] and sf.shape == (0, 4)


def test_arc_ref_equals_a_python_float_sum(api):
    rng = np.random.default_rng(9)
    path_len, seg_states = _ragged(rng, 9, 5)
    pj = rng.uniform(-2.5, 2.5, size=(9, 5, 14))
    segs = {}
    for f in range(9):
        for i in range(int(path_len[f]) - 1):
            n = int(seg_states[f, i])
            st = np.concatenate([pj[f, i][None], rng.uniform(-2.5, 2.5, size=(n - 1, 14))])
            segs[(f, i)] = (1, st, n)
    ref, dis = join(pj, path_len, 5, segs), join(pj, path_len, 5, segs, distinct=True)
    for lay in (ref, dis):
        arc, length = api.dense_arc_ref(lay["rows"], lay["path_first"])
        warc, wlen = arc_py(lay["rows"], lay["path_first"], api.joint_distance)
        assert np.array_equal(bits(arc), bits(warc)) and np.array_equal(bits(length), bits(wlen))
        for f in range(9):
            a, b = lay["path_first"][f], lay["path_first"][f + 1]
            if b > a:
                assert arc[a] == 0.0 and not np.signbit(arc[a]) and length[f] == arc[b - 1]
            else:
                assert length[f] == 0.0 and not np.signbit(length[f])
        lay["arc"], lay["length"] = arc, length
    # a duplicated row adds exactly +0.0: both layouts carry the same arcs at corresponding rows
    keep = distinct_of_reference(ref)
    assert np.array_equal(bits(ref["arc"][keep]), bits(dis["arc"])) and np.array_equal(bits(ref["length"]), bits(dis["length"]))
    for s in ref["seg_first"].reshape(-1):
        if s >= 0:
            assert bits(ref["arc"][s : s + 1])[0] == bits(ref["arc"][s - 1 : s])[0]
