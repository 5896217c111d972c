"""ccmp_path_smooth's own kernels (csrc/ccmp_kernels_smooth.hip: smooth_load, smooth_gather, smooth_bracket, smooth_pick, smooth_accept,
smooth_length, smooth_store) on batches wide and long enough for their indexing to go wrong: 70 ragged paths with 41 active in the first
pass and 18 in the second (path_of over the seg_first / vert_first prefixes, sixteen lanes per item across several 256-thread blocks,
finished paths in both buffers), lengths of 69, 138, 32 and 128 distances (a partial 64-distance chunk behind full ones), a scene case
whose verdict depends on WHICH midpoint's clearance is read, and the call counts.  tests/test_gpu_smooth.py has at most 7 paths, 5
active, and no partial chunk behind a full one.  The batches are built in tests/smooth_cases.py and checked on the oracle alone in
tests/test_smooth_cases.py.  Expected values are never the code under test: smooth_cases.Restatement on the det oracle, and
graph_cases.edge_weight for the lengths; bit for bit (uint64 views, NaN equal to NaN), smooth_cases.same_result.

With a result of 9 vertices no path of the wide batch runs a third pass, so at max_steps 3 stop 2 cannot occur there; the batch is run
at max_steps 3 and once more at max_steps 2, where it does.

Wall time on the MI355X: 1.6 s for the five tests (test_wide_batch 0.9 s, test_long_batch 0.4 s, the others under 0.1 s each), of which
the batches and their restatements take 1.1 s (wide, both modes and both max_steps: 0.76 s; long: 0.33 s).

Mutation check: one-token changes of csrc/ccmp_kernels_smooth.hip, each choosing among values or addresses the unmutated kernel reads for
the same item (no index leaves an allocation, no loop bound or barrier changes), on scratch builds; one run each of this module,
test_gpu_arm_models_planner.py::test_smooth and tests/test_gpu_smooth.py.  All gave wrong answers, none a fault, a hang or an abort.
What failed (test_smooth's share is in its module's docstring as well):
  smooth_length_kernel: `base + q < L` dropped from the            all five tests here, test_smooth (8), 22 of the 23 tests of test_gpu_smooth.py: the
  serial sum                                                       sum reads the slots of shared memory behind the chunk's live ones, which hold
                                                                   whatever the block left there — not only where a partial chunk follows a full one
  smooth_accept_kernel: clear_m at seg_first + i for               test_scene_reads_the_incoming_midpoint; test_gpu_smooth.py::test_scene_case
  seg_first + (i - 1)                                              (test_smooth[*-scene] passes: no vertex there straddles its margin)
  smooth_bracket_kernel: the fallback row `lower ? k : k - 1`      test_wide_batch, test_long_batch, test_smooth (8); test_gpu_smooth.py::
                                                                   test_every_branch, test_scene_case
  smooth_gather_kernel: pair_path[e] = paths[0].f                  test_wide_batch, test_long_batch, test_smooth (8); test_gpu_smooth.py::
                                                                   test_ragged_batch
  smooth_store_kernel: where[0] for where[f]                       test_wide_batch, test_long_batch, test_smooth[*-scene] (4); test_gpu_smooth.py::
                                                                   test_ragged_batch
  smooth_length_kernel: where[0] for where[f]                      the same seven
test_identity_lengths and test_last_counts fail under the first mutant alone: they hold what no listed mutation but that one touches
(the chunk sums at nine lengths; the counters of ccmp_smooth.cpp)."""
import ctypes as C
import time

import numpy as np
import pytest

import smooth_cases as S
from dense_path_cases import oracle_segments
from shortcut_cases import recorded_waypoints
from smooth_cases import Restatement, expect, mirror_fill, same_result
from test_gpu_parity import _oracle_problem
from test_gpu_smooth import GUARD_F64, OBJ, _dev, _guarded, cons  # noqa: F401 (cons is a fixture)

pytestmark = pytest.mark.gpu


def _behind(want, fill):
    """`want` with the rows behind out_len taken from `fill` (what the mirror's outputs start as)"""
    w = dict(want)
    w["joints"] = np.array(fill, dtype=np.float64)
    for f, n in enumerate(want["out_len"]):
        w["joints"][f, :n] = want["joints"][f, :n]
    return w


def _stock(cons, oracle_det, mode):
    c, P = cons(OBJ, mode), S.stock_problem(oracle_det, mode)
    assert bytes(_oracle_problem(oracle_det, c)) == bytes(P)
    return c, P


def test_wide_batch(cons, oracle_det):
    c, P = _stock(cons, oracle_det, 0)
    c1, P1 = _stock(cons, oracle_det, 1)
    t = time.perf_counter()
    case, case1 = S.wide_batch(oracle_det, P), S.wide_batch(oracle_det, P1)
    pj, pl, cap, mc, R = case["pj"], case["pl"], case["out_max_len"], case["min_change"], case["R"]
    assert case["max_steps"] == 3 and S.same_f64(case1["pj"], pj)
    want, want2 = expect(R, pj, pl, 3, mc, cap, GUARD_F64), expect(R, pj, pl, 2, mc, cap, GUARD_F64)
    want1 = expect(case1["R"], pj, pl, 3, case1["min_change"], cap, mirror_fill(pj, cap))
    print("the batch and its three expectations: %.2f s" % (time.perf_counter() - t))
    pj_d, pl_d = _dev(pj), _dev(pl)
    for tile in (1, 7, 65536):
        rc, out, intact, _ = _guarded(c, pj_d, pl_d, cap, opts=(3, mc, 16, 128, 4096, tile))
        assert rc == 0 and intact, tile
        same_result(out, want, ("tile", tile))  # rows behind out_len keep the guard value: `want` was filled with it
    # a result of 9 vertices ends every path before a third pass: stop 2 occurs at max_steps 2 (tests/test_smooth_cases.py)
    assert 2 in want2["stop"] and 2 not in want["stop"]
    rc, out, intact, _ = _guarded(c, pj_d, pl_d, cap, opts=(2, mc, 16, 128, 4096, 65536))
    assert rc == 0 and intact
    same_result(out, want2, "max_steps 2")
    filled = _behind(want, mirror_fill(pj, cap))
    kw = dict(max_steps=3, min_change=mc, out_max_len=cap, stats=True)
    same_result(c.smooth_paths(pj_d, pl_d, **kw), filled, "device form")
    same_result(c.smooth_paths(pj, pl, **kw), filled, "host form")
    same_result(c.smooth_paths(pj_d, pl_d, chunk_states=2, round_budget=8, **kw), filled, "lists of 2, round budget 8")
    same_result(c1.smooth_paths(pj_d, pl_d, max_steps=3, min_change=case1["min_change"], out_max_len=cap, stats=True), want1, "analytic mode")


def test_long_batch(cons, oracle_det):
    c, P = _stock(cons, oracle_det, 0)
    t = time.perf_counter()
    case = S.long_batch(oracle_det, P)
    pj, pl, cap = case["pj"], case["pl"], case["out_max_len"]
    want = expect(Restatement(oracle_det, P), pj, pl, case["max_steps"], case["min_change"], cap, mirror_fill(pj, cap))
    print("the batch and its expectation: %.2f s" % (time.perf_counter() - t))
    assert want["out_len"].tolist() == [139, 129, 2]
    kw = dict(max_steps=case["max_steps"], min_change=case["min_change"], out_max_len=cap, stats=True)
    got = c.smooth_paths(_dev(pj), _dev(pl), **kw)
    same_result(got, want, "device form")
    same_result(c.smooth_paths(pj, pl, **kw), want, "host form")
    # the 139 vertices as a path of their own: every segment's flag is the oracle's traversal of that segment
    dense = c.densify_paths(got["joints"][:1].contiguous(), got["out_len"][:1].contiguous(), distinct=True)
    segs = oracle_segments(oracle_det, P, want["joints"][:1], [139])
    assert np.array_equal(dense["seg_ok"][0].cpu().numpy(), np.array([segs[(0, i)][0] for i in range(138)], dtype=np.uint8))


def test_identity_lengths(cons, oracle_det):
    c, _ = _stock(cons, oracle_det, 0)
    case = S.identity_batch()
    pj, pl, cap = case["pj"], case["pl"], case["out_max_len"]
    want = S.identity_expect(case, mirror_fill(pj, cap))  # the lengths: Python sums of graph_cases.edge_weight
    kw = dict(max_steps=0, out_max_len=cap, stats=True)
    same_result(c.smooth_paths(_dev(pj), _dev(pl), **kw), want, "device form")
    same_result(c.smooth_paths(pj, pl, **kw), want, "host form")
    rc, out, intact, _ = _guarded(c, _dev(pj), _dev(pl), cap, opts=(0, 0.005, 16, 128, 4096, 65536))
    assert rc == 0 and intact
    same_result(out, S.identity_expect(case, GUARD_F64), "guarded")


def test_scene_reads_the_incoming_midpoint(cons, oracle_det):
    from closed_chain_motion_planner_amd import scene as SC

    c, P = _stock(cons, oracle_det, 0)
    sc = SC.ProxyValidityChecker(c).scene
    case = S.straddle_scene_case(oracle_det, P, sc)
    pj, pl, cap, margin = case["pj"], case["pl"], case["out_max_len"], case["margin"]
    want = expect(S.scene_restatement(oracle_det, P, sc, margin), pj, pl, case["max_steps"], case["min_change"], cap, mirror_fill(pj, cap))
    assert want["moved"][0] >= 1 and want["stats"][0, S.REFUSED] >= 1
    for chunk in (2, 16):
        kw = dict(max_steps=case["max_steps"], min_change=case["min_change"], out_max_len=cap, scene=sc, margin=margin, chunk_states=chunk, stats=True)
        same_result(c.smooth_paths(_dev(pj), _dev(pl), **kw), want, ("device form", chunk))
        same_result(c.smooth_paths(pj, pl, **kw), want, ("host form", chunk))


def _last_counts():
    from closed_chain_motion_planner_amd import _lib

    v = [C.c_longlong(-1) for _ in range(3)]
    _lib.lib().ccmp_smooth_last_counts(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)  # extend calls, projector calls, bytes read on the host


def test_last_counts(cons, oracle_det):
    from closed_chain_motion_planner_amd import _lib

    c = cons(OBJ, 0)
    P, pj, pl = recorded_waypoints(oracle_det, OBJ, 0, True)
    R = Restatement(oracle_det, P)
    want = expect(R, pj, pl, 3, 0.005, 33, mirror_fill(pj, 33))
    passes = int(want["passes"].max())
    assert pl.tolist() == [5] and passes == 3 and max(R.list_lengths) > 2
    counts = {}
    for chunk in (2, 16):
        same_result(c.smooth_paths(_dev(pj), _dev(pl), max_steps=3, chunk_states=chunk, stats=True), want, ("device form", chunk))
        counts[("device", chunk)] = _last_counts()
        same_result(c.smooth_paths(pj, pl, max_steps=3, chunk_states=chunk, stats=True), want, ("host form", chunk))
        counts[("host", chunk)] = _last_counts()
    print(counts)
    for (form, chunk), (extend, project, read) in counts.items():
        # a pass: three midpoint steps (a densify of at least one extend call and one projector call each) and one test step
        assert project == 3 * passes and extend >= 4 * passes and read > 0, (form, chunk)
    for chunk in (2, 16):
        assert counts[("device", chunk)][:2] == counts[("host", chunk)][:2], chunk
    assert counts[("device", 2)][0] > counts[("device", 16)][0]  # a list longer than 2 exists: lists of 2 need a continuation
    # NULL for any of the three pointers is accepted
    L = _lib.lib()
    L.ccmp_smooth_last_counts(None, None, None)
    for k in range(3):
        v = [C.c_longlong(-1) for _ in range(3)]
        L.ccmp_smooth_last_counts(*[None if j == k else C.byref(v[j]) for j in range(3)])
        assert [v[j].value for j in range(3) if j != k] == [counts[("host", 16)][j] for j in range(3) if j != k] and v[k].value == -1
