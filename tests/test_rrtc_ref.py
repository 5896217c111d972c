"""The host forms of the RRT-Connect rule (ccmp_rrtc_pick_ref, ccmp_roadmap_nearest_in_tree_ref, ccmp_rrtc_connected_ref: csrc/ccmp_rrtc.h
compiled for the host, the kernels' text) against the plain-Python restatement of tests/rrtc_cases.py, bit for bit.  No device.

Mutations of csrc/ccmp_rrtc.h tried against this file and tests/test_rrtc_cases.py, each reverted afterwards:
  `<` for `<=` in rrtc_arc_step (a row that lands exactly on the range is dropped)   test_pick_ref_on_synthetic_lists (the cases "range equals s_2", "range equals the last stored
                                                                                     row's sum")
  the "at least 1" dropped in rrtc_extend (row 0 becomes the vertex)                 test_pick_ref_on_synthetic_lists (the cases "first step beyond the range")
  the tie to the higher index (graph_closer's `<` on the index turned)               test_nearest_ref_against_brute_force (the duplicated rows: queries that copy row 5 k)
  the sample-order swap in step 4 (step 3's vertices before step 2's)                tests/test_rrtc_cases.py::test_commit_takes_indices_in_the_stated_total_order pins the
                                                                                     restatement; the kernel's order is held to it by tests/test_gpu_rrtc.py (RRTConnect
                                                                                     against HandRRTConnect, store rows and edges bit for bit)"""
import numpy as np
import pytest

import rrtc_cases as R


def _same(got, want, names):
    for n in ("outcome", "row_index"):
        assert got[n].tolist() == want[n].tolist(), [(names[i], int(got[n][i]), int(want[n][i])) for i in np.flatnonzero(got[n] != want[n])]
    assert got["row"].tobytes() == want["row"].tobytes()
    assert got["gap"].tobytes() == want["gap"].tobytes()


def test_pick_ref_on_synthetic_lists(ccmp_built):
    from closed_chain_motion_planner_amd import rrtc_pick_ref

    cases = R.synthetic_cases()
    names = [c[0] for c in cases]
    states, ns, ok, to, d = R.stack_cases(cases)
    for rng in sorted({c[5] for c in cases}):
        sel = np.array([c[5] == rng for c in cases])
        got = rrtc_pick_ref(states[sel], ns[sel], ok[sel], to[sel], d=d[sel], range=rng, mode=0)
        want = R.pick(0, states[sel], ns[sel], ok[sel], to[sel], d=d[sel], rng=rng)
        _same(got, want, [n for n, s in zip(names, sel) if s])
    by = {c[0]: i for i, c in enumerate(cases)}
    full = rrtc_pick_ref(states, ns, ok, to, d=d, range=0.5, mode=0)
    look = lambda name: (int(full["outcome"][by[name]]), int(full["row_index"][by[name]]))
    assert look("range equals s_2: <= keeps row 2") == (R.ADVANCED, 2)
    assert look("range equals the last stored row's sum, full list: unsettled") == (R.UNSETTLED, -1)
    assert look("range equals the last stored row's sum, whole list: advanced") == (R.ADVANCED, 3)
    assert look("first step beyond the range: row 1, advanced") == (R.ADVANCED, 1)
    assert look("first step beyond the range, full list") == (R.ADVANCED, 1)
    assert look("a NaN row") == (R.TRAPPED, -1) and look("a NaN distance") == (R.TRAPPED, -1)
    assert look("ns2 ok1 d0.5") == (R.REACHED, -1) and full["row"][by["ns2 ok1 d0.5"]].tobytes() == to[by["ns2 ok1 d0.5"]].tobytes()  # d == range: reached
    assert look("ns5 ok0 d0.25") == (R.UNSETTLED, -1) and look("ns3 ok0 d0.25") == (R.TRAPPED, -1) and look("ns0 ok1 d0.25") == (R.TRAPPED, -1)
    assert full["row"][by["first step beyond the range: row 1, advanced"]].tobytes() == states[by["first step beyond the range: row 1, advanced"], 1].tobytes()


def test_pick_ref_use_flags_and_connect_mode(ccmp_built):
    from closed_chain_motion_planner_amd import rrtc_pick_ref

    cases = R.synthetic_cases()
    states, ns, ok, to, d = R.stack_cases(cases)
    use = np.array([i % 3 for i in range(len(cases))], dtype=np.uint8)  # 0: none, 1: used, 2: no nearest vertex
    got = rrtc_pick_ref(states, ns, ok, to, d=d, use=use, range=0.5, mode=0)
    _same(got, R.pick(0, states, ns, ok, to, d=d, use=use, rng=0.5), [c[0] for c in cases])
    assert (got["outcome"][use == 0] == R.NONE).all() and (got["outcome"][use == 2] == R.TRAPPED).all()
    # step 3 on the same lists: v = a row near the list's end
    v = states[:, 2].copy()
    v[:, 0] += 0.125
    gotc = rrtc_pick_ref(states, ns, ok, v, use=use, mode=1)
    wantc = R.pick(1, states, ns, ok, v, use=use)
    _same(gotc, wantc, [c[0] for c in cases])
    assert {R.C_NOTHING, R.C_ADDED, R.C_JOINED, R.NONE} == set(gotc["outcome"].tolist())


@pytest.mark.parametrize("N", [0, 1, 2, 65, 257])
def test_nearest_ref_against_brute_force(ccmp_built, N):
    from closed_chain_motion_planner_amd import graph_labels_ref, nearest_in_tree_ref

    joints = R.tree_store(N)
    queries = R.tree_queries(joints, 7) if N else np.random.default_rng(1).uniform(-1, 1, size=(7, 14))
    trees = [("every vertex", 1, [0]), ("none", 1, []), ("alternating, 1 root", 2, [0]), ("nine components, 8 roots", 9, list(range(8)))]
    for name, stride, roots in trees:
        if roots and max(roots) >= N:
            continue
        labels = graph_labels_ref(R.tree_edges(N, stride), N) if N else np.zeros(0, dtype=np.int32)
        idx, dist = nearest_in_tree_ref(joints, labels, roots, queries)
        want_i, want_d = R.brute_nearest(joints, labels, roots, queries)
        assert idx.tolist() == want_i.tolist(), name
        assert dist.tobytes() == want_d.tobytes(), name
        if not roots:
            assert (idx == -1).all() and np.isinf(dist).all()
        else:
            inside = {int(labels[r]) for r in roots}
            assert all(i >= 0 and int(labels[i]) in inside and np.isfinite(joints[i]).all() for i in idx)
    if N >= 65:  # the tie of a duplicated row goes to the lower index: a query that copies row 5 k is answered by 5 k, not by 5 k + 2
        labels = graph_labels_ref(R.tree_edges(N, 1), N)
        q = joints[[5, 20, 25]]
        idx, dist = nearest_in_tree_ref(joints, labels, [0], q)
        assert idx.tolist() == [5, 20, 25] and (dist == 0.0).all() and (joints[[7, 22, 27]] == q).all()


def test_nearest_ref_empty_store_and_bad_roots(ccmp_built):
    from closed_chain_motion_planner_amd import CcmpError, nearest_in_tree_ref

    q = np.zeros((3, 14))
    idx, dist = nearest_in_tree_ref(np.zeros((0, 14)), np.zeros(0, dtype=np.int32), [], q)
    assert idx.tolist() == [-1, -1, -1] and np.isinf(dist).all()
    with pytest.raises(CcmpError):
        nearest_in_tree_ref(np.zeros((2, 14)), np.arange(2, dtype=np.int32), [2], q)
    with pytest.raises(CcmpError):
        nearest_in_tree_ref(np.zeros((2, 14)), np.arange(2, dtype=np.int32), [0] * 9, q)
    only_nan = np.full((2, 14), np.nan)
    idx, dist = nearest_in_tree_ref(only_nan, np.zeros(2, dtype=np.int32), [0], q)
    assert idx.tolist() == [-1, -1, -1] and np.isinf(dist).all()  # a NaN distance is never a candidate


def test_connected_ref_against_the_restatement(ccmp_built):
    from closed_chain_motion_planner_amd import rrtc_connected_ref

    r = np.random.default_rng(3)
    hits = 0
    for trial in range(40):
        N = int(r.integers(1, 12))
        labels = r.integers(0, 4, size=N).astype(np.int32)
        s = R.new_state(r.integers(-1, N + 1, size=int(r.integers(1, 9))), r.integers(-1, N + 1, size=int(r.integers(1, 9))), first_index=trial)
        s["best_gap"], s["counters"]["samples"] = 0.5 * trial, trial
        got, want = rrtc_connected_ref(labels, s), R.connected(labels, s)
        assert R.state_bits(got) == R.state_bits(want), (labels, s, got, want)
        hits += got["status"] == R.SOLVED
        assert R.state_bits(rrtc_connected_ref(labels, got)) == R.state_bits(got)
    assert 0 < hits < 40


def test_both_connected_refs_are_one_text(ccmp_built):
    """ccmp_plan_connected_ref and ccmp_rrtc_connected_ref compile one fold (csrc/ccmp_plan.h: first_connected) over their two state
    types: on the same lists and labels — lengths 0 .. 8, indices -1 .. N (both ends outside the store), N 0 .. 11, labels 0 .. 3 — they
    return the same (status, solved_start, solved_goal), that of the restatement, and leave every other field as given.  The seed was
    chosen on the restatement alone: between 1 and 39 of the 40 cases end SOLVED."""
    import plan_cases as P
    from closed_chain_motion_planner_amd import plan_connected_ref, rrtc_connected_ref

    r = np.random.default_rng(7)
    triple = lambda s: (s["status"], s["solved_start"], s["solved_goal"])
    hits = 0
    for trial in range(40):
        N = int(r.integers(0, 12))
        labels = r.integers(0, 4, size=N).astype(np.int32)
        starts, goals = r.integers(-1, N + 1, size=int(r.integers(0, 9))), r.integers(-1, N + 1, size=int(r.integers(0, 9)))
        sr = R.new_state(starts, goals, first_index=trial)
        sr["best_a"], sr["best_b"], sr["best_gap"], sr["cycle"] = trial, trial + 1, 0.25 * trial, trial
        sr["counters"] = {n: trial + i for i, n in enumerate(R.COUNTERS)}
        sp = P.new_state(np.arange(8) + 0.5 * trial, 1.5 * trial, first_index=trial)
        sp["starts"], sp["goals"] = sr["starts"], sr["goals"]
        sp["nearest"], sp["sprevious"], sp["size_at_check"], sp["cycle"] = trial, trial + 2, trial + 3, trial
        sp["counters"] = {n: 2 * trial + i for i, n in enumerate(P.COUNTERS)}
        want_r, want_p = R.connected(labels, sr), P.connected(labels, sp)
        assert triple(want_r) == triple(want_p)  # the two restatements agree with each other
        hits += want_r["status"] == R.SOLVED
        got_r, got_p = rrtc_connected_ref(labels, sr), plan_connected_ref(labels, sp)
        assert triple(got_r) == triple(got_p) == triple(want_r), (labels, starts, goals, got_r, got_p, want_r)
        assert R.state_bits(got_r) == R.state_bits(want_r) and P.state_bits(got_p) == P.state_bits(want_p), (got_r, want_r, got_p, want_p)
    assert 1 <= hits <= 39, hits
