"""ccmp_graph_shortest_paths_ref (heap Dijkstra + the rule text of csrc/ccmp_path.h compiled for the host) against the plain-Python
restatement of tests/path_cases.py on every case, bit for bit.  No device."""
import numpy as np
import pytest

from path_cases import CASES, case_and_expected, same_answer


@pytest.fixture(scope="module")
def ref(ccmp_built):
    from closed_chain_motion_planner_amd import shortest_paths_ref

    return shortest_paths_ref


@pytest.mark.parametrize("name", list(CASES))
def test_ref_equals_the_restatement(ref, name):
    """cases 1-6: cost, path_len, path, dist_out and pred_out identical; the cost is the left-to-right sum along the path"""
    case, want = case_and_expected(name)
    cost, plen, paths, dist, pred = ref(case["uv"], case["w"], len(case["joints"]), case["src"], case["dst"], full=True)
    same_answer(case, want, cost, plen, paths, dist, pred)
    assert (plen > 0).any()


def test_the_cases_hold_what_they_are_for():
    chain, want = case_and_expected("chain")
    assert want["path_len"][0] == 1100 and want["cost"][0] == 1099 / 16.0 and want["path_len"][1] == 551
    rnd, want = case_and_expected("random")
    assert len(rnd["src"]) == 64 and len(rnd["uv"]) > 4900
    assert (want["path_len"] == 0).sum() >= 10 and (want["path_len"] == 1).sum() >= 2 and np.isinf(want["cost"][want["path_len"] == 0]).all()
    assert (rnd["src"][17], rnd["dst"][17]) == (rnd["src"][0], rnd["dst"][0]) and np.array_equal(want["paths"][17], want["paths"][0])
    ties, want = case_and_expected("ties")
    assert want["cost"][0] == 7.0 and want["path_len"][0] == 15
    # a vertex inside the lattice has two tight parents one level up: the rule must have chosen the smaller
    two = 0
    adj = {}
    for (u, v) in ties["uv"]:
        adj.setdefault(int(u), set()).add(int(v))
        adj.setdefault(int(v), set()).add(int(u))
    d, p = want["dist"][0], want["pred"][0]
    for v in range(64):
        parents = [u for u in adj[v] if d[u] + 0.5 == d[v]]
        if len(parents) == 2:
            two += 1
            assert p[v] == min(parents)
    assert two == 49
    zero, want = case_and_expected("zero_cycle")
    assert want["cost"][2] == 0.0 and want["path_len"][2] == 2 and want["path_len"][0] == 6  # straight across the triangle, not around it
    ab, want = case_and_expected("absorbed")
    assert want["dist"][0][1] == want["dist"][0][2] == 1024.0 and want["path_len"][0] == 6 and want["dist"][4][0] == 1e-17
    nan, want = case_and_expected("nan")
    assert want["paths"][0].tolist() == [0, 1, 4, 3] and want["path_len"][2] == 0 and want["path_len"][3] == 0 and want["path_len"][4] == 0


def test_nan_weights_given_directly(ref):
    """weights no store would compute: NaN, +inf and a negative one never pass; -0.0 is a zero weight"""
    uv = np.array([[0, 1], [1, 2], [0, 2], [2, 3], [3, 4], [0, 4]], np.int32)
    w = np.array([1.0, np.nan, np.inf, -0.0, -1.0, 5.0])
    cost, plen, paths, dist, pred = ref(uv, w, 5, [0, 2, 0], [2, 3, 3], full=True)
    assert plen.tolist() == [0, 2, 0] and np.isinf(cost[0]) and cost[1] == 0.0 and np.signbit(cost[1]) == False  # noqa: E712
    assert dist[0].tolist() == [0.0, 1.0, np.inf, np.inf, 5.0] and pred[0].tolist() == [-1, 0, -1, -1, 0]


@pytest.mark.parametrize("name", ["ties", "chain"])
def test_short_buffer(ref, name):
    """case 7: max_len one below the path's length — the length is reported, the path keeps its sentinel; the other pairs are written"""
    import ctypes as C

    from closed_chain_motion_planner_amd import _lib

    case, want = case_and_expected(name)
    F, n = len(case["src"]), len(case["joints"])
    ml = int(want["path_len"][0]) - 1
    cost, plen, path = np.empty(F), np.empty(F, np.int32), np.full((F, ml), -7, np.int32)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    p = lambda a, t: a.ctypes.data_as(t)
    rc = _lib.lib().ccmp_graph_shortest_paths_ref(p(case["uv"], ip), p(case["w"], dp), len(case["uv"]), n, p(case["src"], ip), p(case["dst"], ip), F, ml, p(cost, dp),
                                                  p(plen, ip), p(path, ip), None, None)
    assert rc == 0
    paths = []
    for f in range(F):
        if want["path_len"][f] > ml:
            assert (path[f] == -7).all()
            paths.append(None)
        else:
            assert (path[f, want["path_len"][f]:] == -7).all()
            paths.append(path[f, :plen[f]])
    assert paths[0] is None and any(q is not None and len(q) for q in paths)
    same_answer(case, want, cost, plen, paths)
