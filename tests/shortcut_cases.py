"""Shortcut solution paths: a plain-Python restatement of the rule of csrc/ccmp_shortcut.h and the expected values the tests compare with.

The expected values are never the code under test.  A pair's test is the det oracle's `is_satisfied(w_j)` followed by ONE uninterrupted
`discrete_geodesic(w_i, w_j, max_states=4096)`; everything else is restated here:

    candidates     (f, i, j), 0 <= i, j < L, j - i >= 2, j - i <= max_span (0: every span), both rows finite, in (f, i, j) order
    admitted edge  j == i + 1, or pair_ok[i][j] == 1
    weight         the joint distance in the device's rounding (graph_cases.edge_weight: an exactly rounded FMA chain and sqrt)
    selection      d[0] = +0.0; d[j] = min over admitted i < j of d[i] + w(i, j) where d[i] is finite, w >= 0 and the sum is finite;
                   hops[j] = the least hops[i] + 1 over the i attaining it; pred[j] = the smallest such i with that hops
    result         kept = the walk of pred from L - 1 written forwards; cost_in = the left-to-right sum of the adjacent weights;
                   cost_out = d[L - 1]; d[L - 1] == +inf: the path unchanged
"""
import math

import numpy as np

from graph_cases import edge_weight

INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_f64(a, b):
    """bit for bit, except that any NaN equals any NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def pairs_py(path_joints, path_len, max_span=0):
    out = []
    for f, L in enumerate(path_len):
        L = int(L)
        fin = [bool(np.isfinite(path_joints[f][i]).all()) for i in range(L)]
        for i in range(L):
            for j in range(i + 2, L):
                if (max_span == 0 or j - i <= max_span) and fin[i] and fin[j]:
                    out.append((f, i, j))
    return np.array(out, dtype=np.int32).reshape(-1, 3)


def weights_exact(rows):
    """(L,L) joint distances of rows whose coordinates are small multiples of 2^-3: every difference, square and sum is exact in binary64,
    so the FMA chain equals plain arithmetic and only the square root rounds (correctly, here and on the device).  NaN rows give NaN."""
    r = np.asarray(rows, dtype=np.float64)
    L = len(r)
    d2 = np.zeros((L, L))
    for c in range(14):
        e = r[:, None, c] - r[None, :, c]
        d2 += e * e
    assert np.all(np.isnan(d2) | (d2 == np.round(d2 * 64) / 64)) and np.nanmax(d2, initial=0.0) < 2 ** 40  # exactness holds
    return np.sqrt(d2)


def weights_fma(rows):
    """(L,L) joint distances in the device's rounding, entry by entry (exact rational arithmetic: for short paths)"""
    L = len(rows)
    W = np.full((L, L), np.nan)
    for i in range(L):
        for j in range(i + 1, L):
            W[i, j] = edge_weight(rows[i], rows[j])
    return W


def select_py(rows, L, ok, W):
    """one path: (kept list, cost_in, cost_out); rows (>= L,14), ok (max_len,max_len), W (L,L) with W[i][j] for i < j"""
    L = int(L)
    if L == 0:
        return [], 0.0, 0.0
    cost_in = 0.0
    for j in range(1, L):
        cost_in = cost_in + float(W[j - 1, j])
    pred = [-1] * L
    dn = np.array([0.0] + [INF] * (L - 1))
    hn = np.full(L, np.iinfo(np.int64).max, dtype=np.int64)
    hn[0] = 0
    for j in range(1, L):
        i = np.arange(j)
        w = W[:j, j]
        adm = (i == j - 1) | (np.asarray(ok)[:j, j] == 1)
        with np.errstate(invalid="ignore", over="ignore"):
            c = dn[:j] + w
            passing = adm & np.isfinite(dn[:j]) & (w >= 0.0) & np.isfinite(c)
        if not passing.any():
            continue
        best = c[passing].min()
        tight = passing & (c == best)
        h = hn[:j][tight].min()
        p = int(np.nonzero(tight & (hn[:j] == h))[0][0])
        dn[j], hn[j], pred[j] = best, h + 1, p
    if not math.isfinite(dn[L - 1]):
        return list(range(L)), cost_in, INF
    kept, v = [], L - 1
    while v >= 0:
        kept.append(v)
        v = pred[v]
    kept.reverse()
    assert len(kept) == hn[L - 1] + 1
    return kept, cost_in, float(dn[L - 1])


def expect(path_joints, path_len, pair_ok, weights=weights_fma):
    """the whole result for F paths as the library lays it out: joints (the input's rows behind out_len), out_len, kept, cost_in, cost_out"""
    pj = np.asarray(path_joints, dtype=np.float64)
    F, ml = pj.shape[0], pj.shape[1]
    out = {"joints": pj.copy(), "out_len": np.zeros(F, dtype=np.int32), "kept": np.full((F, ml), -1, dtype=np.int32), "cost_in": np.zeros(F),
           "cost_out": np.zeros(F)}
    for f in range(F):
        L = int(path_len[f])
        kept, ci, co = select_py(pj[f], L, np.asarray(pair_ok)[f], weights(pj[f, :L]) if L else None)
        out["out_len"][f], out["cost_in"][f], out["cost_out"][f] = len(kept), ci, co
        out["kept"][f, : len(kept)] = kept
        out["joints"][f, : len(kept)] = pj[f, kept]
    return out


def same_selection(got, want, what=""):
    g = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in got.items()}
    assert np.array_equal(g["out_len"], want["out_len"]), (what, g["out_len"], want["out_len"])
    assert np.array_equal(g["kept"], want["kept"]), (what, g["kept"], want["kept"])
    assert same_f64(g["cost_in"], want["cost_in"]), (what, g["cost_in"], want["cost_in"])
    assert same_f64(g["cost_out"], want["cost_out"]), (what, g["cost_out"], want["cost_out"])
    assert same_f64(g["joints"], want["joints"]), what


def oracle_pairs(O, P, path_joints, path_len, max_span=0, edge=None):
    """pair_ok, pair_states, pair_newton (F,max_len,max_len) from the oracle: per candidate is_satisfied(w_j), then one uninterrupted
    traversal.  edge(a, b) -> (ok, n, its) replaces the plain traversal (a scene's)."""
    pj = np.asarray(path_joints, dtype=np.float64)
    F, ml = pj.shape[0], pj.shape[1]
    ok = np.zeros((F, ml, ml), dtype=np.uint8)
    ns = np.zeros((F, ml, ml), dtype=np.int32)
    nw = np.zeros((F, ml, ml), dtype=np.int32)
    memo = {}
    for f, i, j in pairs_py(pj, path_len, max_span):
        key = (pj[f, i].tobytes(), pj[f, j].tobytes())
        if key not in memo:
            if not O.is_satisfied(P, pj[f, j]):
                memo[key] = (0, 1, 0)  # checkMotion: the target fails, nothing is traversed
            elif edge is not None:
                memo[key] = edge(pj[f, i], pj[f, j])
            else:
                r, st, its = O.discrete_geodesic(P, pj[f, i], pj[f, j], max_states=4096)
                memo[key] = (int(r), len(st), int(its))
        ok[f, i, j], ns[f, i, j], nw[f, i, j] = memo[key]
    return ok, ns, nw


def recorded_waypoints(O, obj, mode, projected):
    """(P, path_joints (1,L,14), path_len) of a recorded file's waypoints.  The file's rows do not pass the oracle's is_satisfied (Wine_Bottle:
    |f| = 0.010 / 0.047 against tolerances 0.001 / 0.005), so checkMotion refuses every pair INTO one of them at its target test and nothing
    is traversed; projected=True puts each row through the oracle's own project() first (it moves a joint by 0.015 rad at most), which
    gives waypoints the planner could have produced: on those the traversals run and both outcomes occur."""
    from dense_path_cases import recorded_case

    P, pj, pl, _, _ = recorded_case(O, obj, mode)
    if projected:
        pj = pj.copy()
        for j in range(int(pl[0])):
            pj[0, j] = O.project(P, pj[0, j])[1]
            assert O.is_satisfied(P, pj[0, j])
    return P, pj, pl


def grid_rows(rng, F, ml):
    """rows on the grid of multiples of 2^-3 in [-2, 2]: weights_exact applies"""
    return rng.integers(-16, 17, size=(F, ml, 14)).astype(np.float64) * 0.125


def random_ok(rng, F, ml, density):
    if density <= 0:
        return np.zeros((F, ml, ml), dtype=np.uint8)
    if density >= 1:
        return np.ones((F, ml, ml), dtype=np.uint8)
    return (rng.random((F, ml, ml)) < density).astype(np.uint8)


def collinear(L, ml=None):
    """rows k * 0.125 * e_0: every weight and every sum is exact, so a direct edge ties with its detour"""
    r = np.zeros((1, ml or L, 14))
    r[0, :L, 0] = np.arange(L) * 0.125
    return r
