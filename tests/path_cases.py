"""Cases and an independent restatement for the shortest paths on the roadmap graph (include/ccmp.h: ccmp_roadmap_shortest_paths,
ccmp_graph_shortest_paths_ref; the rule: csrc/ccmp_path.h).  Host only; shared by tests/test_path_ref.py and tests/test_gpu_path.py.

  * `restate`: the rule in plain Python floats — a heapq Dijkstra for d, then hops (breadth first over the tight edges) and predecessors
    (the smallest tight parent one level up) by definition.  No numpy reductions, nothing shared with the library;
  * the case builders.  A case is a store (joints (N,14), poses (N,8)), an edge list uv (E,2) and pairs; the weights are
    graph_cases.edge_weight of the joint rows (exact rational FMA chain, one rounding per step), which is what add_edges computes on the
    device.  Where ties matter the rows differ in ONE coordinate by a power of two, so the weight is that power of two exactly."""
import functools
import heapq
import math

import numpy as np

from graph_cases import edge_weight

INF = float("inf")
NO_HOPS = 2**31 - 1
BASE_ROW = tuple(0.125 * (c - 7) for c in range(14))  # exact binary fractions


def passes(du, w):
    """(the candidate over an edge of weight w from distance du, whether it passes)"""
    c = du + w
    return c, (du < INF and w >= 0.0 and c < INF)  # NaN fails every comparison


def restate(uv, w, n, s):
    """(d, hops, pred) lists of length n for the source s"""
    adj = [[] for _ in range(n)]
    for (u, v), x in zip(uv, w):
        adj[int(u)].append((int(v), float(x)))
        adj[int(v)].append((int(u), float(x)))
    d = [INF] * n
    d[s] = 0.0
    heap = [(0.0, s)]
    while heap:
        du, u = heapq.heappop(heap)
        if du != d[u]:
            continue
        for v, x in adj[u]:
            c, ok = passes(du, x)
            if ok and c < d[v]:
                d[v] = c
                heapq.heappush(heap, (c, v))
    tight = lambda u, x, v: passes(d[u], x)[1] and passes(d[u], x)[0] == d[v]
    hops = [NO_HOPS] * n
    hops[s] = 0
    level, r = [s], 0
    while level:
        r += 1
        nxt = []
        for u in level:
            for v, x in adj[u]:
                if hops[v] == NO_HOPS and tight(u, x, v):
                    hops[v] = r
                    nxt.append(v)
        level = nxt
    pred = [-1] * n
    for v in range(n):
        if hops[v] in (0, NO_HOPS):
            continue
        pred[v] = min(u for u, x in adj[v] if hops[u] == hops[v] - 1 and tight(u, x, v))
    return d, hops, pred


def walk(d, hops, pred, t):
    """(cost, length, path) to t"""
    if hops[t] == NO_HOPS:
        return INF, 0, []
    path = [t]
    while pred[path[-1]] >= 0:
        path.append(pred[path[-1]])
        assert len(path) <= hops[t] + 1
    assert len(path) == hops[t] + 1
    return d[t], len(path), path[::-1]


def expected(case):
    """the restatement on every pair of a case: cost (F,), path_len (F,), paths (list), dist (F,N), pred (F,N)"""
    n, uv, w = len(case["joints"]), case["uv"], case["w"]
    cost, plen, paths, dist, pred = [], [], [], [], []
    memo = {}
    for s, t in zip(case["src"], case["dst"]):
        s, t = int(s), int(t)
        if s not in memo:
            memo[s] = restate(uv, w, n, s)
        d, h, p = memo[s]
        c, ln, path = walk(d, h, p, t)
        cost.append(c), plen.append(ln), paths.append(np.array(path, dtype=np.int32)), dist.append(d), pred.append(p)
    return {"cost": np.array(cost), "path_len": np.array(plen, dtype=np.int32), "paths": paths, "dist": np.array(dist).reshape(len(cost), n),
            "pred": np.array(pred, dtype=np.int32).reshape(len(cost), n)}


def path_cost(case, path):
    """the left-to-right float sum of the weights along a path (parallel edges of a store have equal weights)"""
    wt = {}
    for (u, v), x in zip(case["uv"], case["w"]):
        wt[(int(u), int(v))] = wt[(int(v), int(u))] = float(x)
    acc = 0.0
    for a, b in zip(path[:-1], path[1:]):
        acc = acc + wt[(int(a), int(b))]
    return acc


def _poses(joints, rng=None):
    """poses for a store: the position is the first three joints (NaN rows: the origin), the rotation the identity or a random one"""
    n = len(joints)
    p = np.zeros((n, 8))
    p[:, :3] = np.where(np.isfinite(joints[:, :3]), joints[:, :3], 0.0)
    p[:, 6] = 1.0
    if rng is not None:
        q = rng.normal(size=(n, 4))
        p[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return p


def _case(name, joints, uv, pairs, poses=None):
    joints = np.ascontiguousarray(joints, dtype=np.float64)
    uv = np.ascontiguousarray(uv, dtype=np.int32).reshape(-1, 2)
    w = np.array([edge_weight(joints[u], joints[v]) for u, v in uv], dtype=np.float64)
    pairs = np.array(pairs, dtype=np.int32).reshape(-1, 2)
    case = {"name": name, "joints": joints, "poses": _poses(joints) if poses is None else poses, "uv": uv, "w": w,
            "src": np.ascontiguousarray(pairs[:, 0]), "dst": np.ascontiguousarray(pairs[:, 1])}
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def _rows(n):
    return np.tile(np.array(BASE_ROW), (n, 1))


def _shuffle_edges(uv, rng):
    uv = np.array(uv, dtype=np.int32).reshape(-1, 2)
    flip = rng.random(len(uv)) < 0.5
    uv[flip] = uv[flip][:, ::-1]
    return uv[rng.permutation(len(uv))]


@functools.lru_cache(maxsize=None)
def chain_case():
    """1 100 vertices in a line in shuffled index order, every weight exactly 1/16: more lanes than a block has edges per lane, 1 099
    hops, about 1 100 rounds.  End to end and to the middle, both ways."""
    n = 1100
    rng = np.random.default_rng(11)
    perm = rng.permutation(n)
    joints = _rows(n)
    joints[perm, 0] = np.arange(n) / 16.0
    uv = _shuffle_edges(np.stack([perm[:-1], perm[1:]], axis=1), rng)
    return _case("chain", joints, uv, [(perm[0], perm[-1]), (perm[0], perm[550]), (perm[-1], perm[0]), (perm[550], perm[3])])


@functools.lru_cache(maxsize=None)
def random_case():
    """N = 2 000, E = 5 000, rows drawn as base_store's are (14 joint angles inside the Panda's limits), edges inside five blocks of
    unequal size plus isolated vertices: several components.  64 pairs: inside a block, across blocks (unreachable), to an isolated
    vertex, src == dst, and one pair at three different f."""
    n, E = 2000, 5000
    rng = np.random.default_rng(2000)
    joints = rng.uniform(-2.8, 2.8, (n, 14))
    order = rng.permutation(n)
    sizes = [900, 500, 300, 150, 100]  # 50 vertices stay isolated
    blocks, at = [], 0
    for sz in sizes:
        blocks.append(order[at:at + sz])
        at += sz
    isolated = order[at:]
    uv = []
    for b in blocks:
        m = E * len(b) // sum(sizes)
        pick = rng.integers(0, len(b), (m, 2))
        pick = pick[pick[:, 0] != pick[:, 1]]
        uv.append(b[pick])
    uv = _shuffle_edges(np.concatenate(uv), rng)
    pairs = []
    for i in range(40):
        b = blocks[i % len(blocks)]
        pairs.append(tuple(rng.choice(b, 2, replace=False)))
    for i in range(10):
        pairs.append((rng.choice(blocks[i % 5]), rng.choice(blocks[(i + 1) % 5])))
    for i in range(4):
        pairs.append((rng.choice(blocks[0]), isolated[i]))
    pairs += [(blocks[0][7], blocks[0][7]), (isolated[5], isolated[5]), (isolated[6], blocks[1][0])]
    while len(pairs) < 64:
        pairs.append(pairs[0] if len(pairs) % 2 else pairs[1])  # the same pair again, at other f
    pairs[17] = pairs[0]
    return _case("random", joints, uv, pairs, poses=_poses(joints, rng))


@functools.lru_cache(maxsize=None)
def ties_case():
    """an 8 x 8 lattice in shuffled index order, every weight exactly 0.5, every fifth edge twice (once reversed): many cheapest paths
    and many tight parents per vertex — the predecessors must follow the smallest-index rule everywhere"""
    rng = np.random.default_rng(64)
    perm = rng.permutation(64)
    at = lambda i, j: int(perm[8 * i + j])
    joints = _rows(64)
    uv = []
    for i in range(8):
        for j in range(8):
            joints[at(i, j), 0] = 0.5 * i
            joints[at(i, j), 1] = 0.5 * j
            if i < 7:
                uv.append((at(i, j), at(i + 1, j)))
            if j < 7:
                uv.append((at(i, j), at(i, j + 1)))
    uv += [(b, a) for a, b in uv[::5]]
    pairs = [(at(0, 0), at(7, 7)), (at(7, 0), at(0, 7)), (at(3, 3), at(4, 6)), (at(7, 7), at(0, 0)), (at(2, 5), at(2, 5))]
    return _case("ties", joints, _shuffle_edges(uv, rng), pairs)


@functools.lru_cache(maxsize=None)
def zero_cycle_case():
    """three vertices with identical joint rows joined in a triangle (weights +0.0) with a tail on either side; indices chosen so that a
    rule on distances or indices alone would let two triangle vertices be each other's predecessor"""
    joints = _rows(8)
    #           tail a: 5 - 1      triangle: 4, 0, 6 (identical rows)      tail b: 2 - 7, and 3 hangs off the triangle's vertex 0
    for v, x in ((5, -0.75), (1, -0.25), (4, 0.0), (0, 0.0), (6, 0.0), (2, 0.5), (7, 1.5), (3, 0.0)):
        joints[v, 2] = x
    joints[3, 5] += 0.25
    uv = [(5, 1), (1, 4), (4, 0), (0, 6), (6, 4), (6, 2), (2, 7), (0, 3)]
    pairs = [(5, 7), (7, 5), (4, 6), (0, 7), (6, 3), (3, 5), (0, 0)]
    return _case("zero_cycle", joints, uv, pairs)


@functools.lru_cache(maxsize=None)
def absorbed_case():
    """a long first edge (1024), then an edge of 1e-17 rad that the sum absorbs, then onward, and the same again: vertices at EQUAL
    distance joined by a tight edge in both directions"""
    joints = np.zeros((7, 14))  # (from zero: 0 + 1e-17 is 1e-17, the rows themselves absorb nothing)
    steps = [(0, 1024.0), (1, 1e-17), (2, 0.25), (3, 1e-17), (4, 0.5)]
    for v, (coord, x) in enumerate(steps, start=1):
        joints[v] = joints[v - 1]
        joints[v, coord] += x
    joints[6] = joints[0]
    joints[6, 6] += 1e-17  # and one off the source itself: fl(0 + 1e-17) is not absorbed
    uv = [(0, 1), (2, 1), (2, 3), (4, 3), (4, 5), (6, 0)]
    pairs = [(0, 5), (5, 0), (1, 2), (2, 1), (6, 5), (3, 6)]
    case = _case("absorbed", joints, uv, pairs)
    assert 1024.0 + case["w"][1] == 1024.0 and case["w"][1] > 0.0
    return case


@functools.lru_cache(maxsize=None)
def nan_case():
    """vertex 2 is a pose-only vertex (a NaN joint row): its edges carry NaN weights and are never traversed.  0 - 1 - [2] - 3 with the
    detour 1 - 4 - 3, and vertex 5 behind vertex 2 alone: in 0's component by its label, unreachable by the rule"""
    joints = _rows(6)
    for v, x in ((0, 0.0), (1, 0.5), (3, 1.5), (4, 1.0), (5, 3.0)):
        joints[v, 0] = x
    joints[4, 1] += 2.0
    joints[2, :] = np.nan
    uv = [(0, 1), (1, 2), (2, 3), (1, 4), (4, 3), (2, 5)]
    pairs = [(0, 3), (3, 0), (0, 5), (0, 2), (2, 0), (5, 2)]
    case = _case("nan", joints, uv, pairs)
    assert np.isnan(case["w"][[1, 2, 5]]).all()
    return case


CASES = {"chain": chain_case, "random": random_case, "ties": ties_case, "zero_cycle": zero_cycle_case, "absorbed": absorbed_case, "nan": nan_case}


@functools.lru_cache(maxsize=None)
def case_and_expected(name):
    case = CASES[name]()
    return case, expected(case)


def bits(a):
    """the bytes of an array, every NaN as one canonical NaN"""
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    if a.dtype == np.float64:
        a = np.where(np.isnan(a), np.nan, a)
    return np.ascontiguousarray(a).view(np.uint8)


def same_answer(case, want, cost, path_len, paths, dist=None, pred=None):
    """one form's answer against the restatement, bit for bit; paths: per pair an index array (None: it did not fit)"""
    assert np.array_equal(np.asarray(path_len), want["path_len"]), (case["name"], path_len, want["path_len"])
    assert np.array_equal(bits(np.asarray(cost, dtype=np.float64)), bits(want["cost"])), (case["name"], cost, want["cost"])
    for f, p in enumerate(paths):
        if p is None:
            continue
        assert np.array_equal(np.asarray(p), want["paths"][f]), (case["name"], f, p, want["paths"][f])
        if len(p):
            assert (int(p[0]), int(p[-1])) == (int(case["src"][f]), int(case["dst"][f]))
            got = path_cost(case, p)
            assert got == float(np.asarray(cost)[f]) and math.copysign(1.0, got) == 1.0, (case["name"], f, got, cost[f])
    if dist is not None:
        assert np.array_equal(bits(np.asarray(dist, dtype=np.float64)), bits(want["dist"])), case["name"]
    if pred is not None:
        assert np.array_equal(np.asarray(pred), want["pred"]), case["name"]
