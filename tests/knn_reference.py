"""Reference ranking of the connection step (ccmp_knn_batch): per query, oracle_det.distance to every node (orc_distance: the FMA
chain over the 14 joints, then the square root), NaN distances dropped, the mode applied, sorted by (distance, node index).  The
distances of one (queries, nodes) pair are computed once and shared (`DistanceTable`): a prefix of the nodes or of the queries is a
slice of the same table."""
import ctypes as C

import numpy as np

KNN_ALL, KNN_NOT_SELF, KNN_EARLIER = 0, 1, 2


class DistanceTable:
    """D[q, j] = oracle.distance(queries[q], nodes[j]), one orc_distance call per pair"""

    def __init__(self, oracle, queries, nodes):
        self.queries = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 14)
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64).reshape(-1, 14)
        dp = C.POINTER(C.c_double)
        fn = oracle.lib.orc_distance
        qp = [C.cast(self.queries.ctypes.data + 112 * q, dp) for q in range(len(self.queries))]
        npt = [C.cast(self.nodes.ctypes.data + 112 * j, dp) for j in range(len(self.nodes))]
        self.D = np.empty((len(qp), len(npt)))
        for q, a in enumerate(qp):
            self.D[q] = [fn(a, b) for b in npt]

    def take(self, cols):
        """the table of the same queries over nodes[cols] (a reordering, a repetition): a distance is a function of its pair alone, so
        no pair is computed again"""
        import copy

        t = copy.copy(self)
        t.nodes, t.D = np.ascontiguousarray(self.nodes[cols]), np.ascontiguousarray(self.D[:, cols])
        return t

    def ties_at(self, k, q=0, n_nodes=None):
        """the indices of the nodes whose distance to query q equals the k-th smallest"""
        d = self.D[q, :n_nodes]
        return np.flatnonzero(d == np.sort(d[~np.isnan(d)])[k - 1])

    def rank(self, k, mode=KNN_ALL, self_base=0, n_nodes=None, n_queries=None):
        """(idx (Q,k) int32, dist (Q,k)) for the first n_queries queries over the first n_nodes nodes"""
        N = self.D.shape[1] if n_nodes is None else n_nodes
        Q = self.D.shape[0] if n_queries is None else n_queries
        idx = np.full((Q, k), -1, dtype=np.int32)
        dist = np.full((Q, k), np.inf)
        for q in range(Q):
            d = self.D[q, :N]
            elig = ~np.isnan(d)
            if mode == KNN_NOT_SELF and self_base + q < N:
                elig[self_base + q] = False
            if mode == KNN_EARLIER:
                elig[min(N, self_base + q):] = False
            j = np.flatnonzero(elig)
            order = j[np.lexsort((j, d[j]))][:k]  # ascending by distance, then by index
            idx[q, : len(order)] = order
            dist[q, : len(order)] = d[order]
        return idx, dist


def reference(oracle, nodes, queries, k, mode=KNN_ALL, self_base=0):
    return DistanceTable(oracle, queries, nodes).rank(k, mode, self_base)


THREADS = 256  # ccmp_launch::kKnnThreads: the queries of one block of the many-query kernels
MERGE_NARROW = 64  # up to this many partitions knn_merge_kernel<KC, 64> merges them, above it knn_merge_kernel<KC, 256>


def plan(num_cus, Q, N, tile, few_max, min_part, max_part):
    """ccmp_policy.cpp: plan_knn_tiled restated -> (few form?, nodes per partition, partitions): about two blocks per CU, at most
    max_part partitions, each a multiple of the tile and at least min_part nodes"""
    few = Q <= few_max
    units = Q if few else (Q + THREADS - 1) // THREADS
    want = max(1, min(max_part, (2 * num_cus + units - 1) // units)) if units else 1
    part = (N + want - 1) // want
    part = max(min_part, (part + tile - 1) // tile * tile)
    return few, part, ((N + part - 1) // part if N else 1)


def plan_constants(line):
    """(few_queries, min_partition, max_partitions) from the bracket that ends a ccmp_ctx_describe line of the k-NN kinds"""
    import re

    m = re.search(r"\[few_queries<=(\d+) min_partition=(\d+) max_partitions=(\d+)\]", line)
    assert m, line
    return tuple(int(g) for g in m.groups())


def described_shape(line):
    """(partitions, nodes per partition) as a ccmp_ctx_describe line of the k-NN kinds prints them for its assumed node count"""
    import re

    m = re.search(r", (\d+) partitions of (\d+) (?:nodes|poses)", line)
    assert m, line
    return int(m.group(1)), int(m.group(2))


def nodes_for_partitions(num_cus, Q, tile, consts, partitions, N):
    """N if the plan cuts it into `partitions` partitions on this chip (256 CUs: the sizes the tests name), else the smallest node
    count, in steps of a quarter of the least partition, that it does"""
    few_max, min_part, max_part = consts
    if plan(num_cus, Q, N, tile, few_max, min_part, max_part)[2] == partitions:
        return N
    for n in range(1, max_part * min_part * 4, min_part // 4):
        if plan(num_cus, Q, n, tile, few_max, min_part, max_part)[2] == partitions:
            return n
    raise AssertionError("no node count gives %d partitions on %d CUs" % (partitions, num_cus))
