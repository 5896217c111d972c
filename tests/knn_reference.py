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
