/* ccmp_path.h — shortest paths on the roadmap graph: the planner's solution step (constructSolution, maybeConstructSolution,
 * constructApproximateSolution: stefanBiPRM.cpp:161-239, :480-603), one rule text for host and device.  The kernels of
 * ccmp_kernels_graph.hip (graph_path_*) and ccmp_graph_shortest_paths_ref (ccmp_roadmap.cpp) both compile it: they cannot differ in a bit.
 *
 * The graph is the store's: undirected edges uv[e] with weights w[e] (joint distances: >= 0, or NaN at a pose-only vertex); parallel
 * edges may occur.  All arithmetic is one IEEE double addition, fl(a + b).  For one source s:
 *
 *   candidate   over an edge {u, v} from u: c = fl(d[u] + w).  It PASSES iff d[u] is finite, w >= 0 and c is finite — a NaN never
 *               passes (an edge at a pose-only vertex), nor does a sum that overflowed: +inf means "unreached" and nothing else.
 *   distance    d = the least fixed point of d[s] = +0.0, d[v] = min over passing candidates into v; unreached: +inf.  fl(a + w) is
 *               non-decreasing in a and >= a for w >= 0, so the fixed point is unique: Dijkstra, Bellman-Ford in any relaxation order and
 *               atomicMin arriving in any order all reach it — a function of the edge set alone, bit for bit, with zero weights and
 *               absorbed weights (fl(d + w) == d) included.  Distances are >= +0.0 and never NaN: their order is the order of their
 *               bits as unsigned 64-bit integers, which is what lets the device relax with an integer atomicMin.
 *   tight edge  u -> v: the candidate from u passes and equals d[v].
 *   hops        hops[v] = the breadth-first level of v from s in the directed graph of tight edges (Dijkstra's tree consists of tight
 *               edges: every reached vertex has one); unreached: INT32_MAX.
 *   pred        pred[v] = the smallest u with a tight edge u -> v and hops[u] == hops[v] - 1; -1 for s and for an unreached vertex.
 *               Acyclic by construction (a rule on distances or indices would not be: a zero or absorbed weight lets two vertices be
 *               each other's predecessor).
 *   path        s -> t has hops[t] + 1 vertices, the walk of pred from t, written forwards; its cost d[t] is the left-to-right fl sum
 *               of its weights.  s == t: length 1, cost +0.0.  t unreached: length 0, cost +inf. */
#ifndef CCMP_PATH_H
#define CCMP_PATH_H
#include <stdint.h>
#include <string.h>

#include "../../include/ccmp.h"
#include "ccmp_detmath.h"

namespace ccmp {

constexpr int32_t kPathNoHops = 0x7fffffff; /* hops of an unreached vertex */

CCMP_HD uint64_t path_bits(double x)
{
  uint64_t u;
  memcpy(&u, &x, sizeof u);
  return u;
}

CCMP_HD double path_from_bits(uint64_t u)
{
  double x;
  memcpy(&x, &u, sizeof x);
  return x;
}

/* the candidate over an edge of weight w from an endpoint at distance du; false: it does not pass */
CCMP_HD bool path_candidate(double du, double w, double *c)
{
  const double s = du + w;
  *c = s;
  return du < __builtin_inf() && w >= 0.0 && s < __builtin_inf();
}

/* u -> v is tight: du = d[u], dv = d[v] */
CCMP_HD bool path_tight(double du, double w, double dv)
{
  double c;
  return path_candidate(du, w, &c) && c == dv;
}

/* u -> v is a tree candidate: tight, and u one level above v */
CCMP_HD bool path_parent(double du, int32_t hu, double w, double dv, int32_t hv) { return hu < kPathNoHops && hv == hu + 1 && path_tight(du, w, dv); }

}  // namespace ccmp

#endif /* CCMP_PATH_H */
