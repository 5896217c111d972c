/* ccmp_rrtc.h — RRT-Connect on the roadmap store (include/ccmp.h: ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree): the decisions that are
 * neither a sampler, a traversal nor a graph call, one text for host and device.  The kernels of ccmp_kernels_rrtc.hip and the *_ref
 * forms of ccmp_rrtc.cpp both compile it: they cannot differ in a bit.  include/ccmp.h states the whole cycle and its differences from
 * OMPL's RRTConnect; what is stated HERE is
 *
 *   membership   v is in a side's tree iff label[v] equals the label of one of the side's <= 8 roots (a root outside the store gives none)
 *   nearest      the smallest (graph_joint_dist(joints[v], query), v) over the tree: ccmp_graph.h's distance (the k-NN's FMA chain) and
 *                graph_closer's order; a NaN distance is below nothing
 *   the arc      s_0 = 0, s_j = fl(s_{j-1} + step_j) over the listed states IN LIST ORDER (a serial fold: the order is the rule's); j* =
 *                the largest j with s_j <= range (the <= keeps a row that lands exactly on the range)
 *   extend       rrtc_extend: TRAPPED / ADVANCED (listed state j, at least 1) / REACHED (the sample row) / UNSETTLED
 *   connect      rrtc_connect: NOTHING / ADDED (the last stored state) / JOINED
 *   FULL         size + 2 width > max_vertices
 *   the solution ccmp_plan.h's, one text for both planners: the first pair (s, g), s major and g minor, whose labels agree
 *
 * No arithmetic here rounds differently on host and device: comparisons, sums of two doubles, integer sums. */
#ifndef CCMP_RRTC_H
#define CCMP_RRTC_H
#include "../../include/ccmp.h"
#include "ccmp_detmath.h"

namespace ccmp {

CCMP_HD bool rrtc_full(unsigned long long size, int width, unsigned long long max_vertices)
{
  return size + 2ull * (unsigned long long)width > max_vertices;
}

/* the labels of a side's roots in eight fixed slots (no slot is indexed by a value: they stay in registers); a slot without a root, or
 * with a root outside the store, holds -1, which is no vertex's label.  Returns the number of slots that hold a label. */
CCMP_HD int rrtc_root_labels(const int32_t *roots, int n_roots, const int32_t *labels, unsigned long long N, int32_t lab[CCMP_RRTC_MAX_ROOTS])
{
  int n = 0;
  for (int i = 0; i < CCMP_RRTC_MAX_ROOTS; i++) {
    int32_t l = -1;
    if (i < n_roots) {
      const int32_t r = roots[i];
      if (r >= 0 && (unsigned long long)r < N) { l = labels[r]; n++; }
    }
    lab[i] = l;
  }
  return n;
}

CCMP_HD bool rrtc_in_tree(int32_t label, const int32_t lab[CCMP_RRTC_MAX_ROOTS])
{
  bool in = false;
  for (int i = 0; i < CCMP_RRTC_MAX_ROOTS; i++) in = in || (label >= 0 && lab[i] == label);
  return in;
}

/* the arc's fold over the listed states */
struct rrtc_arc {
  double s;   /* s_i of the last step taken */
  double s_j; /* s_j of j */
  int j;      /* the largest index with s_j <= range so far; 0: `from` */
  int nan;
};
CCMP_HD void rrtc_arc_begin(rrtc_arc *a) { a->s = 0.0; a->s_j = 0.0; a->j = 0; a->nan = 0; }
CCMP_HD void rrtc_arc_step(rrtc_arc *a, int i, double step, double range)
{
  a->s = a->s + step;
  if (a->s != a->s) a->nan = 1;
  else if (a->s <= range) { a->j = i; a->s_j = a->s; }
}

/* step 2's decision of one sample.  m listed states (min(n_states, max_states)), their arc, d = the nearest distance.  *row = the
 * listed state that becomes the vertex, -1: the sample row itself (REACHED) or no vertex. */
CCMP_HD int32_t rrtc_extend(int32_t n_states, int max_states, uint8_t ok, double d, double range, const rrtc_arc *a, int32_t *row)
{
  *row = -1;
  const int m = n_states < 0 ? 0 : n_states > max_states ? max_states : n_states;
  if (a->nan || d != d || !(range > 0.0) || m < 1) return CCMP_RRTC_TRAPPED;
  const bool cut = n_states > max_states || ok == 2;
  if (d <= range) return ok == 1 ? CCMP_RRTC_REACHED : cut ? CCMP_RRTC_UNSETTLED : CCMP_RRTC_TRAPPED;
  if (m < 2) return CCMP_RRTC_TRAPPED;
  const int j = a->j < 1 ? 1 : a->j;
  if (cut && j == m - 1 && a->j >= 1) return CCMP_RRTC_UNSETTLED;
  *row = j;
  return CCMP_RRTC_ADVANCED;
}

/* step 3's decision of one produced vertex v: gap = graph_joint_dist(last stored state, v), NaN without a listed state */
CCMP_HD int32_t rrtc_connect(int32_t n_states, int max_states, uint8_t ok, double gap, int32_t *row)
{
  *row = -1;
  const int m = n_states < 0 ? 0 : n_states > max_states ? max_states : n_states;
  if (m < 1 || gap != gap) return CCMP_RRTC_CONNECT_NOTHING;
  if (ok == 1) return CCMP_RRTC_CONNECT_JOINED;
  if (m < 2) return CCMP_RRTC_CONNECT_NOTHING;
  *row = m - 1;
  return CCMP_RRTC_CONNECT_ADDED;
}

}  // namespace ccmp

#endif /* CCMP_RRTC_H */
