/* ccmp_shortcut.h — shortcut solution paths: the removal of interior vertices (OMPL's PathSimplifier::reduceVertices, which the reference
 * never calls) as one batch of checkMotion tests and one search, one rule text for host and device.  The kernels of
 * ccmp_kernels_shortcut.hip and the host code of ccmp_shortcut.cpp (the tile and continuation loops, ccmp_shortcut_select_ref,
 * ccmp_shortcut_pairs_ref) both compile it: they cannot differ in a bit.
 *
 * Input: F paths of waypoint rows, path f with L = path_len[f] waypoints w_0 .. w_{L-1}.
 *
 *   pair slot      (i, j) with 0 <= i, j < L, j - i >= 2 and j - i <= max_span (0: every span), in (f, i, j) order.  Their number
 *                  depends on L and max_span alone: shortcut_pairs_before counts them in closed form, which is what lets a tile of the
 *                  enumeration start and end inside a path.
 *   candidate      a pair slot whose two rows are finite in all 14 coordinates.  Only candidates are tested.
 *   test           ONE uninterrupted checkMotion(w_i, w_j): isSatisfied(w_j), then discreteGeodesic(w_i, w_j) — the extend step with
 *                  check_target on the first call, continued while dense_open (ccmp_dense.h) says so.  pair_ok = its return value,
 *                  pair_states = its list length, pair_newton = its Newton total: sums of what each extend call contributed (a first
 *                  call all its stored rows, a continuation all but row 0), integer additions.  No candidate: 0, 0, 0.
 *   admitted edge  i -> j: j == i + 1 (the roadmap's own edge, never tested) or pair_ok[i][j] == 1.
 *   weight         w(i, j) = graph_joint_dist(w_i, w_j) (ccmp_graph.h: what commit stores as motionCost).
 *   selection      ccmp_path.h's rule on this DAG from source 0: d[0] = +0.0; d[j] = min over admitted i < j of the passing candidates
 *                  fl(d[i] + w(i, j)) (path_candidate: d[i] finite, w >= 0, sum finite), +inf without one; hops[j] = the least
 *                  hops[i] + 1 over tight i; pred[j] = the smallest tight i with hops[i] == hops[j] - 1.  Every edge goes forwards, so one
 *                  sweep over j is exact, and (d, hops, pred)[j] is the lexicographic minimum of (candidate, hops[i], i) over the
 *                  passing i: shortcut_better is that order.
 *   result         kept = the walk of pred from L - 1 written forwards (hops[L - 1] + 1 entries), -1 behind it; cost_in = the
 *                  left-to-right fl sum of the adjacent weights; cost_out = d[L - 1].  L == 1: kept {0}, costs +0.0.  L == 0: nothing,
 *                  costs +0.0.  d[L - 1] == +inf (an adjacent weight NaN or infinite): identity kept, cost_out = +inf. */
#ifndef CCMP_SHORTCUT_H
#define CCMP_SHORTCUT_H
#include <stdint.h>

#include "../../include/ccmp.h"
#include "ccmp_dense.h"
#include "ccmp_graph.h"
#include "ccmp_path.h"

namespace ccmp {

/* the widest span a path of L waypoints has under max_span */
CCMP_HD int shortcut_span(int L, int max_span) { return (max_span == 0 || max_span > L - 1) ? L - 1 : max_span; }

/* pair slots of one path with a first index below i (0 <= i <= L): first index i' has max(min(L - 1 - i', S) - 1, 0) of them */
CCMP_HD long long shortcut_pairs_before(int L, int max_span, int i)
{
  if (L < 3) return 0;
  const long long S = shortcut_span(L, max_span);
  if (S < 2) return 0;
  if (i > L - 2) i = L - 2;            /* first indices L - 2 and L - 1 have none */
  const long long m = (long long)L - S; /* first indices 0 .. m - 1 have the full S - 1 */
  if (i <= m) return (long long)i * (S - 1);
  const long long t = (long long)i - m; /* then S - 2, S - 3, .. */
  return m * (S - 1) + t * (S - 2) - t * (t - 1) / 2;
}

CCMP_HD long long shortcut_pair_count(int L, int max_span) { return shortcut_pairs_before(L, max_span, L); }

/* pair slot r (0 <= r < shortcut_pair_count) of a path: its (i, j).  A bisection on the closed form: at most 11 steps for L <= 1024. */
CCMP_HD void shortcut_pair_of(int L, int max_span, long long r, int *i_out, int *j_out)
{
  int lo = 0, hi = L - 2; /* the largest i with pairs_before(i) <= r */
  while (lo < hi) {
    const int mid = lo + (hi - lo + 1) / 2;
    if (shortcut_pairs_before(L, max_span, mid) <= r) lo = mid; else hi = mid - 1;
  }
  *i_out = lo;
  *j_out = lo + 2 + (int)(r - shortcut_pairs_before(L, max_span, lo));
}

CCMP_HD bool shortcut_row_finite(const double *row)
{
  bool ok = true;
  for (int c = 0; c < 14; c++) ok = ok && (row[c] - row[c] == 0.0); /* false for NaN and for either infinity */
  return ok;
}

CCMP_HD bool shortcut_admitted(int i, int j, uint8_t ok) { return j == i + 1 || ok == 1; }

/* (candidate, hops of the parent, parent) in lexicographic order; candidates that pass are >= +0.0 and never NaN */
CCMP_HD bool shortcut_better(double ca, int32_t ha, int32_t ia, double cb, int32_t hb, int32_t ib)
{
  return ca < cb || (ca == cb && (ha < hb || (ha == hb && ia < ib)));
}

/* The best parent of a vertex so far: its candidate, the parent's hops and the parent.  Without one: (+inf, kPathNoHops, kShortcutNoPred),
 * behind every passing candidate in the order above. */
constexpr int32_t kShortcutNoPred = 0x7fffffff;
struct shortcut_best {
  double d;
  int32_t parent_hops, pred;
};

CCMP_HD shortcut_best shortcut_none() { return shortcut_best{__builtin_inf(), kPathNoHops, kShortcutNoPred}; }

/* fold parent i (distance di, hops hi) over an admitted edge of weight w into the best of a vertex */
CCMP_HD void shortcut_relax(shortcut_best *b, int i, double di, int32_t hi, double w)
{
  double c;
  if (hi >= kPathNoHops || !path_candidate(di, w, &c)) return;
  if (shortcut_better(c, hi, i, b->d, b->parent_hops, b->pred)) *b = shortcut_best{c, hi, i};
}

/* the better of two partial results (a block's lanes each fold the parents they own, in any split the same minimum) */
CCMP_HD void shortcut_merge(shortcut_best *b, const shortcut_best &o)
{
  if (shortcut_better(o.d, o.parent_hops, o.pred, b->d, b->parent_hops, b->pred)) *b = o;
}

/* An open pair of a continuation call: `prev` = its index in the previous extend call of the tile, `last` = the last row that call stored
 * in its list, `slot` = its slot in the tile. */
struct shortcut_open {
  int32_t prev, last, slot, pad;
};

}  // namespace ccmp

#endif /* CCMP_SHORTCUT_H */
