/* ccmp_dense.h — dense solution paths: PathGeometric::interpolate as ConstrainedProblem::solveOnce runs it between the path search and
 * <obj>_path.txt (ConstrainedPlanningCommon.cpp:207-222), one rule text for host and device.  The kernels of ccmp_kernels_dense.hip and
 * the host code of ccmp_dense.cpp (the continuation loop, ccmp_dense_layout_ref, ccmp_dense_arc_ref) both compile it; the shortcut,
 * smooth and retime units include it for the open / stored rule, the arc bracket and the two helpers of their kernel files.
 *
 * Input: F paths of waypoint rows, path f with L = path_len[f] waypoints w_0 .. w_{L-1} and max(L - 1, 0) segments.
 *
 *   segment list   G_i = the state list of ONE uninterrupted jy_ProjectedStateSpace::discreteGeodesic(w_i, w_{i+1}, interpolate = true)
 *                  (jy_ProjectedStateSpace.cpp:32-96): n_i >= 1 states, G_i[0] = w_i; seg_ok[i] its return value, seg_newton[i] its Newton
 *                  total.  A traversal is cut into extend calls by list length (chunk_states) or round budget; first call + continuations
 *                  are one traversal bit for bit (ccmp_geodesic_batch_ex with carry_in / carry_out).  The call of a segment is OPEN after an
 *                  extend call iff n_states > chunk_states (list full) or ok == 2 (budget spent); it STORED min(n_states, chunk_states)
 *                  rows; a first call contributes all of them, a continuation all but row 0 (the state it started from) — possibly none.
 *   reference      flags = 0: the rows of path f are w_0, G_0, w_1, G_1, .., w_{L-2}, G_{L-2}, w_{L-1}: sum (1 + n_i) + 1 rows, every w_i
 *   layout         with i < L - 1 twice in a row, as PathGeometric::interpolate followed by printAsMatrix writes them.  L == 1: one row.
 *                  L == 0: none.
 *   distinct       CCMP_DENSE_DISTINCT: G_0, G_1, .., G_{L-2}, w_{L-1}: sum n_i + 1 rows.
 *   layout
 *   unreached      a segment with seg_ok = 0 contributes the rows it has; the next waypoint follows (a jump, as in the reference's file).
 *   offsets        paths are packed one after another; path_first[f] = the first row of path f, path_first[F] = the row count;
 *                  seg_first[f][i] = the first row of G_i, -1 for a slot without a segment.
 *   arc            arc[path_first[f]] = +0.0, arc[r] = fl(arc[r-1] + d(row[r-1], row[r])) within a path, d = the joint distance
 *                  (ccmp_graph.h: graph_joint_dist = ccmp_joint_distance); length[f] = the arc of the path's last row, +0.0 for an empty
 *                  path.  A duplicated row adds exactly +0.0: both layouts carry the same arcs at corresponding rows.
 *   arc bracket    arcs s[0 .. n) of a path's rows, monotone, n >= 2, and a target arc 0 < h <= s[n-1]: k = the smallest k >= 1 with
 *                  s[k] >= h, by bisection (no serial chain); t = (h - s[k-1]) / (s[k] - s[k-1]), one IEEE division; lower =
 *                  (h - s[k-1]) <= (s[k] - h).  s[k] > s[k-1] always holds (s[k-1] < h <= s[k]), so a +0.0 step — a duplicated row — is
 *                  never the bracket.  The smoothing's midpoint (ccmp_smooth.h, h = half the arc) and the resampling's targets are this.
 *   clearance      per path over clearance[r] (ccmp_clearance_batch of row r): min_clear = the smallest value, min_row = the first row
 *   summary        attaining it, first_blocked = the first row with clearance < margin (-1: none).  A NaN never attains a minimum and
 *                  is never below a margin.  Empty path: +inf, -1, -1. */
#ifndef CCMP_DENSE_H
#define CCMP_DENSE_H
#include <stddef.h>
#include <stdint.h>

#include "../../include/ccmp.h"
#include "ccmp_graph.h"

namespace ccmp {

/* the call of a segment did not reach the traversal's end: a continuation is due */
CCMP_HD bool dense_open(int32_t n_states, uint8_t ok, int chunk_states) { return n_states > chunk_states || ok == 2; }

/* rows the call stored in its list */
CCMP_HD int32_t dense_stored(int32_t n_states, int chunk_states) { return n_states < chunk_states ? (n_states < 0 ? 0 : n_states) : chunk_states; }

/* rows a path of L waypoints has before its segment i's list begins, given the list lengths before it have been summed into `before`;
 * and the whole path's row count given the sum over all its segments */
CCMP_HD int64_t dense_seg_first(int i, int64_t before, int distinct) { return before + (distinct ? 0 : (int64_t)i + 1); }
CCMP_HD int64_t dense_path_rows(int L, int64_t states, int distinct) { return L <= 0 ? 0 : states + 1 + (distinct ? 0 : (int64_t)L - 1); }

/* one step of the arc's serial chain */
CCMP_HD double dense_arc_step(double arc_prev, double d) { return arc_prev + d; }

/* The arc bracket of the target h on s[0 .. n).  No test of its own: the rule defines it for n >= 2 and 0 < h <= s[n-1], and the callers
 * decide what they hand it (smooth_bracket also comes with h == +0.0, half of the smallest denormal: every s[mid] >= h, so k = 1). */
CCMP_HD void arc_bracket(const double *s, int n, double h, int *k_out, double *t_out, bool *lower)
{
  int lo = 1, hi = n - 1; /* s[hi] >= h */
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (s[mid] >= h) hi = mid; else lo = mid + 1;
  }
  const double below = h - s[lo - 1], above = s[lo] - h;
  *k_out = lo;
  *t_out = below / (s[lo] - s[lo - 1]);
  *lower = below <= above;
}

/* the clearance summary's order: (value, row) ascending; a NaN is never a candidate */
CCMP_HD bool dense_lower(double va, int32_t ra, double vb, int32_t rb) { return va < vb || (va == vb && ra < rb); }

/* Items packed path after path: the path whose range holds item g.  key(a) = path a's first item, ascending over a < n (n >= 1);
 * the last a with key(a) <= g, 0 when there is none.  The array form reads the keys from first[0 .. n). */
template <class Key> CCMP_HD unsigned int path_of(unsigned int n, long long g, Key key)
{
  unsigned int lo = 0, hi = n - 1;
  while (lo < hi) {
    const unsigned int mid = lo + (hi - lo + 1) / 2;
    if (key(mid) <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}
CCMP_HD unsigned int path_of(const int32_t *first, unsigned int n, long long g) { return path_of(n, g, [first](unsigned int a) { return (long long)first[a]; }); }

/* the grid of a launch over n items, per_block of them to a block (host side of the four path kernel units) */
static inline unsigned int blocks_of(size_t n, size_t per_block) { return (unsigned int)((n + per_block - 1) / per_block); }

/* One piece of the result: `count` rows of 14 doubles from src to row dest.  A waypoint copy has its = nullptr; a piece of an extend
 * call's list adds that call's Newton count (*its) to seg_newton[slot] — integer additions, in any order the same total. */
struct dense_chunk {
  const double *src;
  const int32_t *its;
  int32_t count, dest, slot, pad;
};

/* An open segment of one extend call.  Round 0 (prev < 0): from = waypoint `slot`, to = waypoint slot + 1 of path_joints seen as rows
 * [F * max_len][14], no carry.  Continuation: from = row `last` of list `prev` of the previous call, carry = that call's carry row. */
struct dense_open_seg {
  int32_t slot, prev, last, pad;
};

}  // namespace ccmp

#endif /* CCMP_DENSE_H */
