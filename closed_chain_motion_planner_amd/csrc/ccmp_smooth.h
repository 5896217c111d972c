/* ccmp_smooth.h — smooth solution paths: the structure of OMPL's PathSimplifier::smoothBSpline (subdivide, then move every original
 * vertex towards the middle of its two new neighbours), with this project's midpoint, one rule text for host and device.  The kernels
 * of ccmp_kernels_smooth.hip and the host code of ccmp_smooth.cpp (the pass loop, ccmp_smooth_mid_ref, ccmp_smooth_len_after) both
 * compile it: they cannot differ in a bit.  A pass is data-parallel as written: only the original vertices move, each reads only its two
 * new neighbours, and no pass moves a new neighbour — every segment and every interior vertex of every path is one batch per stage.
 *
 * Path f has L = path_len[f] waypoints w_0 .. w_{L-1}.
 *
 *   closed list    of a pair (a, b): the distinct dense rows of the two-waypoint path [a, b] (ccmp_dense.h): G = the list of ONE
 *                  uninterrupted discreteGeodesic(a, b, interpolate = true), then b; n >= 2 rows; arcs s_0 = +0.0,
 *                  s_k = fl(s_{k-1} + joint distance(row_{k-1}, row_k)).
 *   midpoint       mid(a, b): T = s_{n-1}, h = 0.5 T.  Not T > 0: mid = a (DEGENERATE).  Otherwise (k, t, lower) = the arc bracket of h
 *                  (ccmp_dense.h states it, once, for this unit and for ccmp_retime.h: a +0.0 step is never the bracket),
 *                  x = WrapperStateSpace::interpolate(row_{k-1}, row_k, t) (smooth_interpolate: the extend step's text), (y, ok) =
 *                  project(x).  ok: mid = y (PROJECTED).  Not ok: mid = row_{k-1} when lower, else row_k (FALLBACK).
 *                  The midpoint is the blend at exactly half the arc put back on the manifold, not the list state nearest to it: at the
 *                  planner's delta a list has one to seven states, so after one pass most list-state midpoints coincide with a waypoint
 *                  and later passes move the same vertices back and forth.
 *   one pass       on a path with L >= 3: m_i = mid(w_i, w_{i+1}) for every segment; for every interior i: t1 = mid(m_{i-1}, w_i),
 *                  t2 = mid(w_i, m_i), c_i = mid(t1, t2).  c_i is ACCEPTED iff checkMotion(m_{i-1}, c_i) and checkMotion(c_i, m_i) pass
 *                  (each isSatisfied(target), then one uninterrupted discreteGeodesic, forwards, as ccmp_shortcut.h; with a proxy scene the
 *                  scene form with the margin, and also clearance(m_{i-1}) >= margin and clearance(c_i) >= margin, a NaN refusing) —
 *                  otherwise it is REFUSED — and then joint distance(w_i, c_i) > min_change — otherwise it is BELOW.  The new path is
 *                  w_0, m_0, w_1', m_1, .., m_{L-2}, w_{L-1}: 2L - 1 vertices, w_i' = c_i if accepted, else w_i; u = the accepted vertices.
 *   loop           per path, in this order: a waypoint among the first L not finite in all 14 coordinates: stop 4, copied, nothing
 *                  traversed; L < 3: stop 0, copied; then while true: max_steps passes have run: stop 2; 2L - 1 > out_max_len: stop 3;
 *                  a pass; u == 0: stop 1 (that pass's subdivision is kept, as OMPL keeps it).  A path that has stopped takes no part in
 *                  later passes: its result is that of the path run alone.
 *   lengths        length_in / length_out = the left-to-right fl sum of adjacent joint distances; +0.0 for L < 2.
 *   stats          per path, five counts: midpoints projected, fallen back, degenerate; candidates refused, below min_change. */
#ifndef CCMP_SMOOTH_H
#define CCMP_SMOOTH_H
#include <stdint.h>

#include "../../include/ccmp.h"
#include "ccmp_dense.h"
#include "ccmp_graph.h"
#include "ccmp_shortcut.h"

namespace ccmp {

enum : int { kSmoothProjected = 0, kSmoothFallback = 1, kSmoothDegenerate = 2, kSmoothRefused = 3, kSmoothBelow = 4, kSmoothStats = 5 };
enum : int { kSmoothStopShort = 0, kSmoothStopStill = 1, kSmoothStopSteps = 2, kSmoothStopFull = 3, kSmoothStopNonFinite = 4 };

/* WrapperStateSpace::interpolate through KinematicChainSpace::interpolate (KinematicChain.h:145-171), one joint: the text of the extend
 * step (ccmp_geo_edge_body.inc, ccmp_row16_geo_body.inc; the oracle's orc_interpolate) */
CCMP_HD double smooth_interpolate(double fr, double tg, double tt) { return ccmp_joint_interpolate(fr, tg, tt); }

/* vertices of a path after `passes` passes (each L -> 2L - 1), saturating at INT32_MAX; L < 3 stays */
CCMP_HD int32_t smooth_len_after(int32_t L, int passes)
{
  if (L < 3) return L < 0 ? 0 : L;
  int64_t n = L;
  for (int s = 0; s < passes && n < 0x7fffffffLL; s++) n = 2 * n - 1;
  return n > 0x7fffffffLL ? 0x7fffffff : (int32_t)n;
}

/* The bracket of a closed list's half arc: arcs s[0 .. n), monotone.  Returns false for a degenerate list (not T > 0).  Otherwise the arc
 * bracket (ccmp_dense.h) of h = 0.5 T: *k_out, the blend parameter *t_out, and *lower true when the fallback is row k - 1. */
CCMP_HD bool smooth_bracket(const double *s, int n, int *k_out, double *t_out, bool *lower)
{
  *k_out = 0; *t_out = 0.0; *lower = true;
  if (n < 2 || !(s[n - 1] > 0.0)) return false;
  arc_bracket(s, n, 0.5 * s[n - 1], k_out, t_out, lower);
  return true;
}

/* the verdict on a candidate: 0 accepted, kSmoothRefused, kSmoothBelow */
CCMP_HD int smooth_verdict(uint8_t ok_in, uint8_t ok_out, bool has_scene, double clear_from, double clear_cand, double margin, double moved,
                           double min_change)
{
  if (ok_in != 1 || ok_out != 1) return kSmoothRefused;
  if (has_scene && !(clear_from >= margin && clear_cand >= margin)) return kSmoothRefused; /* a NaN refuses */
  if (!(moved > min_change)) return kSmoothBelow;
  return 0;
}

/* One active path of a pass: its index, its length before the pass, and the segments / interior vertices of the active paths before it */
struct smooth_path {
  int32_t f, L, seg_first, vert_first;
};

}  // namespace ccmp

#endif /* CCMP_SMOOTH_H */
