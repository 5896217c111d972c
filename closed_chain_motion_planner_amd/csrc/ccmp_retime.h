/* ccmp_retime.h — resample a dense solution path at even arc and give packed rows time stamps under joint velocity and acceleration
 * limits: PathGeometric::interpolate(count) with this project's blend, and what the reference's scripts/execute_path.py:105-108 replaces
 * by "the same time slice for every printed row".  One rule text for host and device: the kernels of ccmp_kernels_retime.hip and the host
 * code of ccmp_retime.cpp (ccmp_path_timestamps_ref, ccmp_arc_bracket_ref, ccmp_resample_targets_ref, the count of ccmp_path_resample)
 * both compile it with -ffp-contract=off -DCCMP_USE_FMA: the only fused operations are the ones written with CCMP_FMA (the blend's and
 * the joint distance's), and they cannot differ in a bit.
 *
 *   arc bracket    (k, t, lower) of a target arc 0 < h <= s[n-1] on monotone arcs s[0 .. n), n >= 2: ccmp_dense.h states it and
 *                  arc_bracket there is its text, shared with the smoothing's midpoint; ccmp_arc_bracket_ref answers it on the host.
 *
 *   resample       a dense path (ccmp_dense.h, either layout) has rows r_0 .. r_{R-1} and arcs s, T = s[R-1].  Status, tested in this order:
 *                  EMPTY R == 0 (no row out); BROKEN a segment of the path has seg_ok == 0 (none); NONFINITE a row is not finite in all
 *                  14 coordinates (none); POINT not T > 0 (one row: r_0, COPIED); FULL N > max_rows (none); else OK, N rows.
 *                  N = count when count >= 2, else 1 + (int64)ceil(T / spacing) in IEEE double (at least 2; beyond INT32_MAX: FULL).
 *                  Row 0 = r_0 and row N-1 = r_{R-1}, COPIED.  For 0 < j < N-1: h_j = fl(fl((double)j / (double)(N-1)) * T); not h_j > 0:
 *                  r_0, DEGENERATE; else bracket h_j (fl(j / (N-1)) < 1, so h_j <= T), x = ccmp_joint_interpolate(r_{k-1}, r_k, t) per joint,
 *                  (y, ok) = project(x) in the problem's Jacobian mode; ok: y, PROJECTED; else r_{k-1} when lower, else r_k, FALLBACK.
 *                  The new rows carry arcs and a length by the dense arc rule, a kind per row and the four kind counts per path.
 *
 *   time stamps    packed rows of a path, R of them; the path parameter is the row index.  Limits vmax[14], amax[14] finite and > 0,
 *                  0 < beta < 1 = the share of the acceleration budget given to curvature.  Status: EMPTY (R == 0), NONFINITE, else OK.
 *                  R == 1: t_0 = +0.0.  Otherwise, with d_i[c] = r_{i+1}[c] - r_i[c] (i < R-1; the plain difference of the joint distance,
 *                  not the wrap of interpolate: dense rows are a delta apart):
 *                    V_i = min_c vmax_c / |d_i[c]|                       (a zero difference gives +inf)
 *                    x_0 = x_{R-1} = +0.0;  x_i = min(V_{i-1} V_{i-1}, V_i V_i, min_c fl(beta amax_c) / |d_i[c] - d_{i-1}[c]|)
 *                    A = min over i, c of fl((1 - beta) amax_c) / |d_i[c]|,  g = 2 A
 *                    y_i = min over k of e(i, k):  e(i, i) = x_i,  e(i, k) = fl(x_k + fl(g (double)|i - k|))
 *                    R >= 3: dt_i = 2 / (sqrt(y_i) + sqrt(y_{i+1}));   R == 2: dt_0 = 2 / sqrt(min(V_0 V_0, fl(0.5 g)))
 *                    t_0 = +0.0, t_{i+1} = fl(t_i + dt_i) left to right; duration = t_{R-1}
 *                  x is a ceiling on z = (index speed)^2 and y the largest profile under it whose slope is at most g.  Every min is over
 *                  finite values or +inf, never a NaN (a NONFINITE path is not computed), so the order in which a minimum is taken
 *                  cannot change a bit: the kernels reduce across lanes and with an integer atomic minimum on the bit pattern (the order
 *                  of non-negative doubles), the host form runs plain loops.  No window over k is used.
 *
 * What the rule guarantees by construction: y_i <= x_i (the k = i term); interval i's mean index speed 1 / dt_i = (sqrt(y_i) +
 * sqrt(y_{i+1})) / 2 <= V_i, since y_i, y_{i+1} <= V_i V_i — the velocity limit on every interval; |y_{i+1} - y_i| <= g up to the rule's
 * roundings (every term of y_i plus g bounds a term of y_{i+1}).  At the grid rows that is |q''| z <= beta amax and |q'| |z'| / 2 <=
 * (1 - beta) amax: a bound on the PROFILE.  It is NOT a bound on finite differences of the sampled trajectory. */
#ifndef CCMP_RETIME_H
#define CCMP_RETIME_H
#include <stdint.h>

#include "../../include/ccmp.h"
#include "ccmp_dense.h"
#include "ccmp_detmath.h"

namespace ccmp {

enum : int { kRetimeProjected = CCMP_SAMPLE_PROJECTED, kRetimeFallback = CCMP_SAMPLE_FALLBACK, kRetimeDegenerate = CCMP_SAMPLE_DEGENERATE,
             kRetimeCopied = CCMP_SAMPLE_COPIED, kRetimeKinds = 4, kRetimePending = 255 /* between the bracket and the pick: the projector decides */ };
enum : int { kRetimeOk = CCMP_RETIME_OK, kRetimeEmpty = CCMP_RETIME_EMPTY, kRetimeBroken = CCMP_RETIME_BROKEN, kRetimeNonFinite = CCMP_RETIME_NONFINITE,
             kRetimePoint = CCMP_RETIME_POINT, kRetimeFull = CCMP_RETIME_FULL };

/* The limits of a time-stamp call, checked on the host and handed to the kernels by value */
struct retime_limits {
  double vmax[14], amax[14], beta;
};

/* The row count of an OK path with T > 0: count mode or spacing mode; -1 beyond INT32_MAX (FULL).  Host only: the count sizes the result. */
static inline int64_t retime_count(double T, int count, double spacing)
{
  if (count >= 2) return count;
  const double c = __builtin_ceil(T / spacing);
  if (!(c < 2147483647.0)) return -1;
  const int64_t n = 1 + (int64_t)c;
  return n < 2 ? 2 : n; /* (a quotient that underflowed to zero) */
}

/* h_j of an interior row: two roundings */
CCMP_HD double retime_target(int64_t j, int64_t N, double T)
{
  const double u = (double)j / (double)(N - 1);
  return u * T;
}

CCMP_HD double retime_min(double a, double b) { return b < a ? b : a; }

/* one joint's three quotients: d = d_i[c], dp = d_{i-1}[c] */
CCMP_HD double retime_joint_v(double vmax, double d) { return vmax / ccmp_abs(d); }
CCMP_HD double retime_joint_curv(double beta, double amax, double d, double dp)
{
  const double b = beta * amax;
  return b / ccmp_abs(d - dp);
}
CCMP_HD double retime_joint_acc(double beta, double amax, double d)
{
  const double b = (1.0 - beta) * amax;
  return b / ccmp_abs(d);
}

/* the ceiling of an interior row from the joint minima: V_{i-1}, V_i and the curvature quotient */
CCMP_HD double retime_ceiling(double v_prev, double v, double curv) { return retime_min(retime_min(v_prev * v_prev, v * v), curv); }

/* e(i, k), k != i: dist = |i - k| */
CCMP_HD double retime_env_term(double xk, double g, int64_t dist)
{
  const double rise = g * (double)dist;
  return xk + rise;
}

CCMP_HD double retime_dt(double ya, double yb) { return 2.0 / (ccmp_sqrt(ya) + ccmp_sqrt(yb)); }
CCMP_HD double retime_dt_pair(double v0, double g) { return 2.0 / ccmp_sqrt(retime_min(v0 * v0, 0.5 * g)); }

CCMP_HD bool retime_finite(double v) { return v - v == 0.0; }

}  // namespace ccmp

#endif /* CCMP_RETIME_H */
