/* ccmp_setpoints.h — controller-rate setpoints and an execution audit for timed paths: what stands between ccmp_path_timestamps and the
 * robot.  The reference hands positions-only points to its trajectory controller (scripts/execute_path.py:96-110): a linear blend between
 * rows with a velocity jump at every row.  One rule text for host and device: the kernels of ccmp_kernels_setpoints.hip and the host code of
 * ccmp_setpoints.cpp (ccmp_setpoints_ref, ccmp_setpoint_tangents_ref) both compile it with -ffp-contract=off, and it holds NO fused
 * operation: every function below is one rounding per written operation, in the written order, so plain Python floats restate it.
 * Division is IEEE division and the square root is ccmp_sqrt (ccmp_detmath.h), as in the retime unit.
 *
 * Inputs: packed rows [total_rows][14] with path_first [F + 1], stamps time [total_rows] (ccmp_path_timestamps' or any caller's), limits
 * vmax[14], amax[14] finite and > 0, period > 0 finite, max_ticks >= 2.  Path f has rows r_0 .. r_{R-1} and stamps t_0 .. t_{R-1}.
 *
 *   status         tested in this order: EMPTY R == 0 (device form: also a range that is negative, decreasing or beyond total_rows, never
 *                  read); NONFINITE a coordinate or a stamp of the path is not finite; UNORDERED t_0 != 0, or some t_{i+1} < t_i, or
 *                  t_{i+1} == t_i while rows i and i + 1 differ in a coordinate; POINT R == 1 or D = t_{R-1} is not > 0 (one tick: q = r_0,
 *                  qd = 0, tau = +0.0); FULL N > max_ticks or the count is beyond INT32_MAX (no tick); else OK, N ticks.
 *   ticks          N = 1 + (int64)ceil(D / period), at least 2.  tau_0 = +0.0, tau_{N-1} = D, 0 < j < N-1: tau_j = min(fl((double)j period), D).
 *   tangents       PCHIP (Fritsch-Butland), at rest at both ends.  h_i = t_{i+1} - t_i, d_i[c] = r_{i+1}[c] - r_i[c] (the plain difference,
 *                  as in the time stamps), m_i[c] = d_i[c] / h_i when h_i > 0, else +0.0.  w_0 = w_{R-1} = +0.0; interior: w_i[c] = +0.0
 *                  unless m_{i-1}[c] m_i[c] > 0, else w_i[c] = (a + b) / (a / m_{i-1}[c] + b / m_i[c]), a = 2 h_i + h_{i-1}, b = h_i + 2 h_{i-1}.
 *   interior tick  k = the smallest k >= 1 with t_k >= tau_j by arc_bracket (ccmp_dense.h) on the stamps; t_{k-1} < tau_j <= t_k, so the
 *                  bracket has positive width even where stamps repeat.  h = t_k - t_{k-1}, u = (tau_j - t_{k-1}) / h (the bracket's own
 *                  quotient).  Per joint, a = r_{k-1}, d = r_k - r_{k-1}, wa = w_{k-1}, wb = w_k:
 *                    q  = a + (u u (3 - 2u)) d + h (u (1-u)) ((1-u) wa - u wb)
 *                    qd = (6 u (1-u)) d / h + ((1-u)(1-3u)) wa + (u (3u-2)) wb
 *                  in the operation order of setpoint_q / setpoint_qd below.  Ticks 0 and N-1 are copies of r_0 and r_{R-1} with qd = +0.0.
 *   audit          per path, over its ticks j (a NaN is never a contributor; every maximum / minimum is taken under the total order
 *                  "(value, tick)", so no evaluation order can change a bit): speed = max_{j,c} |qd_j[c]| / vmax_c; acceleration =
 *                  max_{j,c} (|qd_{j+1}[c] - qd_j[c]| / (tau_{j+1} - tau_j)) / amax_c over intervals of positive width, at the interval's left
 *                  tick; max |dp| and max angle = the components of the constraint gap f; the smallest clearance; ties go to the smallest
 *                  tick; a peak without contributor is +0.0 (clearance: +inf) at tick -1.  n_off = ticks isSatisfied refuses, n_below =
 *                  ticks with clearance < margin.  stretch = max(1, speed, sqrt(acceleration)).
 *
 * Setpoints are NOT projected: a projection moves a point by up to the projector's tolerance, differently from tick to tick; divided by
 * dt^2 = 1e-6 that is acceleration noise of order 1e3 rad/s^2.  The knob for the gap is the resample spacing; the audit tells whether it
 * is fine enough.
 *
 * What the rule guarantees by construction: the tangent choice keeps every cubic piece monotone, so an interior q_j[c] lies between
 * r_{k-1}[c] and r_k[c] up to the rounding of setpoint_q — rows within the joint bounds command nothing outside them; the trajectory starts
 * and ends at rest on r_0 and r_{R-1}; tau is non-decreasing and ends exactly at D.  qd is the exact derivative of a C1 piecewise cubic,
 * so the acceleration figure is the MEAN acceleration over a tick interval, bounded by the interpolant's own second derivative, not a
 * noisy second difference of positions.  stretch is a report: the tick grid of a stretched call is another grid and nothing is claimed
 * for it. */
#ifndef CCMP_SETPOINTS_H
#define CCMP_SETPOINTS_H
#include <stdint.h>

#include "../../include/ccmp.h"
#include "ccmp_dense.h"
#include "ccmp_detmath.h"

namespace ccmp {

enum : int { kSetpointsOk = CCMP_SETPOINTS_OK, kSetpointsEmpty = CCMP_SETPOINTS_EMPTY, kSetpointsNonFinite = CCMP_SETPOINTS_NONFINITE,
             kSetpointsUnordered = CCMP_SETPOINTS_UNORDERED, kSetpointsPoint = CCMP_SETPOINTS_POINT, kSetpointsFull = CCMP_SETPOINTS_FULL };
enum : int { kPeakSpeed = 0, kPeakAcc = 1, kPeakDp = 2, kPeakAngle = 3, kPeakClearance = 4, kPeaks = 5 };

/* The limits of a call, checked on the host and handed to the kernels by value */
struct setpoint_limits {
  double vmax[14], amax[14];
};

CCMP_HD bool setpoint_finite(double v) { return v - v == 0.0; }

/* N of a path with D > 0; -1 beyond INT32_MAX (FULL) */
CCMP_HD int64_t setpoint_count(double D, double period)
{
  const double c = __builtin_ceil(D / period);
  if (!(c < 2147483647.0)) return -1;
  const int64_t n = 1 + (int64_t)c;
  return n < 2 ? 2 : n; /* (a quotient that underflowed to zero) */
}

/* what is left of the status order once the scan of a path with R >= 1 rows has answered `nonfinite` and `unordered`; *ticks = its ticks */
CCMP_HD int setpoint_status(bool nonfinite, bool unordered, int64_t R, double D, double period, int max_ticks, int32_t *ticks)
{
  *ticks = 0;
  if (nonfinite) return kSetpointsNonFinite;
  if (unordered) return kSetpointsUnordered;
  if (R == 1 || !(D > 0.0)) { *ticks = 1; return kSetpointsPoint; }
  const int64_t n = setpoint_count(D, period);
  if (n < 0 || n > (int64_t)max_ticks) return kSetpointsFull;
  *ticks = (int32_t)n;
  return kSetpointsOk;
}

/* interval i of a path is out of order: its stamps decrease, or repeat while `moved` (rows i and i + 1 differ in a coordinate) */
CCMP_HD bool setpoint_unordered(double ta, double tb, bool moved) { return tb < ta || (tb == ta && moved); }

/* tau_j of an interior tick */
CCMP_HD double setpoint_tau(int64_t j, double period, double D)
{
  const double t = (double)j * period;
  return D < t ? D : t;
}

/* m_i[c] */
CCMP_HD double setpoint_slope(double ra, double rb, double h)
{
  const double d = rb - ra;
  return h > 0.0 ? d / h : 0.0;
}

/* w_i[c] of an interior row: hp = h_{i-1}, h = h_i, mp = m_{i-1}[c], m = m_i[c] */
CCMP_HD double setpoint_tangent(double hp, double h, double mp, double m)
{
  if (!(mp * m > 0.0)) return 0.0;
  const double h2 = 2.0 * h, hp2 = 2.0 * hp;
  const double a = h2 + hp, b = h + hp2;
  const double num = a + b;
  const double qa = a / mp, qb = b / m;
  const double den = qa + qb;
  return num / den;
}

/* q of an interior tick in a bracket of width h at parameter u */
CCMP_HD double setpoint_q(double ra, double rb, double wa, double wb, double h, double u)
{
  const double d = rb - ra, v = 1.0 - u;
  const double uu = u * u, u2 = 2.0 * u;
  const double s3 = 3.0 - u2;
  const double s = uu * s3;
  const double p = s * d;
  const double uv = u * v;
  const double huv = h * uv;
  const double ea = v * wa, eb = u * wb;
  const double e = ea - eb;
  const double bend = huv * e;
  const double lin = ra + p;
  return lin + bend;
}

/* qd of the same tick */
CCMP_HD double setpoint_qd(double ra, double rb, double wa, double wb, double h, double u)
{
  const double d = rb - ra, v = 1.0 - u;
  const double u6 = 6.0 * u, u3 = 3.0 * u;
  const double g = u6 * v;
  const double gd = g * d;
  const double t1 = gd / h;
  const double c1 = 1.0 - u3;
  const double ca = v * c1;
  const double t2 = ca * wa;
  const double c2 = u3 - 2.0;
  const double cb = u * c2;
  const double t3 = cb * wb;
  const double t12 = t1 + t2;
  return t12 + t3;
}

/* Tick j of the N of an OK path on its stamps t [R], D = t[R-1]: *tau, and for j >= 1 the bracket (*k - 1, *k) of tau with its parameter *u.
 * Tick 0 has tau = +0.0 and no bracket (*k = 0); the last tick has tau = D and the bracket D lies in, for a caller that folds by row
 * interval.  False: the rule's own precondition of the bracket fails (an OK path meets it) and no stamp has been read.  The one text of
 * "a tick of the interpolant" for the setpoints, fit and jerk units, on the device and in their _ref forms. */
CCMP_HD bool setpoint_bracket(const double *t, int R, int64_t j, int64_t N, double period, double D, double *tau, int *k, double *u)
{
  *tau = 0.0;
  *k = 0;
  *u = 0.0;
  if (j <= 0) return true;
  const double at = j >= N - 1 ? D : setpoint_tau(j, period, D);
  *tau = at;
  if (!(at > 0.0) || !(at <= D) || R < 2) return false;
  bool lower;
  arc_bracket(t, R, at, k, u, &lower);
  return true;
}

/* one joint's q and qd at the parameter u of the bracket (k - 1, k): r and w are the path's rows and tangents from that joint's element of
 * row 0 on, t the path's stamps.  A caller that needs one of the two hands the other a dummy: the text is inlined and the dead half goes. */
CCMP_HD void setpoint_joint(const double *r, const double *w, const double *t, int k, double u, double *q, double *qd)
{
  const double h = t[k] - t[k - 1];
  const size_t a = (size_t)(k - 1) * 14, b = a + 14;
  *q = setpoint_q(r[a], r[b], w[a], w[b], h, u);
  *qd = setpoint_qd(r[a], r[b], w[a], w[b], h, u);
}

/* one joint's shares of the speed and acceleration ratios; width = tau_{j+1} - tau_j > 0 */
CCMP_HD double setpoint_speed(double qd, double vmax) { return ccmp_abs(qd) / vmax; }
CCMP_HD double setpoint_acc(double qd_a, double qd_b, double width, double amax)
{
  const double dv = ccmp_abs(qd_b - qd_a);
  const double acc = dv / width;
  return acc / amax;
}

/* The order of a peak: (value, tick), larger values first (clearance: smaller), then the smaller tick; tick < 0 = no contributor yet */
CCMP_HD bool setpoint_higher(double v, int32_t j, double bv, int32_t bj) { return v == v && (bj < 0 || v > bv || (v == bv && j < bj)); }
CCMP_HD bool setpoint_lower(double v, int32_t j, double bv, int32_t bj) { return v == v && (bj < 0 || v < bv || (v == bv && j < bj)); }

CCMP_HD double setpoint_stretch(double speed, double acc)
{
  const double r = ccmp_sqrt(acc);
  double s = 1.0;
  if (speed > s) s = speed;
  if (r > s) s = r;
  return s;
}

}  // namespace ccmp

#endif /* CCMP_SETPOINTS_H */
