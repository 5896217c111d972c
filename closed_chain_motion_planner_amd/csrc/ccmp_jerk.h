/* ccmp_jerk.h — jerk-bounded setpoints: a moving window over the setpoints rule's interpolant, with a jerk audit; the unit beside
 * ccmp_path_setpoints for a controller that limits jerk as well as speed and acceleration (a Panda: 7500 .. 10000 rad/s^3, and an interface
 * that refuses an acceleration that jumps at its 1 kHz rate).  ccmp_path_setpoints commands a C1 piecewise cubic: its acceleration jumps at
 * every row, and ccmp_path_fit_timestamps cannot repair that.  One rule text for host and device: the kernels of ccmp_kernels_jerk.hip and
 * ccmp_jerk_setpoints_ref (ccmp_jerk.cpp) both compile it with -ffp-contract=off, and it holds NO fused operation: one rounding per written
 * operation in the written order, IEEE division — plain Python floats restate it.  Status, tick count, tau of an interior tick, tangents,
 * q, qd, the speed and acceleration shares, the order of a peak and the bracket are ccmp_setpoints.h's and ccmp_dense.h's, unchanged.
 *
 * Inputs: packed rows [total_rows][14] with path_first [F + 1], stamps time [total_rows]; vmax[14], amax[14], jmax[14] finite and > 0;
 * period > 0 finite, max_ticks >= 2, window 0 (choose per path) or 1 .. max_window, max_window 1 .. 256, 0 < aim <= 1.
 *
 *   status        EMPTY, NONFINITE, UNORDERED, POINT: the setpoints rule's tests and values.  A POINT path has one tick (q = r_0, qd = +0.0,
 *                 tau = +0.0) and window 0.
 *   input         a path with D = t_{R-1} > 0 has n = (int64)ceil(D / period), the setpoints rule's N - 1.  For any integer i: x_i = (r_0, +0.0)
 *                 for i <= 0, x_i = (r_{R-1}, +0.0) for i >= n, else x_i = (q, qd) of the setpoints rule's interior tick at setpoint_tau(i,
 *                 period, D): the same bracket, the same u, setpoint_q and setpoint_qd.  The arrival sits ON the grid at n period, not at D: a
 *                 window over a sequence needs a uniform grid.
 *   output for W  M = n + W ticks, tau_j = fl((double)j period).  Ticks 0 and M - 1 are copies of r_0 and r_{R-1} with qd = +0.0 (every term of
 *                 their windows is that held value).  Else q_j[c] = (x_{j-W+1}[c] + ... + x_j[c]) / (double)W: summed from the oldest term to the
 *                 newest, one rounding per addition, then ONE division; qd_j[c] the same over the qd parts.  (A running sum carried from
 *                 tick to tick is another rounding sequence and is not this rule.)  M > max_ticks, or a count beyond INT32_MAX: FULL, no tick.
 *   audit         every peak under the setpoints rule's order (value, tick): ties go to the smallest tick, a NaN share keeps its tick from
 *                 contributing, a peak without contributor is +0.0 at tick -1 (clearance: +inf).  speed = max setpoint_speed(qd_j[c], vmax_c);
 *                 acceleration = max setpoint_acc(qd_j[c], qd_{j+1}[c], tau_{j+1} - tau_j, amax_c) at the left tick j; jerk: with the signed
 *                 a_j[c] = (qd_{j+1}[c] - qd_j[c]) / (tau_{j+1} - tau_j), jerk_j[c] = (|a_{j+1}[c] - a_j[c]| / (0.5 (tau_{j+2} - tau_j))) / jmax_c for
 *                 0 <= j <= M - 3, at the MIDDLE tick j + 1 (a path with M < 3 has no contributor); max |dp|, max angle, min clearance, n_off
 *                 and n_below as in the setpoints unit, on the FILTERED q.
 *   the window    window > 0: one measurement of the jerk peak P for W = window; OK when P <= 1, else WINDOW; passes = 0.  window == 0, per
 *                 path: W = 1, passes = 0; measure P for W; P <= 1: OK; else W == max_window: WINDOW (the ticks and the audit of max_window
 *                 are still delivered); else W <- min(max_window, max(W + 1, (int)ceil(W P / aim))), passes += 1, measure again.  A W whose
 *                 M no longer fits is FULL and ends the path: window and passes then name the W that did not fit.
 *
 * What holds by construction.  A mean of values cannot exceed their largest: the filtered speed and acceleration peaks do not rise above the
 * unfiltered ones (W = 1) and q_j[c] stays within the hull of its window's inputs, both up to the rounding of W - 1 additions and a
 * division.  qd_{j+1} - qd_j = (v_{j+1} - v_{j+1-W}) / W telescopes, so a_{j+1} - a_j is a difference of two unfiltered accelerations over W period:
 * the jerk of joint c is at most 2 A_c / (W period), A_c the joint's unfiltered acceleration peak in rad/s^2.  Hence every W >= W* = ceil(max_c
 * 2 A_c / (period jmax_c)) passes; W strictly increases, so the search ends within max_window passes, and it ends in OK whenever W* <=
 * max_window.  (A Panda has amax_c / jmax_c = 0.002 s on every joint: a path whose acceleration ratio is <= 1 passes with W = 4 at 1 ms.)
 * The motion grows by W - 1 ticks and still starts and ends at rest on r_0 and r_{R-1}.
 *
 * What it is NOT.  It is a bound at the ticks of the stated period, on the qd sequence, as the setpoints audit is; it is not a third
 * difference of positions (a two-row path with D <= period has n = 1 and every qd zero, whatever its rows).  The filtered ticks no longer
 * pass through the rows: they lag by (W - 1) / 2 ticks and cut corners by the order of a (W period)^2 / 24 — the gap, isSatisfied and
 * clearance figures of the same call are what tell whether that matters.  It is not a jerk-optimal profile. */
#ifndef CCMP_JERK_H
#define CCMP_JERK_H
#include "ccmp_setpoints.h"

namespace ccmp {

enum : int { kJerkOpen = -1, kJerkOk = CCMP_JERK_OK, kJerkFull = CCMP_JERK_FULL, kJerkWindow = CCMP_JERK_WINDOW };
enum : int { kJerkPeakSpeed = 0, kJerkPeakAcc = 1, kJerkPeakJerk = 2, kJerkPeakDp = 3, kJerkPeakAngle = 4, kJerkPeakClearance = 5, kJerkPeaks = 6 };
enum : int { kJerkMaxWindow = 256 };

/* The limits of a call, checked on the host and handed to the kernels by value */
struct jerk_limits {
  double vmax[14], amax[14], jmax[14];
};

/* tau_j of an output tick */
CCMP_HD double jerk_tau(int64_t j, double period) { return (double)j * period; }

/* M of a path with n tick intervals under the window W; 0: FULL */
CCMP_HD int32_t jerk_ticks(int64_t n, int W, int max_ticks)
{
  const int64_t M = n + (int64_t)W;
  return M > (int64_t)max_ticks ? 0 : (int32_t)M;
}

/* the mean of a window whose terms have been summed, oldest to newest, into `sum` */
CCMP_HD double jerk_mean(double sum, int W) { return sum / (double)W; }

/* a_j[c], signed; width = tau_{j+1} - tau_j */
CCMP_HD double jerk_acc(double qd_a, double qd_b, double width)
{
  const double dv = qd_b - qd_a;
  return dv / width;
}

/* one joint's share of the jerk ratio at the middle tick j + 1: a0 = a_j[c], a1 = a_{j+1}[c], span = tau_{j+2} - tau_j */
CCMP_HD double jerk_ratio(double a0, double a1, double span, double jmax)
{
  const double da = ccmp_abs(a1 - a0);
  const double half = 0.5 * span;
  const double jerk = da / half;
  return jerk / jmax;
}

/* the share of joint c at the middle tick of three filtered velocities va, vb, vc at ticks j, j + 1, j + 2 */
CCMP_HD double jerk_share(double va, double vb, double vc, int64_t j, double period, double jmax)
{
  const double t0 = jerk_tau(j, period), t1 = jerk_tau(j + 1, period), t2 = jerk_tau(j + 2, period);
  const double a0 = jerk_acc(va, vb, t1 - t0), a1 = jerk_acc(vb, vc, t2 - t1);
  return jerk_ratio(a0, a1, t2 - t0, jmax);
}

/* the window that follows W when the jerk peak P > 1 was measured for it; W < max_window */
CCMP_HD int jerk_next_window(int W, double P, double aim, int max_window)
{
  const double x = (double)W * P;
  const double y = x / aim;
  const double c = __builtin_ceil(y);
  int next = c < (double)max_window ? (int)c : max_window; /* (P is no NaN: a NaN never contributes to a peak) */
  if (next < W + 1) next = W + 1;
  return next < max_window ? next : max_window;
}

}  // namespace ccmp

#endif /* CCMP_JERK_H */
