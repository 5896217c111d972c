/* ccmp_fit.h — time stamps fitted to the limits at the controller's rate: the step between ccmp_path_timestamps and ccmp_path_setpoints.  The
 * time-stamp rule bounds its profile at the rows; the setpoints' audit measures what a controller is commanded between them.  This rule closes
 * that loop: it measures the commanded motion at the ticks of the stated period, dilates ONLY the row intervals in which it exceeds a limit,
 * measures again on the new stamps and repeats until the audit passes.  One rule text for host and device: the kernels of
 * ccmp_kernels_fit.hip and ccmp_path_fit_timestamps_ref (ccmp_fit.cpp) both compile it with -ffp-contract=off, and it holds NO fused operation:
 * one rounding per written operation, IEEE division, ccmp_sqrt — plain Python floats restate it.  Status, tick count, tau, tangents, qd, the
 * speed and acceleration shares and the bracket are ccmp_setpoints.h's and ccmp_dense.h's, unchanged.
 *
 * Inputs: packed rows [total_rows][14] with path_first [F + 1], stamps time [total_rows]; vmax[14], amax[14] finite and > 0; period > 0 finite,
 * max_ticks >= 2, 0 < aim <= 1, max_passes >= 0.  Per path, with stamps t (the input stamps at pass 0) and passes = 0:
 *
 *   1 status      the setpoints rule's on (rows, t): status and N.  EMPTY, NONFINITE, UNORDERED, POINT and FULL end the path with that status
 *                 and the stamps it was found on (at pass 0: the input's); peak = the last measurement made, +0.0 without one.
 *   2 ticks       tau_j and the tangents w of the setpoints rule; for 1 <= j <= N-1 k_j = arc_bracket(t, tau_j), and k_0 = k_1.  qd_0 =
 *                 qd_{N-1} = +0.0, an interior qd_j[c] = setpoint_qd on the bracket k_j.
 *   3 per tick    s_j = max_c setpoint_speed(qd_j[c], vmax_c); for j < N-1 with tau_{j+1} - tau_j > 0: a_j = max_c setpoint_acc(qd_j[c],
 *                 qd_{j+1}[c], tau_{j+1} - tau_j, amax_c).  A figure with a NaN share never contributes, as in the audit.
 *   4 per row interval k = 1 .. R-1: S_k = max{ s_j : k_j = k }, A_k = max{ a_j : k_j <= k <= k_{j+1} } (a tick interval that spans several
 *                 row intervals — rows closer than the period — hands its acceleration to every one of them); an empty set gives +0.0.
 *                 Every value is non-negative, so every maximum is order-free (and the maximum of the bit patterns).
 *   5 done        P_s = max_k S_k, P_a = max_k A_k.  P_s <= 1 and P_a <= 1: FITTED, stamps untouched.  Else passes == max_passes: PASSES,
 *                 stamps as measured.
 *   6 dilation    f_k = max(1, S_k / aim, ccmp_sqrt(A_k / aim)); h'_k = fl((t_k - t_{k-1}) f_k); t'_0 = +0.0, t'_k = fl(t'_{k-1} + h'_k), left to
 *                 right; passes += 1; back to 1.
 *
 * Outputs: time_out, status (the setpoints values with 0 = FITTED, and PASSES = 6), passes, peak (P_s, P_a of the last measurement), duration
 * (the last stamp of time_out; +0.0 EMPTY, NaN NONFINITE), factor (time_out's interval over the input's at the interval's right row; row 0 and
 * intervals of no positive input width: 1.0).
 *
 * By construction f_k >= 1: stamps stay ordered, an interval of no width keeps none, and no interval or duration shrinks by more than the
 * rounding of the stamps' sum (factor is a quotient of differences of summed stamps and can read one spacing of a stamp below 1); a path that
 * is done is never touched again whatever its batch neighbours do; the result is a function of the inputs alone.  What it is NOT: it is not TOPP-RA (no
 * optimality is claimed, only the audit's own figures at the ticks of the stated period), it has no jerk limit, and its convergence is
 * observed, not proven — which is why aim < 1 is the default (with aim = 1 the peaks creep towards 1 from above) and why PASSES is a status. */
#ifndef CCMP_FIT_H
#define CCMP_FIT_H
#include "ccmp_setpoints.h"

namespace ccmp {

enum : int { kFitOpen = -1, kFitFitted = CCMP_FIT_FITTED, kFitPasses = CCMP_FIT_PASSES };

/* (the tick of step 2, its tau and its bracket, is setpoint_bracket of ccmp_setpoints.h: the last tick's bracket is what this rule asks of it) */

/* step 5 */
CCMP_HD bool fit_done(double Ps, double Pa) { return Ps <= 1.0 && Pa <= 1.0; }

/* f_k */
CCMP_HD double fit_factor(double S, double A, double aim)
{
  const double s = S / aim;
  const double qa = A / aim;
  const double r = ccmp_sqrt(qa);
  double f = 1.0;
  if (s > f) f = s;
  if (r > f) f = r;
  return f;
}

/* h'_k */
CCMP_HD double fit_width(double ta, double tb, double f)
{
  const double h = tb - ta;
  return h * f;
}

/* factor of an interval: the output's width over the input's */
CCMP_HD double fit_ratio(double in_a, double in_b, double out_a, double out_b)
{
  const double hin = in_b - in_a;
  if (!(hin > 0.0)) return 1.0;
  const double hout = out_b - out_a;
  return hout / hin;
}

/* the duration a status that ends a path without a measurement leaves: `last` = the path's last stamp (not read for EMPTY and NONFINITE) */
CCMP_HD double fit_closed_duration(int status, double last)
{
  if (status == kSetpointsEmpty) return 0.0;
  if (status == kSetpointsNonFinite) return __builtin_nan("");
  return last;
}

}  // namespace ccmp

#endif /* CCMP_FIT_H */
