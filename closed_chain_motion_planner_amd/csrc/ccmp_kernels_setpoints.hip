// ccmp_kernels_setpoints.hip — controller-rate setpoints and the execution audit of timed paths on the device (ccmp_path_setpoints; the rule
// is csrc/ccmp_setpoints.h, compiled here and in ccmp_setpoints.cpp: one text, the same bits).  The constraint gap, isSatisfied and the
// clearance of the ticks are the function, is-satisfied and clearance launchers, unchanged, run once each over all ticks of all paths; this
// unit scans, interpolates and audits:
//   setpoints_status_kernel   one 256-lane block per path: the path's range checked against the row count (a range that is negative,
//                             decreasing or beyond the rows is never trusted: the path counts as EMPTY), every coordinate and stamp tested
//                             for finiteness, every interval for its order; writes status[f] and the path's tick count.
//   setpoints_tangent_kernel  sixteen lanes per row, lanes 0 .. 13 one joint each: the two slopes and the row's tangent.
//   setpoints_sample_kernel   sixteen lanes per tick.  The tick's path by bisection on tick_first; the tick by the rule's setpoint_bracket
//                             and setpoint_joint (the fit and jerk units' too); lanes 0 .. 13 q and qd of one joint each, lane 14 writes
//                             tau, lane 15 the NaN a clearance holds until a scene has answered.
//   setpoints_peak_kernel     one 256-lane block per path: audit_fold of ccmp_lanes.h (the jerk unit's too) with five columns, the widths
//                             from tau, and stretch.
// No grid barrier, no spin; every loop is bounded by its data; lanes beyond the data are masked; every offset read from memory is
// range-checked before use.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_lanes.h"
#include "ccmp_launch.h"
#include "ccmp_setpoints.h"

namespace {

using ccmp::blocks_of;
using ccmp::path_of;
using ccmp::setpoint_limits;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void setpoints_status_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                                   const double *__restrict__ time, long long total_rows, double period,
                                                                   int max_ticks, int32_t *__restrict__ status, int32_t *__restrict__ ticks)
{
  const int f = blockIdx.x, t = threadIdx.x;
  const long long first = path_first[f], end = path_first[f + 1];
  const bool range = first >= 0 && end > first && end <= total_rows; // block-uniform
  int bad = 0, order = 0;
  if (range) {
    for (long long w = first * 14 + t; w < end * 14; w += kThreads)
      if (!ccmp::setpoint_finite(rows[w])) bad = 1;
    for (long long r = first + t; r < end; r += kThreads)
      if (!ccmp::setpoint_finite(time[r])) bad = 1;
  }
  bad = __syncthreads_or(bad);
  if (range && !bad) { // block-uniform; every value is finite from here on
    if (t == 0 && time[first] != 0.0) order = 1;
    for (long long r = first + t; r + 1 < end; r += kThreads) {
      const double ta = time[r], tb = time[r + 1];
      bool moved = false;
      if (tb == ta)
        for (int c = 0; c < 14; c++) moved = moved || rows[(size_t)r * 14 + c] != rows[(size_t)(r + 1) * 14 + c];
      if (ccmp::setpoint_unordered(ta, tb, moved)) order = 1;
    }
  }
  order = __syncthreads_or(order);
  if (t == 0) {
    int32_t n = 0;
    status[f] = range ? ccmp::setpoint_status(bad != 0, order != 0, end - first, bad ? 0.0 : time[end - 1], period, max_ticks, &n) : ccmp::kSetpointsEmpty;
    ticks[f] = n;
  }
}

__global__ __launch_bounds__(kThreads) void setpoints_tangent_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                                    const double *__restrict__ time, unsigned int F, long long total_rows,
                                                                    const int32_t *__restrict__ status, double *__restrict__ tangent)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long r = (long long)(t >> 4);
  const int c = (int)(t & 15);
  if (r >= total_rows || c >= 14) return;
  const unsigned int f = path_of(path_first, F, r);
  if (status[f] != ccmp::kSetpointsOk) return; // an OK path's range has been checked
  const long long first = path_first[f], end = path_first[f + 1];
  if (r < first || r >= end) return;
  double w = 0.0;
  if (r > first && r + 1 < end) {
    const double tp = time[r - 1], tc = time[r], tn = time[r + 1];
    const double hp = tc - tp, h = tn - tc;
    const double qp = rows[(size_t)(r - 1) * 14 + c], q = rows[(size_t)r * 14 + c], qn = rows[(size_t)(r + 1) * 14 + c];
    w = ccmp::setpoint_tangent(hp, h, ccmp::setpoint_slope(qp, q, hp), ccmp::setpoint_slope(q, qn, h));
  }
  tangent[(size_t)r * 14 + c] = w;
}

__global__ __launch_bounds__(kThreads) void setpoints_sample_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                                   const double *__restrict__ time, const double *__restrict__ tangent,
                                                                   const int32_t *__restrict__ status, const int32_t *__restrict__ tick_first,
                                                                   unsigned int F, long long M, long long total_rows, double period,
                                                                   double *__restrict__ q, double *__restrict__ qd, double *__restrict__ tau,
                                                                   double *__restrict__ clearance)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long g = (long long)(t >> 4);
  const int c = (int)(t & 15);
  if (g >= M) return;
  const unsigned int f = path_of(tick_first, F, g);
  const long long j = g - tick_first[f], N = (long long)tick_first[f + 1] - tick_first[f];
  const long long first = path_first[f], R = (long long)path_first[f + 1] - first;
  const int st = status[f];
  if (j < 0 || j >= N || first < 0 || R < 1 || first + R > total_rows || (st != ccmp::kSetpointsOk && st != ccmp::kSetpointsPoint)) return; // never trusted
  long long src = first; // the row a copied tick is
  double at = 0.0, u = 0.0;
  int k = 0; // > 0: an interior tick in the bracket (k - 1, k)
  if (st == ccmp::kSetpointsOk && j > 0) {
    if (!ccmp::setpoint_bracket(time + first, (int)R, j, N, period, time[first + R - 1], &at, &k, &u)) return; // (an OK path meets the precondition)
    if (j == N - 1) { // a copy, whatever its bracket
      src = first + R - 1;
      k = 0;
    }
  }
  if (c < 14) {
    double x = rows[(size_t)src * 14 + c], xd = 0.0;
    if (k > 0) ccmp::setpoint_joint(rows + (size_t)first * 14 + c, tangent + (size_t)first * 14 + c, time + first, k, u, &x, &xd);
    q[g * 14 + c] = x;
    qd[g * 14 + c] = xd;
  } else if (c == 14) {
    tau[g] = at;
  } else {
    clearance[g] = __builtin_nan("");
  }
}

// the audit's trait (ccmp_lanes.h: audit_fold): five columns, the widths from the tau the sample kernel wrote, stretch
struct SetpointsAudit {
  static constexpr int kCols = ccmp::kPeaks, kSpeed = ccmp::kPeakSpeed, kAcc = ccmp::kPeakAcc, kJerk = -1, kDp = ccmp::kPeakDp, kAngle = ccmp::kPeakAngle,
                       kClearance = ccmp::kPeakClearance;
  static constexpr bool kStretch = true;
  const double *tau;
  __device__ double width(size_t g, long long) const { return tau[g + 1] - tau[g]; }
};

__global__ __launch_bounds__(kThreads) void setpoints_peak_kernel(const double *__restrict__ qd, const double *__restrict__ tau, const double *__restrict__ fgap,
                                                                 const uint8_t *__restrict__ satisfied, const double *__restrict__ clearance,
                                                                 const int32_t *__restrict__ tick_first, long long M, setpoint_limits lim, double margin,
                                                                 double *__restrict__ peak, int32_t *__restrict__ peak_tick, int32_t *__restrict__ counts,
                                                                 double *__restrict__ stretch)
{
  ccmp_lanes::audit_fold<SetpointsAudit, kThreads>(SetpointsAudit{tau}, lim.vmax, lim.amax, qd, fgap, satisfied, clearance, tick_first, M, margin, peak, peak_tick,
                                                   counts, stretch);
}

}  // namespace

namespace ccmp_launch {

hipError_t setpoints_status(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, double period, int max_ticks,
                            int32_t *status, int32_t *ticks, hipStream_t st)
{
  hipLaunchKernelGGL(setpoints_status_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, rows, path_first, time, (long long)total_rows, period, max_ticks,
                     status, ticks);
  return hipGetLastError();
}

hipError_t setpoints_tangent(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const int32_t *status,
                             double *tangent, hipStream_t st)
{
  hipLaunchKernelGGL(setpoints_tangent_kernel, dim3(blocks_of(total_rows * 16, kThreads)), dim3(kThreads), 0, st, rows, path_first, time, (unsigned int)F,
                     (long long)total_rows, status, tangent);
  return hipGetLastError();
}

hipError_t setpoints_sample(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *status,
                            const int32_t *tick_first, size_t F, size_t M, size_t total_rows, double period, double *q, double *qd, double *tau,
                            double *clearance, hipStream_t st)
{
  hipLaunchKernelGGL(setpoints_sample_kernel, dim3(blocks_of(M * 16, kThreads)), dim3(kThreads), 0, st, rows, path_first, time, tangent, status, tick_first,
                     (unsigned int)F, (long long)M, (long long)total_rows, period, q, qd, tau, clearance);
  return hipGetLastError();
}

hipError_t setpoints_peak(const double *qd, const double *tau, const double *f, const uint8_t *satisfied, const double *clearance, const int32_t *tick_first,
                          size_t F, size_t M, const ccmp::setpoint_limits &lim, double margin, double *peak, int32_t *peak_tick, int32_t *counts,
                          double *stretch, hipStream_t st)
{
  hipLaunchKernelGGL(setpoints_peak_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, qd, tau, f, satisfied, clearance, tick_first, (long long)M, lim, margin,
                     peak, peak_tick, counts, stretch);
  return hipGetLastError();
}

}  // namespace ccmp_launch
