/* ccmp_lanes.h — what the kernels of the three timed-path units share on the device (ccmp_kernels_setpoints.hip, ccmp_kernels_fit.hip,
 * ccmp_kernels_jerk.hip): the bit patterns of non-negative doubles, the DPP row folds of sixteen lanes, and the audit fold of the two peak
 * kernels.  Device only; the rule texts stay in ccmp_setpoints.h, ccmp_fit.h and ccmp_jerk.h. */
#ifndef CCMP_LANES_H
#define CCMP_LANES_H
#include <hip/hip_runtime.h>

#include "ccmp_setpoints.h"

namespace ccmp_lanes {

typedef unsigned long long u64;

// non-negative doubles order as their bit patterns: what the 64-bit unsigned atomic maxima of the fit and jerk units rest on
__device__ __forceinline__ u64 bits_of(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ double value_of(u64 b) { return __longlong_as_double((long long)b); }

// a DPP row operation on one 32-bit half
template <int kCtrl> __device__ __forceinline__ int dpp32(int v) { return __builtin_amdgcn_update_dpp(v, v, kCtrl, 0xf, 0xf, false); }
template <int kCtrl> __device__ __forceinline__ double dpp64(double v)
{
  return __hiloint2double(dpp32<kCtrl>(__double2hiint(v)), dpp32<kCtrl>(__double2loint(v)));
}
// The maximum over the sixteen lanes of a DPP row of non-negative doubles without a NaN, in every lane of the row: rotations by 8, 4, 2, 1
// (row_ror:n is 0x120 + n).  The whole row is active wherever this is called.
__device__ __forceinline__ double row_max(double v)
{
  double o;
  o = dpp64<0x128>(v); v = o > v ? o : v;
  o = dpp64<0x124>(v); v = o > v ? o : v;
  o = dpp64<0x122>(v); v = o > v ? o : v;
  o = dpp64<0x121>(v); v = o > v ? o : v;
  return v;
}
__device__ __forceinline__ int row_or(int v)
{
  v |= dpp32<0x128>(v);
  v |= dpp32<0x124>(v);
  v |= dpp32<0x122>(v);
  v |= dpp32<0x121>(v);
  return v;
}

// one lane's or one block's peaks: kCols (value, tick) pairs
template <int kCols> struct Peaks {
  double v[kCols];
  int32_t j[kCols];
};

template <class A> __device__ __forceinline__ void offer(Peaks<A::kCols> &p, int which, double v, int32_t j)
{
  const bool better = which == A::kClearance ? ccmp::setpoint_lower(v, j, p.v[which], p.j[which]) : ccmp::setpoint_higher(v, j, p.v[which], p.j[which]);
  if (better) { p.v[which] = v; p.j[which] = j; }
}

// The audit of one path by one block of kThreads lanes: every lane folds its ticks into the (value, tick) peaks and the two counts, the block
// folds the lanes in LDS under the same total order (setpoint_higher; the clearance: setpoint_lower) — the answer is a function of the inputs
// alone.  What differs between the units is the trait A:
//   kCols                 the columns of peak and peak_tick
//   kSpeed, kAcc, kDp, kAngle, kClearance   where each figure goes; kJerk the jerk column, -1 where the unit has none
//   kStretch              whether stretch [f] is written
//   width(g, j)           tau_{j+1} - tau_j of tick j < last, the tick's index in the batch being g
//   jerk(qd, g, j, c)     (kJerk >= 0) joint c's jerk share at the middle tick j of j - 1, j, j + 1
// vmax and amax are the call's limits; qd, fgap, satisfied and clearance the ticks' arrays; tick_first [F + 1] is never trusted.
template <class A, int kThreads>
__device__ __forceinline__ void audit_fold(const A &a, const double *vmax, const double *amax, const double *__restrict__ qd, const double *__restrict__ fgap,
                                           const uint8_t *__restrict__ satisfied, const double *__restrict__ clearance, const int32_t *__restrict__ tick_first,
                                           long long total_ticks, double margin, double *__restrict__ peak, int32_t *__restrict__ peak_tick,
                                           int32_t *__restrict__ counts, double *__restrict__ stretch)
{
  constexpr int kCols = A::kCols;
  __shared__ double s_v[kCols][kThreads];
  __shared__ int32_t s_j[kCols][kThreads];
  __shared__ int32_t s_n[2][kThreads];
  const int f = blockIdx.x, t = threadIdx.x;
  long long first = tick_first[f], N = (long long)tick_first[f + 1] - first;
  if (first < 0 || N < 0 || first + N > total_ticks) N = 0; // block-uniform: never trusted, a path without ticks
  Peaks<kCols> p;
#pragma unroll
  for (int w = 0; w < kCols; w++) { p.v[w] = w == A::kClearance ? __builtin_inf() : 0.0; p.j[w] = -1; }
  int32_t n_off = 0, n_below = 0;
  for (long long j = t; j < N; j += kThreads) {
    const size_t g = (size_t)(first + j);
    const bool has_next = j + 1 < N, has_prev = j > 0;
    const double width = has_next ? a.width(g, j) : 0.0;
    double speed = 0.0, acc = 0.0, jerk = 0.0; // (the maxima over the joints: finite values, any order)
    bool speed_nan = false, acc_nan = false, jerk_nan = false;
    for (int c = 0; c < 14; c++) {
      const double v = qd[g * 14 + c];
      const double s = ccmp::setpoint_speed(v, vmax[c]);
      speed_nan = speed_nan || s != s;
      if (s > speed) speed = s;
      if (width > 0.0) {
        const double x = ccmp::setpoint_acc(v, qd[(g + 1) * 14 + c], width, amax[c]);
        acc_nan = acc_nan || x != x;
        if (x > acc) acc = x;
      }
      if constexpr (A::kJerk >= 0) {
        if (has_next && has_prev) { // this tick is the middle one of j - 1, j, j + 1
          const double k = a.jerk(qd, g, j, c);
          jerk_nan = jerk_nan || k != k;
          if (k > jerk) jerk = k;
        }
      }
    }
    if (!speed_nan) offer<A>(p, A::kSpeed, speed, (int32_t)j);
    if (width > 0.0 && !acc_nan) offer<A>(p, A::kAcc, acc, (int32_t)j);
    if constexpr (A::kJerk >= 0)
      if (has_next && has_prev && !jerk_nan) offer<A>(p, A::kJerk, jerk, (int32_t)j);
    offer<A>(p, A::kDp, fgap[g * 2], (int32_t)j);
    offer<A>(p, A::kAngle, fgap[g * 2 + 1], (int32_t)j);
    const double cl = clearance[g];
    offer<A>(p, A::kClearance, cl, (int32_t)j);
    n_off += satisfied[g] ? 0 : 1;
    n_below += cl < margin ? 1 : 0;
  }
#pragma unroll
  for (int w = 0; w < kCols; w++) { s_v[w][t] = p.v[w]; s_j[w][t] = p.j[w]; }
  s_n[0][t] = n_off;
  s_n[1][t] = n_below;
  __syncthreads();
  for (int m = kThreads / 2; m > 0; m >>= 1) { // block-uniform: every lane meets every barrier
    if (t < m) {
#pragma unroll
      for (int w = 0; w < kCols; w++) {
        const double v = s_v[w][t + m], bv = s_v[w][t];
        const int32_t j = s_j[w][t + m], bj = s_j[w][t];
        const bool better = j >= 0 && (w == A::kClearance ? ccmp::setpoint_lower(v, j, bv, bj) : ccmp::setpoint_higher(v, j, bv, bj));
        if (better) { s_v[w][t] = v; s_j[w][t] = j; }
      }
      s_n[0][t] += s_n[0][t + m];
      s_n[1][t] += s_n[1][t + m];
    }
    __syncthreads();
  }
  if (t < kCols) {
    peak[(size_t)f * kCols + t] = s_v[t][0];
    peak_tick[(size_t)f * kCols + t] = s_j[t][0];
  } else if (t < kCols + 2) {
    counts[(size_t)f * 2 + (t - kCols)] = s_n[t - kCols][0];
  } else if (A::kStretch && t == kCols + 2) {
    stretch[f] = ccmp::setpoint_stretch(s_v[A::kSpeed][0], s_v[A::kAcc][0]);
  }
}

}  // namespace ccmp_lanes

#endif /* CCMP_LANES_H */
