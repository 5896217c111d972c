// ccmp_kernels_fit.hip — time stamps fitted to the limits at the controller's rate on the device (ccmp_path_fit_timestamps; the rule is
// csrc/ccmp_fit.h, compiled here and in ccmp_fit.cpp: one text, the same bits).  The status scan and the tangents of a pass are the setpoints
// unit's launchers, unchanged; this unit measures and dilates.  The ticks are never materialised: rows, stamps and tangents are the only
// memory traffic, and the per-row-interval maxima S and A are all a pass leaves.
//   fit_begin_kernel     one 256-lane block per path: the path's range checked (a range that is negative, decreasing or beyond the rows is
//                        never read and never written), the input stamps copied to time_out, the path's result words reset to "open".
//   fit_measure_kernel   the hot path.  Sixteen lanes per tick interval j, lanes 0 .. 13 one joint each.  The interval's path by bisection on
//                        tick_first; the brackets of tau_j and tau_{j+1} (setpoint_bracket) and qd at both (setpoint_joint: the setpoints
//                        rule's tick, as in its sample kernel); s_j and a_j folded across the sixteen lanes with the DPP row folds of
//                        ccmp_lanes.h; neighbouring groups of a wavefront with the same brackets merged; then a
//                        64-bit unsigned atomic maximum on the bit pattern (non-negative doubles order as their bits) into S[k_j] and
//                        A[k_j .. k_{j+1}], the sixteen lanes striding that range.
//   fit_dilate_kernel    one wavefront per path: P_s and P_a folded, FITTED / PASSES / open decided; an open path's h' 64 at a time, lane 0's
//                        left-to-right sum, the stamps written in place, S and A cleared for the next pass.
//   fit_factor_kernel    per row: time_out's interval over the input's.
// No grid barrier, no spin; every loop is bounded by its data; lanes beyond the data are masked; every offset read from memory is
// range-checked before use.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_fit.h"
#include "ccmp_lanes.h"
#include "ccmp_launch.h"

namespace {

using ccmp::blocks_of;
using ccmp::path_of;
using ccmp::setpoint_limits;
constexpr int kThreads = 256;
constexpr int kWave = 64;
using ccmp_lanes::bits_of;
using ccmp_lanes::row_max;
using ccmp_lanes::row_or;
using ccmp_lanes::u64;
using ccmp_lanes::value_of;

__global__ __launch_bounds__(kThreads) void fit_begin_kernel(const int32_t *__restrict__ path_first, const double *__restrict__ time, long long total_rows,
                                                            double *__restrict__ time_out, int32_t *__restrict__ status, int32_t *__restrict__ passes,
                                                            double *__restrict__ peak, double *__restrict__ duration)
{
  const int f = blockIdx.x, t = threadIdx.x;
  const long long first = path_first[f], end = path_first[f + 1];
  if (first >= 0 && end > first && end <= total_rows) // block-uniform
    for (long long r = first + t; r < end; r += kThreads) time_out[r] = time[r];
  if (t == 0) {
    status[f] = ccmp::kFitOpen;
    passes[f] = 0;
    peak[(size_t)f * 2] = 0.0;
    peak[(size_t)f * 2 + 1] = 0.0;
    duration[f] = 0.0;
  }
}

__global__ __launch_bounds__(kThreads) void fit_measure_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                              const double *__restrict__ time, const double *__restrict__ tangent,
                                                              const int32_t *__restrict__ tick_first, unsigned int F, long long M, long long total_rows,
                                                              double period, setpoint_limits lim, u64 *__restrict__ S, u64 *__restrict__ A)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long g = (long long)(t >> 4);
  const int c = (int)(t & 15), lane = (int)(threadIdx.x & (kWave - 1));
  double s = 0.0, a = 0.0;  // the group's s_j and a_j (+0.0: nothing to fold)
  long long lo = -1, hi = -1; // the rows of S and A the group folds into: first + k_j .. first + k_{j+1}; -1: none
  if (g < M) {                // (whole groups of sixteen take the same way through here: a DPP row is all active or all idle)
    const unsigned int f = path_of(tick_first, F, g);
    const long long j = g - tick_first[f], n = (long long)tick_first[f + 1] - tick_first[f]; // n = N - 1 tick intervals
    const long long first = path_first[f], R = (long long)path_first[f + 1] - first;
    if (j >= 0 && j < n && first >= 0 && R >= 2 && first + R <= total_rows) { // never trusted
      const double *tp = time + first;
      const double D = tp[R - 1];
      int k0, k1;
      double tau0, tau1, u0, u1;
      // (false: the rule's own precondition of a bracket; an OK path meets it)
      if (ccmp::setpoint_bracket(tp, (int)R, j + 1, n + 1, period, D, &tau1, &k1, &u1) && ccmp::setpoint_bracket(tp, (int)R, j, n + 1, period, D, &tau0, &k0, &u0)) {
        if (j == 0) k0 = k1;
        if (k0 >= 1 && k0 <= k1 && k1 < R) {
          const double width = tau1 - tau0;
          int nan = 0;
          if (c < 14) {
            const double *r = rows + (size_t)first * 14 + c, *w = tangent + (size_t)first * 14 + c;
            double v0 = 0.0, v1 = 0.0, x; // (x: the position half, never used)
            if (j > 0) ccmp::setpoint_joint(r, w, tp, k0, u0, &x, &v0);
            if (j + 1 < n) ccmp::setpoint_joint(r, w, tp, k1, u1, &x, &v1);
            s = ccmp::setpoint_speed(v0, lim.vmax[c]);
            if (s != s) { nan |= 1; s = 0.0; }
            if (width > 0.0) {
              a = ccmp::setpoint_acc(v0, v1, width, lim.amax[c]);
              if (a != a) { nan |= 2; a = 0.0; }
            }
          }
          s = row_max(s);
          a = row_max(a);
          nan = row_or(nan);
          if (nan & 1) s = 0.0; // a NaN share: the figure does not contribute
          if (nan & 2) a = 0.0;
          lo = first + k0;
          hi = first + k1;
        }
      }
    }
  }
  // Neighbouring groups of the wavefront with the same brackets: the first of such a run folds for all of them.  Every lane of the wavefront
  // takes part in the exchanges (blocks are whole wavefronts); a group without work has lo = -1 and heads nothing.
  double sm = s, am = a;
  bool run = true;
#pragma unroll
  for (int r = 1; r < kWave / 16; r++) {
    const int src = lane + 16 * r;
    const long long olo = __shfl(lo, src & (kWave - 1)), ohi = __shfl(hi, src & (kWave - 1));
    const double os = __shfl(s, src & (kWave - 1)), oa = __shfl(a, src & (kWave - 1));
    run = run && src < kWave && olo == lo && ohi == hi;
    if (run) {
      sm = os > sm ? os : sm;
      am = oa > am ? oa : am;
    }
  }
  const long long plo = __shfl(lo, (lane + kWave - 16) & (kWave - 1)), phi = __shfl(hi, (lane + kWave - 16) & (kWave - 1));
  const bool head = lo >= 1 && hi < total_rows && (lane < 16 || plo != lo || phi != hi);
  if (head) {
    if (c == 0 && sm > 0.0) atomicMax(S + lo, bits_of(sm)); // (+0.0 is what the arrays hold already)
    if (am > 0.0)
      for (long long k = lo + c; k <= hi; k += 16) atomicMax(A + k, bits_of(am));
  }
}

__global__ __launch_bounds__(kWave) void fit_dilate_kernel(const int32_t *__restrict__ path_first, const int32_t *__restrict__ sp_status, double aim,
                                                          int max_passes, double *__restrict__ time, u64 *__restrict__ S, u64 *__restrict__ A,
                                                          int32_t *__restrict__ status, int32_t *__restrict__ passes, double *__restrict__ peak,
                                                          double *__restrict__ duration)
{
  __shared__ double s_h[kWave], s_t[kWave];
  const int f = blockIdx.x, lane = threadIdx.x;
  if (status[f] != ccmp::kFitOpen) return; // block-uniform: a path that is done is never touched again
  const int st = sp_status[f];
  if (st != ccmp::kSetpointsOk) { // block-uniform: the setpoints status ends the path (its range has been checked unless it is EMPTY)
    if (lane == 0) {
      const bool read = st != ccmp::kSetpointsEmpty && st != ccmp::kSetpointsNonFinite;
      duration[f] = ccmp::fit_closed_duration(st, read ? time[(long long)path_first[f + 1] - 1] : 0.0);
      status[f] = st;
    }
    return;
  }
  const long long first = path_first[f], R = (long long)path_first[f + 1] - first; // checked by the status kernel; R >= 2
  u64 ps = 0, pa = 0;
  for (long long k = 1 + lane; k < R; k += kWave) {
    const u64 sv = S[first + k], av = A[first + k];
    ps = sv > ps ? sv : ps;
    pa = av > pa ? av : pa;
  }
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const u64 os = __shfl_xor(ps, m), oa = __shfl_xor(pa, m);
    ps = os > ps ? os : ps;
    pa = oa > pa ? oa : pa;
  }
  const double Ps = value_of(ps), Pa = value_of(pa);
  const int n = passes[f];
  const bool done = ccmp::fit_done(Ps, Pa);
  if (lane == 0) {
    peak[(size_t)f * 2] = Ps;
    peak[(size_t)f * 2 + 1] = Pa;
  }
  if (done || n >= max_passes) { // block-uniform
    if (lane == 0) {
      status[f] = done ? ccmp::kFitFitted : ccmp::kFitPasses;
      duration[f] = time[first + R - 1];
    }
    return;
  }
  double acc = 0.0;          // lane 0's running time
  double carry = time[first]; // the OLD stamp left of the chunk: the chunk before has overwritten it in memory
  for (long long base = 0; base < R - 1; base += kWave) { // block-uniform: every lane meets every barrier and every exchange
    const long long left = R - 1 - base;
    const int m = left < kWave ? (int)left : kWave;
    const long long k = base + lane + 1;
    const double tk = lane < m ? time[first + k] : 0.0;
    const double up = __shfl_up(tk, 1);
    const double tprev = lane == 0 ? carry : up;
    carry = __shfl(tk, m - 1);
    if (lane < m) {
      s_h[lane] = ccmp::fit_width(tprev, tk, ccmp::fit_factor(value_of(S[first + k]), value_of(A[first + k]), aim));
      S[first + k] = 0;
      A[first + k] = 0;
    }
    __syncthreads();
    if (lane == 0)
      for (int q = 0; q < m; q++) {
        acc = acc + s_h[q];
        s_t[q] = acc;
      }
    __syncthreads();
    if (lane < m) time[first + k] = s_t[lane];
  }
  if (lane == 0) {
    time[first] = 0.0; // t'_0 = +0.0
    passes[f] = n + 1;
    duration[f] = acc;
  }
}

__global__ __launch_bounds__(kThreads) void fit_factor_kernel(const int32_t *__restrict__ path_first, unsigned int F, long long total_rows,
                                                             const double *__restrict__ time, const double *__restrict__ time_out,
                                                             double *__restrict__ factor)
{
  const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= total_rows) return;
  const unsigned int f = path_of(path_first, F, r);
  const long long first = path_first[f], end = path_first[f + 1];
  if (first < 0 || end > total_rows || r < first || r >= end) return; // a range that is never read is never written
  factor[r] = r == first ? 1.0 : ccmp::fit_ratio(time[r - 1], time[r], time_out[r - 1], time_out[r]);
}

}  // namespace

namespace ccmp_launch {

hipError_t fit_begin(const int32_t *path_first, const double *time, size_t F, size_t total_rows, double *time_out, int32_t *status, int32_t *passes,
                     double *peak, double *duration, hipStream_t st)
{
  hipLaunchKernelGGL(fit_begin_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, path_first, time, (long long)total_rows, time_out, status, passes, peak,
                     duration);
  return hipGetLastError();
}

hipError_t fit_measure(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *tick_first, size_t F,
                       size_t M, size_t total_rows, double period, const ccmp::setpoint_limits &lim, unsigned long long *S, unsigned long long *A,
                       hipStream_t st)
{
  hipLaunchKernelGGL(fit_measure_kernel, dim3(blocks_of(M * 16, kThreads)), dim3(kThreads), 0, st, rows, path_first, time, tangent, tick_first, (unsigned int)F,
                     (long long)M, (long long)total_rows, period, lim, S, A);
  return hipGetLastError();
}

hipError_t fit_dilate(const int32_t *path_first, const int32_t *sp_status, size_t F, double aim, int max_passes, double *time, unsigned long long *S,
                      unsigned long long *A, int32_t *status, int32_t *passes, double *peak, double *duration, hipStream_t st)
{
  hipLaunchKernelGGL(fit_dilate_kernel, dim3((unsigned int)F), dim3(kWave), 0, st, path_first, sp_status, aim, max_passes, time, S, A, status, passes, peak,
                     duration);
  return hipGetLastError();
}

hipError_t fit_factor(const int32_t *path_first, size_t F, size_t total_rows, const double *time, const double *time_out, double *factor, hipStream_t st)
{
  hipLaunchKernelGGL(fit_factor_kernel, dim3(blocks_of(total_rows, kThreads)), dim3(kThreads), 0, st, path_first, (unsigned int)F, (long long)total_rows, time,
                     time_out, factor);
  return hipGetLastError();
}

}  // namespace ccmp_launch
