// ccmp_kernels_retime.hip — resample dense solution paths at even arc and time-stamp packed rows on the device (ccmp_path_resample,
// ccmp_path_timestamps; the rule is csrc/ccmp_retime.h, compiled here and in ccmp_retime.cpp: one text, the same bits).  The projections
// are the projector's kernels and the arcs of the new rows the dense unit's arc kernel, both unchanged; this unit brackets, picks and stamps:
//   retime_status_kernel     one 256-lane block per path: the path's range checked against the row count (a range that is negative,
//                            decreasing or beyond the rows is never trusted: the path counts as EMPTY), then every coordinate of its rows
//                            tested for finiteness; writes status[f] and resets the path's word of the minimum of A.
//   resample_bracket_kernel  sixteen lanes per output row.  The row's path by bisection on the output prefix; the bracket of h_j on the
//                            path's dense arcs; lanes 0 .. 13 blend (a copied or degenerate row: the source row itself), lane 14 writes the
//                            fallback (or source) row, lane 15 the kind so far (pending: the projector decides).
//   resample_pick_kernel     sixteen lanes per output row: projected, fallback, degenerate or copied from the projector's flag into the
//                            packed rows; lane 14 writes the kind, lane 15 counts it (integer atomics: any order, the same totals).
//   retime_ceiling_kernel    sixteen lanes per row, lanes 0 .. 13 one joint each: d_i, d_{i-1}, the three quotients and the acceleration
//                            quotient, a cross-lane minimum into x_i and the row's share of A; lane 0 folds that share into the path's
//                            minimum with an integer atomic minimum on the bit pattern (non-negative doubles order as their bits).
//   retime_envelope_kernel   sixteen lanes per row: y_i as the minimum over every k of the path, k strided over the lanes.
//   retime_stamp_kernel      one wavefront per path: dt 64 at a time, then lane 0's left-to-right sum, then 64 coalesced stores.
// No grid barrier, no spin; every loop is bounded by its data; lanes beyond the data are masked; every offset read from memory is
// range-checked before use.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_launch.h"
#include "ccmp_retime.h"

namespace {

using ccmp::blocks_of;
using ccmp::path_of; // (ccmp_dense.h: the path of a packed row)
using ccmp::retime_limits;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr unsigned long long kNoA = ~0ull; // above the bits of every double >= 0, +inf included: no interval has contributed

// the minimum over the sixteen lanes of a row's group (finite values or +inf: the order cannot change a bit)
__device__ __forceinline__ double min16(double v)
{
  for (int m = 8; m > 0; m >>= 1) v = ccmp::retime_min(v, __shfl_xor(v, m, 16));
  return v;
}

__global__ __launch_bounds__(kThreads) void retime_status_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                                long long total_rows, int32_t *__restrict__ status,
                                                                unsigned long long *__restrict__ a_bits)
{
  const int f = blockIdx.x, t = threadIdx.x;
  const long long first = path_first[f], end = path_first[f + 1];
  int bad = 0;
  const bool range = first >= 0 && end >= first && end <= total_rows; // block-uniform
  if (range)
    for (long long w = first * 14 + t; w < end * 14; w += kThreads)
      if (!ccmp::retime_finite(rows[w])) bad = 1;
  bad = __syncthreads_or(bad);
  if (t == 0) {
    status[f] = (!range || end == first) ? ccmp::kRetimeEmpty : (bad ? ccmp::kRetimeNonFinite : ccmp::kRetimeOk);
    if (a_bits) a_bits[f] = kNoA;
  }
}

__global__ __launch_bounds__(kThreads) void resample_bracket_kernel(const double *__restrict__ rows, const double *__restrict__ arc,
                                                                   const int32_t *__restrict__ path_first, const int32_t *__restrict__ status,
                                                                   const int32_t *__restrict__ out_first, unsigned int F, long long M,
                                                                   long long total_rows, double *__restrict__ x, int32_t *__restrict__ choice,
                                                                   uint8_t *__restrict__ kind)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long g = (long long)(t >> 4);
  const int c = (int)(t & 15);
  if (g >= M) return;
  const unsigned int f = path_of(out_first, F, g);
  const long long j = g - out_first[f], N = (long long)out_first[f + 1] - out_first[f];
  const long long first = path_first[f], R = (long long)path_first[f + 1] - first;
  if (j < 0 || j >= N || first < 0 || R < 1 || first + R > total_rows) return; // never trusted
  long long src = first;
  int what = ccmp::kRetimeCopied, k = 1;
  double tt = 0.0;
  bool lower = true;
  if (status[f] == ccmp::kRetimeOk && j > 0) {
    if (j == N - 1) {
      src = first + R - 1;
    } else {
      const double h = ccmp::retime_target(j, N, arc[first + R - 1]);
      what = ccmp::kRetimeDegenerate;
      if (h > 0.0 && R >= 2 && h <= arc[first + R - 1]) {
        ccmp::arc_bracket(arc + first, (int)R, h, &k, &tt, &lower);
        what = ccmp::kRetimePending;
      }
    }
  }
  if (c < 14) {
    x[g * 14 + c] = what == ccmp::kRetimePending ? ccmp_joint_interpolate(rows[(size_t)(first + k - 1) * 14 + c], rows[(size_t)(first + k) * 14 + c], tt)
                                                 : rows[(size_t)src * 14 + c];
  } else if (c == 14) {
    choice[g] = (int32_t)(what == ccmp::kRetimePending ? first + (lower ? k - 1 : k) : src);
  } else {
    kind[g] = (uint8_t)what;
  }
}

__global__ __launch_bounds__(kThreads) void resample_pick_kernel(const double *__restrict__ rows, const int32_t *__restrict__ out_first, unsigned int F,
                                                                long long M, long long total_rows, const int32_t *__restrict__ choice,
                                                                const uint8_t *__restrict__ kind_so_far, const double *__restrict__ y,
                                                                const uint8_t *__restrict__ ok, double *__restrict__ out_rows,
                                                                uint8_t *__restrict__ kind, int32_t *__restrict__ counts)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long g = (long long)(t >> 4);
  const int c = (int)(t & 15);
  if (g >= M) return;
  const int32_t ch = choice[g];
  int what = kind_so_far[g];
  if (ch < 0 || (long long)ch >= total_rows || (what != ccmp::kRetimePending && what >= ccmp::kRetimeKinds)) return; // never trusted
  if (what == ccmp::kRetimePending) what = ok[g] ? ccmp::kRetimeProjected : ccmp::kRetimeFallback;
  if (c < 14) {
    out_rows[g * 14 + c] = what == ccmp::kRetimeProjected ? y[g * 14 + c] : rows[(size_t)ch * 14 + c];
  } else if (c == 14) {
    kind[g] = (uint8_t)what;
  } else {
    const unsigned int f = path_of(out_first, F, g);
    atomicAdd(counts + (size_t)f * ccmp::kRetimeKinds + what, 1);
  }
}

__global__ __launch_bounds__(kThreads) void retime_ceiling_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first, unsigned int F,
                                                                 long long total_rows, const int32_t *__restrict__ status, retime_limits lim,
                                                                 double *__restrict__ ceiling, unsigned long long *__restrict__ a_bits)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long r = (long long)(t >> 4);
  const int c = (int)(t & 15);
  if (r >= total_rows) return; // (whole groups of sixteen leave together)
  const unsigned int f = path_of(path_first, F, r);
  if (status[f] != ccmp::kRetimeOk) return; // an OK path's range has been checked
  const long long first = path_first[f], end = path_first[f + 1];
  if (r < first || r >= end) return;
  const long long i = r - first, R = end - first;
  const double inf = __builtin_inf();
  double v = inf, vp = inf, curv = inf, acc = inf;
  if (c < 14) {
    const double q = rows[(size_t)r * 14 + c];
    const bool has_next = i + 1 < R, has_prev = i > 0;
    const double d = has_next ? rows[(size_t)(r + 1) * 14 + c] - q : 0.0, dp = has_prev ? q - rows[(size_t)(r - 1) * 14 + c] : 0.0;
    const double vmax = lim.vmax[c], amax = lim.amax[c];
    if (has_next) { v = ccmp::retime_joint_v(vmax, d); acc = ccmp::retime_joint_acc(lim.beta, amax, d); }
    if (has_prev) vp = ccmp::retime_joint_v(vmax, dp);
    if (has_next && has_prev) curv = ccmp::retime_joint_curv(lim.beta, amax, d, dp);
  }
  v = min16(v); vp = min16(vp); curv = min16(curv); acc = min16(acc);
  if (c == 0) {
    ceiling[r] = (i == 0 || i == R - 1) ? 0.0 : ccmp::retime_ceiling(vp, v, curv);
    if (i + 1 < R) atomicMin(a_bits + f, (unsigned long long)__double_as_longlong(acc));
  }
}

__global__ __launch_bounds__(kThreads) void retime_envelope_kernel(const double *__restrict__ ceiling, const int32_t *__restrict__ path_first, unsigned int F,
                                                                  long long total_rows, const int32_t *__restrict__ status,
                                                                  const unsigned long long *__restrict__ a_bits, double *__restrict__ envelope)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const long long r = (long long)(t >> 4);
  const int c = (int)(t & 15);
  if (r >= total_rows) return;
  const unsigned int f = path_of(path_first, F, r);
  if (status[f] != ccmp::kRetimeOk) return;
  const long long first = path_first[f], end = path_first[f + 1];
  if (r < first || r >= end) return;
  const unsigned long long ab = a_bits[f];
  const double g = 2.0 * (ab == kNoA ? __builtin_inf() : __longlong_as_double((long long)ab)); // (one row: no other k, g is not used)
  double y = __builtin_inf();
  for (long long k = first + c; k < end; k += 16) {
    const double xk = ceiling[k];
    y = ccmp::retime_min(y, k == r ? xk : ccmp::retime_env_term(xk, g, k > r ? k - r : r - k));
  }
  y = min16(y);
  if (c == 0) envelope[r] = y;
}

__global__ __launch_bounds__(kWave) void retime_stamp_kernel(const double *__restrict__ rows, const double *__restrict__ envelope,
                                                            const int32_t *__restrict__ path_first, const int32_t *__restrict__ status,
                                                            const unsigned long long *__restrict__ a_bits, retime_limits lim, double *__restrict__ time,
                                                            double *__restrict__ duration)
{
  __shared__ double s_d[kWave], s_t[kWave];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int st = status[f];
  if (st != ccmp::kRetimeOk) { // block-uniform
    if (lane == 0) duration[f] = st == ccmp::kRetimeEmpty ? 0.0 : __builtin_nan("");
    return;
  }
  const long long first = path_first[f], R = (long long)path_first[f + 1] - first; // checked by the status kernel
  if (lane == 0) time[first] = 0.0;
  if (R == 1) {
    if (lane == 0) duration[f] = 0.0;
    return;
  }
  const double g = 2.0 * __longlong_as_double((long long)a_bits[f]);
  if (R == 2) {
    double v = __builtin_inf();
    if (lane < 14) v = ccmp::retime_joint_v(lim.vmax[lane], rows[(size_t)(first + 1) * 14 + lane] - rows[(size_t)first * 14 + lane]);
    v = min16(v);
    if (lane == 0) {
      const double t1 = 0.0 + ccmp::retime_dt_pair(v, g);
      time[first + 1] = t1;
      duration[f] = t1;
    }
    return;
  }
  double a = 0.0; // lane 0's running time
  for (long long base = 0; base < R - 1; base += kWave) { // block-uniform: every lane meets every barrier
    const long long left = R - 1 - base;
    const int m = left < kWave ? (int)left : kWave;
    const long long i = base + lane;
    if (lane < m) s_d[lane] = ccmp::retime_dt(envelope[first + i], envelope[first + i + 1]);
    __syncthreads();
    if (lane == 0)
      for (int q = 0; q < m; q++) {
        a = a + s_d[q];
        s_t[q] = a;
      }
    __syncthreads();
    if (lane < m) time[first + i + 1] = s_t[lane];
  }
  if (lane == 0) duration[f] = a;
}

}  // namespace

namespace ccmp_launch {

hipError_t retime_status(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, int32_t *status, unsigned long long *a_bits, hipStream_t st)
{
  hipLaunchKernelGGL(retime_status_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, rows, path_first, (long long)total_rows, status, a_bits);
  return hipGetLastError();
}

hipError_t resample_bracket(const double *rows, const double *arc, const int32_t *path_first, const int32_t *status, const int32_t *out_first, size_t F, size_t M,
                            size_t total_rows, double *x, int32_t *choice, uint8_t *kind, hipStream_t st)
{
  hipLaunchKernelGGL(resample_bracket_kernel, dim3(blocks_of(M * 16, kThreads)), dim3(kThreads), 0, st, rows, arc, path_first, status, out_first, (unsigned int)F,
                     (long long)M, (long long)total_rows, x, choice, kind);
  return hipGetLastError();
}

hipError_t resample_pick(const double *rows, const int32_t *out_first, size_t F, size_t M, size_t total_rows, const int32_t *choice, const uint8_t *kind_so_far,
                         const double *y, const uint8_t *ok, double *out_rows, uint8_t *kind, int32_t *counts, hipStream_t st)
{
  hipLaunchKernelGGL(resample_pick_kernel, dim3(blocks_of(M * 16, kThreads)), dim3(kThreads), 0, st, rows, out_first, (unsigned int)F, (long long)M,
                     (long long)total_rows, choice, kind_so_far, y, ok, out_rows, kind, counts);
  return hipGetLastError();
}

hipError_t retime_ceiling(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const int32_t *status, const ccmp::retime_limits &lim,
                          double *ceiling, unsigned long long *a_bits, hipStream_t st)
{
  hipLaunchKernelGGL(retime_ceiling_kernel, dim3(blocks_of(total_rows * 16, kThreads)), dim3(kThreads), 0, st, rows, path_first, (unsigned int)F,
                     (long long)total_rows, status, lim, ceiling, a_bits);
  return hipGetLastError();
}

hipError_t retime_envelope(const double *ceiling, const int32_t *path_first, size_t F, size_t total_rows, const int32_t *status, const unsigned long long *a_bits,
                           double *envelope, hipStream_t st)
{
  hipLaunchKernelGGL(retime_envelope_kernel, dim3(blocks_of(total_rows * 16, kThreads)), dim3(kThreads), 0, st, ceiling, path_first, (unsigned int)F,
                     (long long)total_rows, status, a_bits, envelope);
  return hipGetLastError();
}

hipError_t retime_stamp(const double *rows, const double *envelope, const int32_t *path_first, const int32_t *status, const unsigned long long *a_bits,
                        const ccmp::retime_limits &lim, size_t F, double *time, double *duration, hipStream_t st)
{
  hipLaunchKernelGGL(retime_stamp_kernel, dim3((unsigned int)F), dim3(kWave), 0, st, rows, envelope, path_first, status, a_bits, lim, time, duration);
  return hipGetLastError();
}

}  // namespace ccmp_launch
