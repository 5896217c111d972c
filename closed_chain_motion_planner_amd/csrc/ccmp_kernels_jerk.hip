// ccmp_kernels_jerk.hip — jerk-bounded setpoints on the device (ccmp_path_jerk_setpoints; the rule is csrc/ccmp_jerk.h, compiled here and in
// ccmp_jerk.cpp: one text, the same bits).  The status scan and the tangents are the setpoints unit's launchers, unchanged; the gap,
// isSatisfied and the clearance of the ticks are the function, is-satisfied and clearance launchers, unchanged.  This unit searches the
// window, samples and audits:
//   jerk_measure_kernel   the hot path of the window search.  One block per tile of T output ticks of one open path (the tile's path by
//                         bisection on tile_first).  The T + W + 1 input velocities the tile's windows and its two look-ahead ticks need are
//                         computed from rows, stamps and tangents, sixteen lanes per input tick, lanes 0 .. 13 one joint each, and parked in
//                         LDS; then every output tick's window is summed from LDS in the rule's order, oldest to newest, and divided once;
//                         then sixteen lanes per output tick form a_j, a_{j+1} and the jerk share, fold the joints with DPP row rotations,
//                         the block folds its lanes, and ONE 64-bit unsigned atomic maximum on the bit pattern goes into P[f] (the values
//                         are non-negative doubles, which order as their bits).  No x, q or qd array exists in memory during the search.
//   jerk_decide_kernel    one lane per path: the first call opens the paths (setpoints status, first window, M or FULL); every later one
//                         reads and clears P[f] and decides OK / WINDOW / FULL / the next W.  word[f] = M of an open path, -1 - M of a closed.
//   jerk_sample_kernel    one block per tile of a delivered path's ticks: both parts of x staged the same way, q, qd, tau of every tick
//                         with the path's final W, the copies at both ends, the NaN a clearance holds until a scene has answered.
//   jerk_peak_kernel      one 256-lane block per path: audit_fold of ccmp_lanes.h (setpoints_peak_kernel's too) with six columns, the
//                         widths from the rule's grid and no stretch.  Its jerk peak is the P the last measurement saw: the same functions
//                         on the same bits.
// A tick of the interpolant (input_of) is the setpoints rule's setpoint_bracket and setpoint_joint; the DPP row folds are ccmp_lanes.h's.
// No grid barrier, no spin; every loop is bounded by its data or by a constant; lanes beyond the data are masked; every offset read from
// memory is range-checked before use.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_jerk.h"
#include "ccmp_lanes.h"
#include "ccmp_launch.h"

namespace {

using ccmp::blocks_of;
using ccmp::jerk_limits;
using ccmp::path_of;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kTile = ccmp_launch::kJerkTile;             // output ticks per block of the measure kernel at most
constexpr int kSampleTile = ccmp_launch::kJerkSampleTile; // ... of the sample kernel, which stages both parts of x
constexpr int kMaxW = ccmp::kJerkMaxWindow;
using ccmp_lanes::bits_of;
using ccmp_lanes::row_max;
using ccmp_lanes::row_or;
using ccmp_lanes::u64;
using ccmp_lanes::value_of;

// static LDS of the two staging kernels: both within the 64 KB a block may have
static_assert(((kTile + kMaxW + 1) + (kTile + 2)) * 14 * sizeof(double) + 64 <= 65536, "jerk_measure_kernel: LDS");
static_assert((kSampleTile + kMaxW - 1) * 28 * sizeof(double) <= 65536, "jerk_sample_kernel: LDS");

// One path as the staging kernels see it, range-checked: rows r, stamps t, tangents w of its R >= 2 rows, n tick intervals
struct PathView {
  const double *r, *t, *w;
  long long R, n;
  double D;
};

// x_i of the rule for joint c < 14: *xq its position part, the return value its velocity part.  The sixteen lanes of a group share i.
__device__ __forceinline__ double input_of(const PathView &p, long long i, int c, double period, double *xq)
{
  if (i <= 0) { *xq = p.r[c]; return 0.0; }
  if (i >= p.n) { *xq = p.r[(size_t)(p.R - 1) * 14 + c]; return 0.0; }
  int k;
  double at, u, xd;
  // (false: the rule's own precondition of the bracket; an OK path meets it)
  if (!ccmp::setpoint_bracket(p.t, (int)p.R, i, p.n + 1, period, p.D, &at, &k, &u)) { *xq = p.r[c]; return 0.0; }
  ccmp::setpoint_joint(p.r + c, p.w + c, p.t, k, u, xq, &xd);
  return xd;
}

__global__ __launch_bounds__(kThreads) void jerk_measure_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                               const double *__restrict__ time, const double *__restrict__ tangent,
                                                               const int32_t *__restrict__ tile_first, const int32_t *__restrict__ word,
                                                               const int32_t *__restrict__ window, const int32_t *__restrict__ sp_ticks, unsigned int F,
                                                               long long total_rows, double period, int T, jerk_limits lim, u64 *__restrict__ P)
{
  __shared__ double s_x[(kTile + kMaxW + 1) * 14]; // the velocity parts of x_{j0-W+1} .. x_{j0+T+1}
  __shared__ double s_v[(kTile + 2) * 14];         // the filtered qd of ticks j0 .. j0 + T + 1
  __shared__ double s_m[kThreads / kWave];
  const int t = threadIdx.x;
  const unsigned int f = path_of(tile_first, F, (long long)blockIdx.x);
  const long long tile = (long long)blockIdx.x - tile_first[f];
  const long long M = word[f], first = path_first[f], R = (long long)path_first[f + 1] - first, n = (long long)sp_ticks[f] - 1;
  const int W = window[f];
  // block-uniform, never trusted: an open path, its tile, its range, the window and the tile length within the LDS above
  if (T < 1 || T > kTile || W < 1 || W > kMaxW || tile < 0 || M < 3 || n < 1 || M != n + W || tile * T >= M || first < 0 || R < 2 || first + R > total_rows) return;
  const long long j0 = tile * T;
  PathView p = {rows + (size_t)first * 14, time + first, tangent + (size_t)first * 14, R, n, time[first + R - 1]};
  const int c = t & 15;
  // 1. the inputs: sixteen lanes per input tick
  const int n_in = T + W + 1;
  for (int idx = t >> 4; idx < n_in; idx += kThreads / 16) {
    if (c < 14) {
      double xq;
      s_x[idx * 14 + c] = input_of(p, j0 - W + 1 + idx, c, period, &xq);
    }
  }
  __syncthreads();
  // 2. the windows of the ticks j0 .. j0 + T + 1 that exist: one (tick, joint) per lane and step
  for (int e = t; e < (T + 2) * 14; e += kThreads) {
    const int tt = e / 14, cc = e - tt * 14;
    const long long j = j0 + tt;
    if (j >= M) continue;
    double sum = s_x[tt * 14 + cc];
    for (int k = 1; k < W; k++) sum = sum + s_x[(tt + k) * 14 + cc];
    s_v[e] = j == 0 || j == M - 1 ? 0.0 : ccmp::jerk_mean(sum, W);
  }
  __syncthreads();
  // 3. the jerk shares of the middle ticks j + 1, j = j0 .. j0 + T - 1 with j <= M - 3: sixteen lanes per tick (whole DPP rows take the same way)
  double best = 0.0;
  for (int base = 0; base < T * 16; base += kThreads) { // block-uniform
    const int tt = (base + t) >> 4;
    const long long j = j0 + tt;
    double s = 0.0;
    int nan = 0;
    if (tt < T && j + 2 < M && c < 14) {
      s = ccmp::jerk_share(s_v[tt * 14 + c], s_v[(tt + 1) * 14 + c], s_v[(tt + 2) * 14 + c], j, period, lim.jmax[c]);
      if (s != s) { nan = 1; s = 0.0; }
    }
    s = row_max(s);
    nan = row_or(nan);
    if (!nan && s > best) best = s; // a NaN share: the tick does not contribute
  }
  for (int m = kWave / 2; m > 0; m >>= 1) {
    const double o = __shfl_xor(best, m);
    best = o > best ? o : best;
  }
  if ((t & (kWave - 1)) == 0) s_m[t / kWave] = best;
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < kThreads / kWave; w++) best = s_m[w] > best ? s_m[w] : best;
    if (best > 0.0) atomicMax(P + f, bits_of(best)); // (+0.0 is what P holds already)
  }
}

__global__ __launch_bounds__(kThreads) void jerk_decide_kernel(const int32_t *__restrict__ sp_status, const int32_t *__restrict__ sp_ticks, unsigned int F, int begin,
                                                              int fixed, int max_window, double aim, int max_ticks, u64 *__restrict__ P,
                                                              int32_t *__restrict__ status, int32_t *__restrict__ window, int32_t *__restrict__ passes,
                                                              int32_t *__restrict__ word)
{
  const unsigned int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= F) return;
  const int st = sp_status[f];
  const long long n = (long long)sp_ticks[f] - 1;
  if (begin) {
    P[f] = 0;
    passes[f] = 0;
    if (st != ccmp::kSetpointsOk || n < 1) { // the setpoints status ends the path: one tick for a POINT, none for the others
      status[f] = st != ccmp::kSetpointsOk ? st : ccmp::kSetpointsEmpty; // (never the latter: an OK path has N >= 2)
      window[f] = st == ccmp::kSetpointsFull ? (fixed ? fixed : 1) : 0; // FULL names the window that did not fit
      word[f] = -1 - (st == ccmp::kSetpointsPoint ? 1 : 0);
      return;
    }
    const int W = fixed ? fixed : 1;
    const int32_t M = ccmp::jerk_ticks(n, W, max_ticks);
    window[f] = W;
    status[f] = M ? ccmp::kJerkOpen : ccmp::kJerkFull;
    word[f] = M ? M : -1;
    return;
  }
  if (status[f] != ccmp::kJerkOpen) return; // a path that is done is never touched again
  const double peak = value_of(P[f]);
  P[f] = 0;
  const int W = window[f];
  const int32_t M = word[f];
  if (peak <= 1.0 || fixed || W >= max_window) {
    status[f] = peak <= 1.0 ? ccmp::kJerkOk : ccmp::kJerkWindow;
    word[f] = -1 - M;
    return;
  }
  const int next = ccmp::jerk_next_window(W, peak, aim, max_window);
  const int32_t Mn = ccmp::jerk_ticks(n, next, max_ticks);
  window[f] = next;
  passes[f] = passes[f] + 1;
  if (!Mn) status[f] = ccmp::kJerkFull;
  word[f] = Mn ? Mn : -1;
}

__global__ __launch_bounds__(kThreads) void jerk_sample_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                              const double *__restrict__ time, const double *__restrict__ tangent,
                                                              const int32_t *__restrict__ tile_first, const int32_t *__restrict__ tick_first,
                                                              const int32_t *__restrict__ status, const int32_t *__restrict__ window,
                                                              const int32_t *__restrict__ sp_ticks, unsigned int F, long long total_ticks, long long total_rows,
                                                              double period, int T, double *__restrict__ q, double *__restrict__ qd, double *__restrict__ tau,
                                                              double *__restrict__ clearance)
{
  __shared__ double s_q[(kSampleTile + kMaxW - 1) * 14], s_d[(kSampleTile + kMaxW - 1) * 14]; // both parts of x_{j0-W+1} .. x_{j0+T-1}
  const int t = threadIdx.x;
  const unsigned int f = path_of(tile_first, F, (long long)blockIdx.x);
  const long long tile = (long long)blockIdx.x - tile_first[f];
  const long long g0 = tick_first[f], M = (long long)tick_first[f + 1] - g0;
  const long long first = path_first[f], R = (long long)path_first[f + 1] - first;
  const int st = status[f], W = window[f];
  // block-uniform, never trusted
  if (T < 1 || T > kSampleTile || tile < 0 || g0 < 0 || M < 1 || g0 + M > total_ticks || tile * T >= M || first < 0 || R < 1 || first + R > total_rows) return;
  if (st == ccmp::kSetpointsPoint) { // one tick: the row, at rest
    if (M != 1) return;
    if (t < 14) { q[(size_t)g0 * 14 + t] = rows[(size_t)first * 14 + t]; qd[(size_t)g0 * 14 + t] = 0.0; }
    else if (t == 14) tau[g0] = 0.0;
    else if (t == 15) clearance[g0] = __builtin_nan("");
    return;
  }
  const long long n = (long long)sp_ticks[f] - 1;
  if ((st != ccmp::kJerkOk && st != ccmp::kJerkWindow) || W < 1 || W > kMaxW || R < 2 || n < 1 || M != n + W) return;
  const long long j0 = tile * T;
  PathView p = {rows + (size_t)first * 14, time + first, tangent + (size_t)first * 14, R, n, time[first + R - 1]};
  const int c = t & 15;
  const int n_in = T + W - 1;
  for (int idx = t >> 4; idx < n_in; idx += kThreads / 16) {
    if (c < 14) {
      double xq;
      s_d[idx * 14 + c] = input_of(p, j0 - W + 1 + idx, c, period, &xq);
      s_q[idx * 14 + c] = xq;
    }
  }
  __syncthreads();
  for (int e = t; e < T * 16; e += kThreads) {
    const int tt = e >> 4;
    const long long j = j0 + tt;
    if (j >= M) continue;
    const size_t g = (size_t)(g0 + j);
    if (c < 14) {
      double x, xd = 0.0;
      if (j == 0) {
        x = p.r[c];
      } else if (j == M - 1) {
        x = p.r[(size_t)(R - 1) * 14 + c];
      } else {
        double sq = s_q[tt * 14 + c], sd = s_d[tt * 14 + c];
        for (int k = 1; k < W; k++) {
          sq = sq + s_q[(tt + k) * 14 + c];
          sd = sd + s_d[(tt + k) * 14 + c];
        }
        x = ccmp::jerk_mean(sq, W);
        xd = ccmp::jerk_mean(sd, W);
      }
      q[g * 14 + c] = x;
      qd[g * 14 + c] = xd;
    } else if (c == 14) {
      tau[g] = ccmp::jerk_tau(j, period);
    } else {
      clearance[g] = __builtin_nan("");
    }
  }
}

// the audit's trait (ccmp_lanes.h: audit_fold): six columns, the widths from the rule's own grid, the jerk share at the middle tick, no stretch
struct JerkAudit {
  static constexpr int kCols = ccmp::kJerkPeaks, kSpeed = ccmp::kJerkPeakSpeed, kAcc = ccmp::kJerkPeakAcc, kJerk = ccmp::kJerkPeakJerk, kDp = ccmp::kJerkPeakDp,
                       kAngle = ccmp::kJerkPeakAngle, kClearance = ccmp::kJerkPeakClearance;
  static constexpr bool kStretch = false;
  double period;
  const double *jmax;
  __device__ double width(size_t, long long j) const { return ccmp::jerk_tau(j + 1, period) - ccmp::jerk_tau(j, period); }
  __device__ double jerk(const double *qd, size_t g, long long j, int c) const
  {
    return ccmp::jerk_share(qd[(g - 1) * 14 + c], qd[g * 14 + c], qd[(g + 1) * 14 + c], j - 1, period, jmax[c]);
  }
};

__global__ __launch_bounds__(kThreads) void jerk_peak_kernel(const double *__restrict__ qd, const double *__restrict__ fgap, const uint8_t *__restrict__ satisfied,
                                                            const double *__restrict__ clearance, const int32_t *__restrict__ tick_first, long long total_ticks,
                                                            double period, jerk_limits lim, double margin, double *__restrict__ peak,
                                                            int32_t *__restrict__ peak_tick, int32_t *__restrict__ counts)
{
  ccmp_lanes::audit_fold<JerkAudit, kThreads>(JerkAudit{period, lim.jmax}, lim.vmax, lim.amax, qd, fgap, satisfied, clearance, tick_first, total_ticks, margin, peak,
                                              peak_tick, counts, nullptr);
}

}  // namespace

namespace ccmp_launch {

hipError_t jerk_measure(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *tile_first, size_t tiles,
                        const int32_t *word, const int32_t *window, const int32_t *sp_ticks, size_t F, size_t total_rows, double period, int tile_ticks,
                        const ccmp::jerk_limits &lim, unsigned long long *P, hipStream_t st)
{
  hipLaunchKernelGGL(jerk_measure_kernel, dim3((unsigned int)tiles), dim3(kThreads), 0, st, rows, path_first, time, tangent, tile_first, word, window, sp_ticks,
                     (unsigned int)F, (long long)total_rows, period, tile_ticks, lim, P);
  return hipGetLastError();
}

hipError_t jerk_decide(const int32_t *sp_status, const int32_t *sp_ticks, size_t F, bool begin, int fixed_window, int max_window, double aim, int max_ticks,
                       unsigned long long *P, int32_t *status, int32_t *window, int32_t *passes, int32_t *word, hipStream_t st)
{
  hipLaunchKernelGGL(jerk_decide_kernel, dim3(blocks_of(F, kThreads)), dim3(kThreads), 0, st, sp_status, sp_ticks, (unsigned int)F, begin ? 1 : 0, fixed_window,
                     max_window, aim, max_ticks, P, status, window, passes, word);
  return hipGetLastError();
}

hipError_t jerk_sample(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *tile_first, size_t tiles,
                       const int32_t *tick_first, const int32_t *status, const int32_t *window, const int32_t *sp_ticks, size_t F, size_t total_ticks,
                       size_t total_rows, double period, int tile_ticks, double *q, double *qd, double *tau, double *clearance, hipStream_t st)
{
  hipLaunchKernelGGL(jerk_sample_kernel, dim3((unsigned int)tiles), dim3(kThreads), 0, st, rows, path_first, time, tangent, tile_first, tick_first, status, window,
                     sp_ticks, (unsigned int)F, (long long)total_ticks, (long long)total_rows, period, tile_ticks, q, qd, tau, clearance);
  return hipGetLastError();
}

hipError_t jerk_peak(const double *qd, const double *f, const uint8_t *satisfied, const double *clearance, const int32_t *tick_first, size_t F, size_t total_ticks,
                     double period, const ccmp::jerk_limits &lim, double margin, double *peak, int32_t *peak_tick, int32_t *counts, hipStream_t st)
{
  hipLaunchKernelGGL(jerk_peak_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, qd, f, satisfied, clearance, tick_first, (long long)total_ticks, period, lim,
                     margin, peak, peak_tick, counts);
  return hipGetLastError();
}

}  // namespace ccmp_launch
