// ccmp_kernels_smooth.hip — smooth solution paths on the device (ccmp_path_smooth; the rule is csrc/ccmp_smooth.h, compiled here and in
// ccmp_smooth.cpp: one text, the same bits).  The traversals and the projections are the extend step's and the projector's kernels,
// unchanged; this unit moves rows between them and decides:
//   smooth_load_kernel      sixteen lanes per waypoint row: the caller's rows into the call's first path buffer; a lane that meets a
//                           non-finite coordinate marks its path.
//   smooth_gather_kernel    sixteen lanes per pair of one stage of a pass.  The pair's path comes from a bisection on the active paths'
//                           prefixes.  Stage 0: (w_i, w_{i+1}) per segment; 1: (m_{i-1}, w_i) and (w_i, m_i) per interior vertex; 2: (t1, t2);
//                           3: the two checkMotion tests (m_{i-1}, c_i) and (c_i, m_i), as separate from / to rows.
//   smooth_bracket_kernel   sixteen lanes per pair: the bisection of the pair's monotone arc array for the bracket of half the arc, then
//                           lanes 0 .. 13 blend; lane 14 notes the fallback row (-1: degenerate).
//   smooth_pick_kernel      sixteen lanes per pair: projected, fallback or degenerate from the projector's flag; lane 14 counts.
//   smooth_accept_kernel    sixteen lanes per vertex of the subdivided path: the verdict on an interior vertex's candidate, the row into
//                           the other path buffer; lane 14 counts u and the stats (integer atomics: any order, the same totals).
//   smooth_length_kernel    one wavefront per path: the distances 64 at a time, then lane 0's left-to-right sum.
//   smooth_store_kernel     sixteen lanes per row of the result: rows behind out_len are not written.
// No grid barrier, no spin; every loop is bounded by its data; lanes beyond the data are masked.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_launch.h"
#include "ccmp_smooth.h"

namespace {

using ccmp::blocks_of;
using ccmp::path_of; // (ccmp_dense.h: the active path of an item, by its key)
using ccmp::smooth_path;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void smooth_load_kernel(const double *__restrict__ path_joints, const int32_t *__restrict__ path_len,
                                                              unsigned long long slots, int max_len, int cap, double *__restrict__ buf,
                                                              uint8_t *__restrict__ bad)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long s = t >> 4; // f * max_len + k
  const int c = (int)(t & 15);
  if (s >= slots || c >= 14) return;
  const unsigned long long f = s / (unsigned long long)max_len;
  const int k = (int)(s % (unsigned long long)max_len);
  if (k >= path_len[f] || k >= cap) return;
  const double v = path_joints[s * 14 + c];
  buf[(f * (unsigned long long)cap + (unsigned long long)k) * 14 + c] = v;
  if (!(v - v == 0.0)) bad[f] = 1; // every writer writes the same value
}

__global__ __launch_bounds__(kThreads) void smooth_gather_kernel(int stage, const smooth_path *__restrict__ paths, unsigned int nA, unsigned int E,
                                                                const double *__restrict__ cur, int cap, const double *__restrict__ m,
                                                                const double *__restrict__ t12, const double *__restrict__ cand,
                                                                double *__restrict__ pairs, double *__restrict__ from, double *__restrict__ to,
                                                                int32_t *__restrict__ pair_path)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long e = t >> 4;
  const int c = (int)(t & 15);
  if (e >= E) return;
  const long long item = stage == 0 ? (long long)e : (stage == 2 ? (long long)e : (long long)(e >> 1)); // a segment, or an interior vertex
  const unsigned int a = stage == 0 ? path_of(nA, item, [&](unsigned int x) { return (long long)paths[x].seg_first; })
                                    : path_of(nA, item, [&](unsigned int x) { return (long long)paths[x].vert_first; });
  const smooth_path P = paths[a];
  const double *rows = cur + (size_t)P.f * (size_t)cap * 14;
  const double *pa = nullptr, *pb = nullptr;
  if (stage == 0) {
    const long long i = item - P.seg_first;
    if (i < 0 || i + 1 >= P.L) return;
    pa = rows + (size_t)i * 14;
    pb = rows + (size_t)(i + 1) * 14;
  } else {
    const long long i = item - P.vert_first + 1; // the interior vertex
    if (i < 1 || i + 1 >= P.L) return;
    const int side = (int)(e & 1);
    const double *m_in = m + ((size_t)P.seg_first + (size_t)(i - 1)) * 14, *m_out = m + ((size_t)P.seg_first + (size_t)i) * 14;
    const double *w = rows + (size_t)i * 14;
    if (stage == 1) { pa = side ? w : m_in; pb = side ? m_out : w; }
    else if (stage == 2) { pa = t12 + (size_t)item * 28; pb = pa + 14; }
    else { const double *ci = cand + (size_t)item * 14; pa = side ? ci : m_in; pb = side ? m_out : ci; }
  }
  if (c < 14) {
    if (stage == 3) { from[e * 14 + c] = pa[c]; to[e * 14 + c] = pb[c]; }
    else { pairs[e * 28 + c] = pa[c]; pairs[e * 28 + 14 + c] = pb[c]; }
  } else if (c == 14 && pair_path) {
    pair_path[e] = P.f;
  }
}

__global__ __launch_bounds__(kThreads) void smooth_bracket_kernel(const double *__restrict__ rows, const double *__restrict__ arc,
                                                                 const int32_t *__restrict__ path_first, unsigned int E, long long total_rows,
                                                                 double *__restrict__ x, int32_t *__restrict__ choice)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long e = t >> 4;
  const int c = (int)(t & 15);
  if (e >= E) return;
  const long long first = path_first[e], n = (long long)path_first[e + 1] - first;
  if (first < 0 || n < 1 || first + n > total_rows) return; // never trusted
  int k;
  double tt;
  bool lower;
  const bool live = ccmp::smooth_bracket(arc + first, (int)n, &k, &tt, &lower);
  if (c < 14) {
    const double lo = rows[(size_t)(first + (live ? k - 1 : 0)) * 14 + c];
    x[e * 14 + c] = live ? ccmp::smooth_interpolate(lo, rows[(size_t)(first + k) * 14 + c], tt) : lo;
  } else if (c == 14) {
    choice[e] = live ? (int32_t)(first + (lower ? k - 1 : k)) : -1;
  }
}

__global__ __launch_bounds__(kThreads) void smooth_pick_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first,
                                                              const int32_t *__restrict__ choice, const double *__restrict__ y,
                                                              const uint8_t *__restrict__ ok, const int32_t *__restrict__ pair_path, unsigned int E,
                                                              long long total_rows, unsigned int F, double *__restrict__ mid, int32_t *__restrict__ stats)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long e = t >> 4;
  const int c = (int)(t & 15);
  if (e >= E) return;
  const long long first = path_first[e];
  const int32_t ch = choice[e];
  if (first < 0 || first >= total_rows || (long long)ch >= total_rows) return; // never trusted
  const int kind = ch < 0 ? ccmp::kSmoothDegenerate : (ok[e] ? ccmp::kSmoothProjected : ccmp::kSmoothFallback);
  if (c < 14) {
    mid[e * 14 + c] = kind == ccmp::kSmoothDegenerate ? rows[(size_t)first * 14 + c] : (kind == ccmp::kSmoothProjected ? y[e * 14 + c] : rows[(size_t)ch * 14 + c]);
  } else if (c == 14) {
    const int32_t f = pair_path[e];
    if (f >= 0 && (unsigned int)f < F) atomicAdd(stats + (size_t)f * ccmp::kSmoothStats + kind, 1);
  }
}

__global__ __launch_bounds__(kThreads) void smooth_accept_kernel(const smooth_path *__restrict__ paths, unsigned int nA, unsigned int items,
                                                                const double *__restrict__ cur, int cap, const double *__restrict__ m,
                                                                const double *__restrict__ cand, const uint8_t *__restrict__ test_ok,
                                                                const double *__restrict__ clear_m, const double *__restrict__ clear_c, double margin,
                                                                double min_change, double *__restrict__ next, int32_t *__restrict__ moved,
                                                                int32_t *__restrict__ stats)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long g = t >> 4;
  const int c = (int)(t & 15);
  if (g >= items) return;
  // active path a holds the new vertices [2 seg_first + a, ..): each path has 2 (L - 1) + 1 of them
  const unsigned int a = path_of(nA, (long long)g, [&](unsigned int x) { return 2ll * paths[x].seg_first + (long long)x; });
  const smooth_path P = paths[a];
  const long long j = (long long)g - (2ll * P.seg_first + (long long)a);
  if (j < 0 || j > 2ll * (P.L - 1) || j >= cap) return;
  const double *rows = cur + (size_t)P.f * (size_t)cap * 14;
  const double *src;
  if (j & 1) {
    src = m + ((size_t)P.seg_first + (size_t)(j >> 1)) * 14;
  } else {
    const long long i = j >> 1;
    src = rows + (size_t)i * 14;
    if (i >= 1 && i + 1 < P.L) {
      const size_t v = (size_t)P.vert_first + (size_t)(i - 1);
      const double *ci = cand + v * 14;
      const int verdict = ccmp::smooth_verdict(test_ok[2 * v], test_ok[2 * v + 1], clear_m != nullptr, clear_m ? clear_m[(size_t)P.seg_first + (size_t)(i - 1)] : 0.0,
                                               clear_c ? clear_c[v] : 0.0, margin, ccmp::graph_joint_dist(src, ci), min_change);
      if (verdict == 0) src = ci;
      if (c == 14) {
        if (verdict == 0) atomicAdd(moved + P.f, 1);
        else atomicAdd(stats + (size_t)P.f * ccmp::kSmoothStats + verdict, 1);
      }
    }
  }
  if (c < 14) next[((size_t)P.f * (size_t)cap + (size_t)j) * 14 + c] = src[c];
}

__global__ __launch_bounds__(64) void smooth_length_kernel(const double *__restrict__ buf0, const double *__restrict__ buf1, const uint8_t *__restrict__ where,
                                                          const int32_t *__restrict__ len, int cap, double *__restrict__ length)
{
  __shared__ double s_d[64];
  const int f = blockIdx.x, lane = threadIdx.x;
  int L = len[f];
  L = L < 0 ? 0 : (L > cap ? cap : L);
  const double *rows = ((where && where[f]) ? buf1 : buf0) + (size_t)f * (size_t)cap * 14;
  double a = 0.0;
  for (int base = 1; base < L; base += 64) { // block-uniform: every lane meets every barrier
    const int j = base + lane;
    if (j < L) s_d[lane] = ccmp::graph_joint_dist(rows + (size_t)(j - 1) * 14, rows + (size_t)j * 14);
    __syncthreads();
    if (lane == 0)
      for (int q = 0; q < 64 && base + q < L; q++) a = a + s_d[q];
    __syncthreads();
  }
  if (lane == 0) length[f] = a;
}

__global__ __launch_bounds__(kThreads) void smooth_store_kernel(const double *__restrict__ buf0, const double *__restrict__ buf1, const uint8_t *__restrict__ where,
                                                               const int32_t *__restrict__ len, unsigned long long slots, int cap,
                                                               double *__restrict__ out_joints)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long s = t >> 4; // f * cap + k
  const int c = (int)(t & 15);
  if (s >= slots || c >= 14) return;
  const unsigned long long f = s / (unsigned long long)cap;
  const int k = (int)(s % (unsigned long long)cap);
  if (k >= len[f]) return;
  out_joints[s * 14 + c] = (where[f] ? buf1 : buf0)[s * 14 + c];
}

}  // namespace

namespace ccmp_launch {

hipError_t smooth_load(const double *path_joints, const int32_t *path_len, size_t F, int max_len, int cap, double *buf, uint8_t *bad, hipStream_t st)
{
  const size_t slots = F * (size_t)max_len;
  hipLaunchKernelGGL(smooth_load_kernel, dim3(blocks_of(slots * 16, kThreads)), dim3(kThreads), 0, st, path_joints, path_len, (unsigned long long)slots, max_len,
                     cap, buf, bad);
  return hipGetLastError();
}

hipError_t smooth_gather(int stage, const ccmp::smooth_path *paths, size_t nA, size_t E, const double *cur, int cap, const double *m, const double *t12,
                         const double *cand, double *pairs, double *from, double *to, int32_t *pair_path, hipStream_t st)
{
  hipLaunchKernelGGL(smooth_gather_kernel, dim3(blocks_of(E * 16, kThreads)), dim3(kThreads), 0, st, stage, paths, (unsigned int)nA, (unsigned int)E, cur, cap, m,
                     t12, cand, pairs, from, to, pair_path);
  return hipGetLastError();
}

hipError_t smooth_bracket(const double *rows, const double *arc, const int32_t *path_first, size_t E, size_t total_rows, double *x, int32_t *choice,
                          hipStream_t st)
{
  hipLaunchKernelGGL(smooth_bracket_kernel, dim3(blocks_of(E * 16, kThreads)), dim3(kThreads), 0, st, rows, arc, path_first, (unsigned int)E,
                     (long long)total_rows, x, choice);
  return hipGetLastError();
}

hipError_t smooth_pick(const double *rows, const int32_t *path_first, const int32_t *choice, const double *y, const uint8_t *ok, const int32_t *pair_path,
                       size_t E, size_t total_rows, size_t F, double *mid, int32_t *stats, hipStream_t st)
{
  hipLaunchKernelGGL(smooth_pick_kernel, dim3(blocks_of(E * 16, kThreads)), dim3(kThreads), 0, st, rows, path_first, choice, y, ok, pair_path, (unsigned int)E,
                     (long long)total_rows, (unsigned int)F, mid, stats);
  return hipGetLastError();
}

hipError_t smooth_accept(const ccmp::smooth_path *paths, size_t nA, size_t items, const double *cur, int cap, const double *m, const double *cand,
                         const uint8_t *test_ok, const double *clear_m, const double *clear_c, double margin, double min_change, double *next,
                         int32_t *moved, int32_t *stats, hipStream_t st)
{
  hipLaunchKernelGGL(smooth_accept_kernel, dim3(blocks_of(items * 16, kThreads)), dim3(kThreads), 0, st, paths, (unsigned int)nA, (unsigned int)items, cur, cap, m,
                     cand, test_ok, clear_m, clear_c, margin, min_change, next, moved, stats);
  return hipGetLastError();
}

hipError_t smooth_length(const double *buf0, const double *buf1, const uint8_t *where, const int32_t *len, size_t F, int cap, double *length, hipStream_t st)
{
  hipLaunchKernelGGL(smooth_length_kernel, dim3((unsigned int)F), dim3(64), 0, st, buf0, buf1, where, len, cap, length);
  return hipGetLastError();
}

hipError_t smooth_store(const double *buf0, const double *buf1, const uint8_t *where, const int32_t *len, size_t F, int cap, double *out_joints,
                        hipStream_t st)
{
  const size_t slots = F * (size_t)cap;
  hipLaunchKernelGGL(smooth_store_kernel, dim3(blocks_of(slots * 16, kThreads)), dim3(kThreads), 0, st, buf0, buf1, where, len, (unsigned long long)slots, cap,
                     out_joints);
  return hipGetLastError();
}

}  // namespace ccmp_launch
