// ccmp_kernels_dense.hip — dense solution paths on the device (ccmp_path_densify; the rule is csrc/ccmp_dense.h, compiled here and in
// ccmp_dense.cpp: one text, the same bits).  The traversals themselves are the extend step's kernels, unchanged; this unit moves rows
// and sums:
//   dense_gather_kernel     sixteen lanes per open segment of one extend call: from [14], to [14] and, for a continuation, carry_in [2].
//                           A first call reads its endpoints from the waypoint rows, a continuation the last stored row of the previous
//                           call's list and that call's carry row.
//   dense_pack_kernel       one wavefront per chunk (a waypoint row, or the rows one extend call contributes to one segment — possibly
//                           none): the rows go to their final place, lane 0 adds the call's Newton count to the segment's total (integer
//                           atomics: any order, the same sum).  A chunk that would reach beyond the result is skipped, never trusted.
//   dense_arc_kernel        one 64-lane block per path.  The arc is a serial chain of FP64 additions by definition; the loads are kept
//                           off it: the wavefront computes 64 joint distances at a time into LDS, then lane 0 adds them in row order, then
//                           the 64 arcs are stored coalesced.  Writes length[f] as well.
//   dense_clear_kernel      one 256-lane block per path over the clearance kernel's output: each lane keeps the lowest (value, row) of the
//                           rows first + lane, first + lane + 256, .. and the first row below the margin, then a tree in LDS; (value, row)
//                           is a total order, the smaller row wins a tie: no block shape changes the answer.
// No grid barrier, no spin; every loop carries its bound; lanes beyond the data are masked.
#include <hip/hip_runtime.h>

#include "ccmp_dense.h"
#include "ccmp_detmath.h"
#include "ccmp_launch.h"

namespace {

using ccmp::blocks_of;
using ccmp::dense_chunk;
using ccmp::dense_open_seg;
constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kNoRow = 0x7fffffff; // no candidate yet: behind every row

__global__ __launch_bounds__(kThreads) void dense_gather_kernel(const dense_open_seg *__restrict__ open, unsigned int E, const double *__restrict__ waypoints,
                                                               const double *__restrict__ prev_states, int chunk_states,
                                                               const double *__restrict__ prev_carry, double *__restrict__ from, double *__restrict__ to,
                                                               double *__restrict__ carry_in)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long k = t >> 4;
  const int c = (int)(t & 15);
  if (k >= E) return;
  const dense_open_seg s = open[k];
  if (c < 14) {
    const double *src = s.prev < 0 ? waypoints + (size_t)s.slot * 14 : prev_states + ((size_t)s.prev * (size_t)chunk_states + (size_t)s.last) * 14;
    from[k * 14 + c] = src[c];
    to[k * 14 + c] = waypoints[((size_t)s.slot + 1) * 14 + c];
  } else if (carry_in && s.prev >= 0) {
    carry_in[k * 2 + (c - 14)] = prev_carry[(size_t)s.prev * 2 + (c - 14)];
  }
}

__global__ __launch_bounds__(kThreads) void dense_pack_kernel(const dense_chunk *__restrict__ chunks, unsigned int n, double *__restrict__ rows,
                                                             unsigned long long total_rows, int32_t *__restrict__ seg_newton, unsigned int slots)
{
  const unsigned int id = blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  if (id >= n) return;
  const dense_chunk ch = chunks[id];
  if (ch.count < 0 || ch.dest < 0 || (unsigned long long)ch.dest + (unsigned long long)ch.count > total_rows) return;
  const int words = ch.count * 14;
  double *dst = rows + (size_t)ch.dest * 14;
  for (int j = lane; j < words; j += kWave) dst[j] = ch.src[j];
  if (lane == 0 && ch.its && ch.slot >= 0 && (unsigned int)ch.slot < slots) atomicAdd(seg_newton + ch.slot, *ch.its);
}

__global__ __launch_bounds__(kWave) void dense_arc_kernel(const double *__restrict__ rows, const int32_t *__restrict__ path_first, double *__restrict__ arc,
                                                         double *__restrict__ length)
{
  __shared__ double s_d[kWave], s_a[kWave];
  const int f = blockIdx.x, lane = threadIdx.x;
  const int first = path_first[f], end = path_first[f + 1];
  double a = 0.0; // lane 0's running arc
  for (int base = first; base < end; base += kWave) { // block-uniform: every lane meets every barrier
    const int left = end - base, m = left < kWave ? left : kWave;
    const int r = base + lane;
    double d = 0.0;
    if (lane < m && r > first) d = ccmp::graph_joint_dist(rows + (size_t)(r - 1) * 14, rows + (size_t)r * 14);
    s_d[lane] = d;
    __syncthreads();
    if (lane == 0)
      for (int j = 0; j < m; j++) {
        if (base + j > first) a = ccmp::dense_arc_step(a, s_d[j]);
        s_a[j] = a;
      }
    __syncthreads();
    if (lane < m) arc[r] = s_a[lane];
  }
  if (lane == 0) length[f] = a; // +0.0 for an empty path
}

__global__ __launch_bounds__(kThreads) void dense_clear_kernel(const double *__restrict__ clearance, const int32_t *__restrict__ path_first, double margin,
                                                              double *__restrict__ min_clear, int32_t *__restrict__ min_row, int32_t *__restrict__ first_blocked)
{
  __shared__ double s_v[kThreads];
  __shared__ int32_t s_r[kThreads], s_b[kThreads];
  const int f = blockIdx.x, t = threadIdx.x;
  const int first = path_first[f], end = path_first[f + 1];
  double v = __builtin_inf();
  int32_t row = kNoRow, blocked = kNoRow;
  for (long long r = (long long)first + t; r < end; r += kThreads) { // ascending rows: the first of equals stays
    const double c = clearance[r];
    if (ccmp::dense_lower(c, (int32_t)r, v, row)) { v = c; row = (int32_t)r; }
    if (c < margin && (int32_t)r < blocked) blocked = (int32_t)r;
  }
  s_v[t] = v; s_r[t] = row; s_b[t] = blocked;
  __syncthreads();
  for (int w = kThreads / 2; w > 0; w >>= 1) {
    if (t < w) {
      if (ccmp::dense_lower(s_v[t + w], s_r[t + w], s_v[t], s_r[t])) { s_v[t] = s_v[t + w]; s_r[t] = s_r[t + w]; }
      if (s_b[t + w] < s_b[t]) s_b[t] = s_b[t + w];
    }
    __syncthreads();
  }
  if (t == 0) {
    min_clear[f] = s_v[0];
    min_row[f] = s_r[0] == kNoRow ? -1 : s_r[0];
    first_blocked[f] = s_b[0] == kNoRow ? -1 : s_b[0];
  }
}

}  // namespace

namespace ccmp_launch {

hipError_t dense_gather(const ccmp::dense_open_seg *open, size_t E, const double *waypoints, const double *prev_states, int chunk_states,
                        const double *prev_carry, double *from, double *to, double *carry_in, hipStream_t st)
{
  hipLaunchKernelGGL(dense_gather_kernel, dim3(blocks_of(E * 16, kThreads)), dim3(kThreads), 0, st, open, (unsigned int)E, waypoints, prev_states, chunk_states,
                     prev_carry, from, to, carry_in);
  return hipGetLastError();
}

hipError_t dense_pack(const ccmp::dense_chunk *chunks, size_t n, double *rows, size_t total_rows, int32_t *seg_newton, size_t slots, hipStream_t st)
{
  hipLaunchKernelGGL(dense_pack_kernel, dim3(blocks_of(n, kThreads / kWave)), dim3(kThreads), 0, st, chunks, (unsigned int)n, rows, (unsigned long long)total_rows,
                     seg_newton, (unsigned int)slots);
  return hipGetLastError();
}

hipError_t dense_arc(const double *rows, const int32_t *path_first, size_t F, double *arc, double *length, hipStream_t st)
{
  hipLaunchKernelGGL(dense_arc_kernel, dim3((unsigned int)F), dim3(kWave), 0, st, rows, path_first, arc, length);
  return hipGetLastError();
}

hipError_t dense_clearance_summary(const double *clearance, const int32_t *path_first, size_t F, double margin, double *min_clear, int32_t *min_row,
                                   int32_t *first_blocked, hipStream_t st)
{
  hipLaunchKernelGGL(dense_clear_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, clearance, path_first, margin, min_clear, min_row, first_blocked);
  return hipGetLastError();
}

}  // namespace ccmp_launch
