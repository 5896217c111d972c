// ccmp_kernels_shortcut.hip — shortcut solution paths on the device (ccmp_path_shortcut, ccmp_shortcut_select; the rule is
// csrc/ccmp_shortcut.h, compiled here and in ccmp_shortcut.cpp: one text, the same bits).  The traversals themselves are the extend
// step's kernels, unchanged; this unit enumerates, counts and searches:
//   shortcut_enumerate_kernel   sixteen lanes per pair slot of one tile.  The slot's path comes from a bisection on the prefix over paths,
//                               its (i, j) from the closed form of the rule: a tile may start and end inside a path.  Lanes 0 .. 13 move
//                               the endpoint rows, lane 14 writes the slot's matrix cell.  A slot with a non-finite row is no candidate:
//                               cell -1, zero rows.
//   shortcut_regather_kernel    sixteen lanes per open pair of a continuation: from = the last stored row of the previous call's list,
//                               to and the carry as they were.
//   shortcut_scatter_kernel     one lane per pair of an extend call: states and Newton rounds the call contributed are added to the pair's
//                               cells (integer additions; one lane owns a cell in any one call), the flag once the pair is no longer open.
//                               Without a cell array (explicit pairs: the smoothing's test step) slot k's cell is cell_base + k.
//   shortcut_select_kernel      one 256-lane block per path: d, hops, pred and the adjacent weights live in LDS; for each j the lanes fold
//                               the parents i = lane, lane + 256, .. < j, then a tree in LDS takes the lexicographic minimum — a total
//                               order, so no block shape changes the answer.  Lane 0 sums cost_in and walks pred.
//   shortcut_kept_kernel        sixteen lanes per kept row: out_joints[f][k] = path_joints[f][kept[f][k]].
// No grid barrier, no spin; every loop is bounded by L <= CCMP_SHORTCUT_MAX_LEN or by its data; lanes beyond the data are masked.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_launch.h"
#include "ccmp_shortcut.h"

namespace {

using ccmp::blocks_of;
using ccmp::shortcut_best;
using ccmp::shortcut_open;
constexpr int kThreads = 256;
constexpr int kMaxLen = CCMP_SHORTCUT_MAX_LEN;

__global__ __launch_bounds__(kThreads) void shortcut_enumerate_kernel(const double *__restrict__ path_joints, const int32_t *__restrict__ path_len,
                                                                     const long long *__restrict__ prefix, unsigned int F, int max_len, int max_span,
                                                                     long long first, unsigned int T, long long *__restrict__ cell,
                                                                     double *__restrict__ from, double *__restrict__ to)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long k = t >> 4;
  const int c = (int)(t & 15);
  if (k >= T) return;
  const long long g = first + (long long)k; // the slot's rank over all paths
  unsigned int lo = 0, hi = F - 1;          // the last path with prefix[f] <= g: paths without slots repeat their successor's prefix
  while (lo < hi) {
    const unsigned int mid = lo + (hi - lo + 1) / 2;
    if (prefix[mid] <= g) lo = mid; else hi = mid - 1;
  }
  const unsigned int f = lo;
  int L = path_len[f];
  L = L < 0 ? 0 : (L > max_len ? max_len : L);
  const long long r = g - prefix[f];
  bool cand = r >= 0 && r < ccmp::shortcut_pair_count(L, max_span); // a rank outside the enumeration moves nothing
  int i = 0, j = 0;
  if (cand) ccmp::shortcut_pair_of(L, max_span, r, &i, &j);
  cand = cand && i >= 0 && j < L && j - i >= 2;
  const double *wi = path_joints + ((size_t)f * (size_t)max_len + (size_t)i) * 14;
  const double *wj = path_joints + ((size_t)f * (size_t)max_len + (size_t)j) * 14;
  if (cand) cand = ccmp::shortcut_row_finite(wi) && ccmp::shortcut_row_finite(wj);
  if (c < 14) {
    from[k * 14 + c] = cand ? wi[c] : 0.0;
    to[k * 14 + c] = cand ? wj[c] : 0.0;
  } else if (c == 14) {
    cell[k] = cand ? ((long long)f * max_len + i) * (long long)max_len + j : -1;
  }
}

__global__ __launch_bounds__(kThreads) void shortcut_regather_kernel(const shortcut_open *__restrict__ open, unsigned int E,
                                                                    const double *__restrict__ prev_states, int chunk_states,
                                                                    const double *__restrict__ prev_to, const double *__restrict__ prev_carry,
                                                                    double *__restrict__ from, double *__restrict__ to, double *__restrict__ carry_in)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long k = t >> 4;
  const int c = (int)(t & 15);
  if (k >= E) return;
  const shortcut_open s = open[k];
  if (s.prev < 0 || s.last < 0 || s.last >= chunk_states) return; // never trusted
  if (c < 14) {
    from[k * 14 + c] = prev_states[((size_t)s.prev * (size_t)chunk_states + (size_t)s.last) * 14 + c];
    to[k * 14 + c] = prev_to[(size_t)s.prev * 14 + c];
  } else {
    carry_in[k * 2 + (c - 14)] = prev_carry[(size_t)s.prev * 2 + (c - 14)];
  }
}

__global__ __launch_bounds__(kThreads) void shortcut_scatter_kernel(const shortcut_open *__restrict__ open, unsigned int E, const long long *__restrict__ cell,
                                                                   long long cell_base, const int32_t *__restrict__ n_states, const uint8_t *__restrict__ ok,
                                                                   const int32_t *__restrict__ newton, const uint8_t *__restrict__ blocked,
                                                                   int chunk_states, unsigned long long cells, uint8_t *__restrict__ pair_ok,
                                                                   int32_t *__restrict__ pair_states, int32_t *__restrict__ pair_newton)
{
  const unsigned long long k = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (k >= E) return;
  const long long slot = open ? open[k].slot : (long long)k;
  const long long m = cell ? cell[slot] : cell_base + slot; // a tile of explicit pairs has no cell array: its entries are consecutive
  if (m < 0 || (unsigned long long)m >= cells) return; // no candidate
  const int32_t stored = ccmp::dense_stored(n_states[k], chunk_states);
  const int32_t add = open ? (stored > 0 ? stored - 1 : 0) : stored; // a continuation's row 0 repeats the state it started from
  if (pair_states) pair_states[m] += add;
  if (pair_newton) pair_newton[m] += newton[k];
  const bool final_ = (blocked && blocked[k]) || !ccmp::dense_open(n_states[k], ok[k], chunk_states);
  if (final_) pair_ok[m] = ok[k];
}

__global__ __launch_bounds__(kThreads) void shortcut_select_kernel(const double *__restrict__ path_joints, const int32_t *__restrict__ path_len, int max_len,
                                                                  const uint8_t *__restrict__ pair_ok, int32_t *__restrict__ out_len,
                                                                  int32_t *__restrict__ kept, double *__restrict__ cost_in, double *__restrict__ cost_out)
{
  __shared__ double s_d[kMaxLen], s_adj[kMaxLen], s_c[kThreads];
  __shared__ int32_t s_hops[kMaxLen], s_pred[kMaxLen], s_h[kThreads], s_i[kThreads];
  const int f = blockIdx.x, t = threadIdx.x;
  int L = path_len[f];
  L = (L < 0 || L > max_len || L > kMaxLen) ? 0 : L; // the host forms refuse such a length; here it is an empty path
  const double *rows = path_joints + (size_t)f * (size_t)max_len * 14;
  const uint8_t *okm = pair_ok + (size_t)f * (size_t)max_len * (size_t)max_len;
  int32_t *kp = kept + (size_t)f * (size_t)max_len;
  for (int j = t; j < L; j += kThreads) s_adj[j] = j > 0 ? ccmp::graph_joint_dist(rows + (size_t)(j - 1) * 14, rows + (size_t)j * 14) : 0.0;
  if (t == 0 && L > 0) { s_d[0] = 0.0; s_hops[0] = 0; s_pred[0] = -1; }
  __syncthreads();
  for (int j = 1; j < L; j++) { // block-uniform: every lane meets every barrier
    shortcut_best b = ccmp::shortcut_none();
    for (int i = t; i < j; i += kThreads) { // ascending parents per lane
      if (!ccmp::shortcut_admitted(i, j, i + 1 == j ? 1 : okm[(size_t)i * (size_t)max_len + (size_t)j])) continue;
      const double w = i + 1 == j ? s_adj[j] : ccmp::graph_joint_dist(rows + (size_t)i * 14, rows + (size_t)j * 14);
      ccmp::shortcut_relax(&b, i, s_d[i], s_hops[i], w);
    }
    s_c[t] = b.d; s_h[t] = b.parent_hops; s_i[t] = b.pred;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
      if (t < w && ccmp::shortcut_better(s_c[t + w], s_h[t + w], s_i[t + w], s_c[t], s_h[t], s_i[t])) {
        s_c[t] = s_c[t + w]; s_h[t] = s_h[t + w]; s_i[t] = s_i[t + w];
      }
      __syncthreads();
    }
    if (t == 0) {
      const bool reached = s_i[0] != ccmp::kShortcutNoPred;
      s_d[j] = reached ? s_c[0] : __builtin_inf();
      s_hops[j] = reached ? s_h[0] + 1 : ccmp::kPathNoHops;
      s_pred[j] = reached ? s_i[0] : -1;
    }
    __syncthreads();
  }
  const bool unchanged = L > 0 && s_hops[L - 1] == ccmp::kPathNoHops; // d[L - 1] == +inf: the path comes back as it is
  const int n = L == 0 ? 0 : (unchanged ? L : s_hops[L - 1] + 1);
  for (int k = t; k < max_len; k += kThreads) kp[k] = (unchanged && k < L) ? k : -1;
  __syncthreads();
  if (t == 0) {
    double a = 0.0;
    for (int j = 1; j < L; j++) a = a + s_adj[j];
    cost_in[f] = a;
    cost_out[f] = L == 0 ? 0.0 : s_d[L - 1];
    out_len[f] = n;
    if (!unchanged && L > 0) {
      int v = L - 1;
      for (int k = n - 1; k >= 0 && v >= 0 && v < L; k--) { // n <= L steps; pred descends
        kp[k] = v;
        v = s_pred[v];
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void shortcut_kept_kernel(const double *__restrict__ path_joints, const int32_t *__restrict__ out_len,
                                                                const int32_t *__restrict__ kept, unsigned long long slots, int max_len,
                                                                double *__restrict__ out_joints)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const unsigned long long s = t >> 4; // f * max_len + k
  const int c = (int)(t & 15);
  if (s >= slots || c >= 14) return;
  const unsigned long long f = s / (unsigned long long)max_len;
  const int k = (int)(s % (unsigned long long)max_len);
  if (k >= out_len[f]) return;
  const int v = kept[s];
  if (v < 0 || v >= max_len) return;
  out_joints[s * 14 + c] = path_joints[(f * (unsigned long long)max_len + (unsigned long long)v) * 14 + c];
}

}  // namespace

namespace ccmp_launch {

hipError_t shortcut_enumerate(const double *path_joints, const int32_t *path_len, const long long *prefix, size_t F, int max_len, int max_span,
                              long long first, size_t T, long long *cell, double *from, double *to, hipStream_t st)
{
  hipLaunchKernelGGL(shortcut_enumerate_kernel, dim3(blocks_of(T * 16, kThreads)), dim3(kThreads), 0, st, path_joints, path_len, prefix, (unsigned int)F, max_len,
                     max_span, first, (unsigned int)T, cell, from, to);
  return hipGetLastError();
}

hipError_t shortcut_regather(const ccmp::shortcut_open *open, size_t E, const double *prev_states, int chunk_states, const double *prev_to,
                             const double *prev_carry, double *from, double *to, double *carry_in, hipStream_t st)
{
  hipLaunchKernelGGL(shortcut_regather_kernel, dim3(blocks_of(E * 16, kThreads)), dim3(kThreads), 0, st, open, (unsigned int)E, prev_states, chunk_states, prev_to,
                     prev_carry, from, to, carry_in);
  return hipGetLastError();
}

hipError_t shortcut_scatter(const ccmp::shortcut_open *open, size_t E, const long long *cell, long long cell_base, const int32_t *n_states, const uint8_t *ok,
                            const int32_t *newton, const uint8_t *blocked, int chunk_states, size_t cells, uint8_t *pair_ok, int32_t *pair_states,
                            int32_t *pair_newton, hipStream_t st)
{
  hipLaunchKernelGGL(shortcut_scatter_kernel, dim3(blocks_of(E, kThreads)), dim3(kThreads), 0, st, open, (unsigned int)E, cell, cell_base, n_states, ok, newton, blocked,
                     chunk_states, (unsigned long long)cells, pair_ok, pair_states, pair_newton);
  return hipGetLastError();
}

hipError_t shortcut_select(const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok, int32_t *out_len,
                           int32_t *kept, double *cost_in, double *cost_out, hipStream_t st)
{
  hipLaunchKernelGGL(shortcut_select_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, path_joints, path_len, max_len, pair_ok, out_len, kept, cost_in,
                     cost_out);
  return hipGetLastError();
}

hipError_t shortcut_gather_kept(const double *path_joints, const int32_t *out_len, const int32_t *kept, size_t F, int max_len, double *out_joints,
                                hipStream_t st)
{
  const size_t slots = F * (size_t)max_len;
  hipLaunchKernelGGL(shortcut_kept_kernel, dim3(blocks_of(slots * 16, kThreads)), dim3(kThreads), 0, st, path_joints, out_len, kept,
                     (unsigned long long)slots, max_len, out_joints);
  return hipGetLastError();
}

}  // namespace ccmp_launch
