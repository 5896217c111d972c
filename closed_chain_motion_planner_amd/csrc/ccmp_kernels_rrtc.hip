// ccmp_kernels_rrtc.hip — RRT-Connect on the roadmap store (ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree; the rule: csrc/ccmp_rrtc.h): the
// kernels between the sampler, the traversals and the graph calls of a cycle.  None waits for another or spins, every loop is bounded by
// an argument or a constant, every vertex index is range-checked before it addresses a row, registers and LDS only.
//   rrtc_nearest_kernel        blocks over (query, partition) — the queries on the grid's x, which takes 2^31 - 1 of them: a lane strides over the partition's rows, keeps those whose label is one of
//                              the <= 8 root labels (wave-uniform: scalar registers), takes graph_joint_dist — FP64, the k-NN's FMA chain —
//                              and keeps its best (distance, index); the bests are reduced by PAIR COMPARISON across the wavefront
//                              (shuffles) and across the block's four wavefronts (LDS).  No atomics on floats: (distance, index) is a total
//                              order, so no launch shape changes the answer.  More than one partition: the bests go to a workspace and
//   rrtc_nearest_merge_kernel  reduces them the same way, one block per query.
//   rrtc_edges_kernel          what the traversal sees: from = the nearest vertex's joints, to = the query row, and use = 0 (a flag says the
//                              row is no sample / no vertex), 2 (no nearest vertex) or 1; an unused edge runs from a zero row to a zero row
//                              (no NaN endpoint reaches a traversal)
//   rrtc_pick_kernel           one edge per group of sixteen lanes, lane c < 14 holds component c of the listed state at hand.  The partial
//                              sums are taken serially in list order — the order is the rule's — each step's FMA chain over the components
//                              fed by shuffles within the group.  Writes the outcome, the new row and its parent.
//   rrtc_commit_kernel         ONE block, width <= 256: an exclusive scan over the keep flags gives step 4's total order; writes the compact
//                              rows, the uv entries, the counts the host reads, the tallies and the state update (next_index, best_gap)
// The cycle's solution test is ccmp_kernels_plan.hip's plan_connected_kernel, instantiated there for ccmp_rrtc_state.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_graph.h"
#include "ccmp_launch.h"
#include "ccmp_rrtc.h"

namespace {

using ccmp_launch::GraphStore;
using ccmp_launch::RrtcCommit;
using ccmp_launch::RrtcPick;
constexpr int kWave = 64;
constexpr int kThreads = ccmp_launch::kRrtcThreads;
constexpr int kEmptyIdx = 0x7fffffff;
constexpr int kGroup = 16;

// the block's 256 bests -> lane 0's (d, i): shuffles within a wavefront, LDS across the four
__device__ __forceinline__ void best_reduce(double &d, int &i, double *ld, int *li)
{
#pragma unroll
  for (int off = kWave / 2; off >= 1; off >>= 1) {
    const double od = __shfl_xor(d, off, kWave);
    const int oi = __shfl_xor(i, off, kWave);
    if (ccmp::graph_closer(od, oi, d, i)) { d = od; i = oi; }
  }
  const int t = threadIdx.x, w = t / kWave;
  if ((t & (kWave - 1)) == 0) { ld[w] = d; li[w] = i; }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 1; k < kThreads / kWave; k++)
      if (ccmp::graph_closer(ld[k], li[k], d, i)) { d = ld[k]; i = li[k]; }
  }
}

__global__ __launch_bounds__(kThreads) void rrtc_nearest_kernel(const GraphStore s, const int32_t *__restrict__ roots, int n_roots,
                                                                const double *__restrict__ queries, unsigned int part, int P, double *ws_d, int32_t *ws_i,
                                                                int32_t *idx, double *dist)
{
  __shared__ double ld[kThreads / kWave];
  __shared__ int li[kThreads / kWave];
  const int t = threadIdx.x, p = blockIdx.y;
  const size_t q = blockIdx.x;
  const unsigned int N = (unsigned int)s.N;
  int32_t lab[CCMP_RRTC_MAX_ROOTS];
  const int nl = ccmp::rrtc_root_labels(roots, n_roots, s.labels, s.N, lab); // the same for every lane
  double x[14];
#pragma unroll
  for (int c = 0; c < 14; c++) x[c] = queries[q * 14 + c];
  double bd = __builtin_inf();
  int bi = kEmptyIdx;
  if (nl > 0) {
    const unsigned int lo = (unsigned int)p * part, hi = lo + part < N ? lo + part : N;
    for (unsigned int j = lo + t; j < hi; j += kThreads) {
      if (!ccmp::rrtc_in_tree(s.labels[j], lab)) continue;
      const double d = ccmp::graph_joint_dist(s.joints + (size_t)j * 14, x);
      if (ccmp::graph_closer(d, (int)j, bd, bi)) { bd = d; bi = (int)j; } // a NaN distance is below nothing
    }
  }
  best_reduce(bd, bi, ld, li);
  if (t != 0) return;
  if (P == 1) {
    idx[q] = bi == kEmptyIdx ? -1 : bi;
    dist[q] = bd;
  } else {
    ws_d[q * (size_t)P + p] = bd;
    ws_i[q * (size_t)P + p] = bi;
  }
}

__global__ __launch_bounds__(kThreads) void rrtc_nearest_merge_kernel(int P, const double *__restrict__ ws_d, const int32_t *__restrict__ ws_i, int32_t *idx,
                                                                      double *dist)
{
  __shared__ double ld[kThreads / kWave];
  __shared__ int li[kThreads / kWave];
  const int t = threadIdx.x;
  const size_t q = blockIdx.x;
  double d = t < P ? ws_d[q * (size_t)P + t] : __builtin_inf();
  int i = t < P ? ws_i[q * (size_t)P + t] : kEmptyIdx;
  best_reduce(d, i, ld, li);
  if (t == 0) {
    idx[q] = i == kEmptyIdx ? -1 : i;
    dist[q] = d;
  }
}

__global__ __launch_bounds__(kThreads) void rrtc_edges_kernel(const GraphStore s, const int32_t *__restrict__ idx, const double *__restrict__ rows,
                                                              const uint8_t *__restrict__ f0, const uint8_t *__restrict__ f1, const uint8_t *__restrict__ f2,
                                                              unsigned int E, double *__restrict__ from, double *__restrict__ to, uint8_t *__restrict__ use)
{
  const unsigned int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= E) return;
  const bool on = (!f0 || f0[e]) && (!f1 || f1[e]) && (!f2 || f2[e]);
  const int32_t n = idx[e];
  const bool has = n >= 0 && (unsigned long long)n < s.N;
  const uint8_t u = !on ? 0 : has ? 1 : 2;
  use[e] = u;
#pragma unroll
  for (int c = 0; c < 14; c++) {
    from[(size_t)e * 14 + c] = u == 1 ? s.joints[(size_t)n * 14 + c] : 0.0;
    to[(size_t)e * 14 + c] = u == 1 ? rows[(size_t)e * 14 + c] : 0.0;
  }
}

// graph_joint_dist(a, b) of the rows whose component `lane` this lane holds: the same chain, its operands fetched within the group
__device__ __forceinline__ double group_dist(double a, double b)
{
  const double e = a - b;
  double d2 = 0.0;
#pragma unroll
  for (int c = 0; c < 14; c++) {
    const double ec = __shfl(e, c, kGroup);
    d2 = CCMP_FMA(ec, ec, d2);
  }
  return ccmp_sqrt(d2);
}

__global__ __launch_bounds__(kThreads) void rrtc_pick_kernel(const RrtcPick c)
{
  const unsigned int e = (blockIdx.x * kThreads + threadIdx.x) / kGroup;
  const int lane = threadIdx.x & (kGroup - 1);
  if (e >= c.E) return; // a whole group leaves together
  const int ms = c.max_states;
  const uint8_t use = c.use ? c.use[e] : 1;
  const int32_t ns = c.n_states[e];
  const int m = use != 1 ? 0 : ns < 0 ? 0 : ns > ms ? ms : ns;
  const double *st = c.states + (size_t)e * ms * 14;
  const bool comp = lane < 14;
  const double tgt = comp ? c.to[(size_t)e * 14 + lane] : 0.0;
  int32_t outcome, row = -1;
  double gap = __builtin_nan("");
  if (c.mode == 0) {
    ccmp::rrtc_arc a;
    ccmp::rrtc_arc_begin(&a);
    double prev = comp && m > 0 ? st[lane] : 0.0;
    for (int i = 1; i < m; i++) {
      const double cur = comp ? st[(size_t)i * 14 + lane] : 0.0;
      ccmp::rrtc_arc_step(&a, i, group_dist(prev, cur), c.range);
      prev = cur;
    }
    outcome = use == 0 ? CCMP_RRTC_NONE : ccmp::rrtc_extend(m > 0 ? ns : 0, ms, c.ok[e], c.d[e], c.range, &a, &row);
  } else {
    const double last = comp && m > 0 ? st[(size_t)(m - 1) * 14 + lane] : 0.0;
    const double g = group_dist(last, tgt);
    if (m > 0) gap = g;
    outcome = use == 0 ? CCMP_RRTC_NONE : ccmp::rrtc_connect(m > 0 ? ns : 0, ms, c.ok[e], gap, &row);
  }
  const bool reached = c.mode == 0 && outcome == CCMP_RRTC_REACHED;
  const bool vertex = reached || row >= 0;
  const bool edge = vertex || (c.mode == 1 && outcome == CCMP_RRTC_CONNECT_JOINED);
  if (comp) c.row[(size_t)e * 14 + lane] = reached ? tgt : (row >= 0 && row < m) ? st[(size_t)row * 14 + lane] : 0.0;
  if (lane != 0) return;
  c.outcome[e] = outcome;
  c.row_index[e] = row;
  if (c.parent) c.parent[e] = edge && c.nearest ? c.nearest[e] : -1;
  if (c.made) c.made[e] = vertex ? 1 : 0;
  if (c.gap) c.gap[e] = gap;
}

__global__ __launch_bounds__(kThreads) void rrtc_commit_kernel(const GraphStore s, ccmp_rrtc_state *state, const RrtcCommit c)
{
  __shared__ int sa[kThreads], sb[kThreads];
  __shared__ int cnt[8];
  __shared__ double ld[kThreads / kWave];
  __shared__ int li[kThreads / kWave];
  const int t = threadIdx.x, W = c.W;
  const bool in = t < W;
  const int32_t oa = in ? c.outA[t] : CCMP_RRTC_NONE, ob = in ? c.outB[t] : CCMP_RRTC_NONE;
  const bool keepA = oa == CCMP_RRTC_ADVANCED || oa == CCMP_RRTC_REACHED;
  const bool keepB = keepA && ob == CCMP_RRTC_CONNECT_ADDED, joined = keepA && ob == CCMP_RRTC_CONNECT_JOINED;
  if (t < 8) cnt[t] = 0;
  sa[t] = keepA ? 1 : 0;
  sb[t] = keepB ? 1 : 0;
  __syncthreads();
  for (int off = 1; off < kThreads; off <<= 1) { // inclusive scans of both flags
    const int va = t >= off ? sa[t - off] : 0, vb = t >= off ? sb[t - off] : 0;
    __syncthreads();
    sa[t] += va;
    sb[t] += vb;
    __syncthreads();
  }
  const int nA = sa[kThreads - 1], nB = sb[kThreads - 1];
  const int posA = sa[t] - (keepA ? 1 : 0), posB = sb[t] - (keepB ? 1 : 0);
  const int32_t N = (int32_t)s.N, vA = N + posA, vB = N + nA + posB;
  if (in) {
    if (keepA)
      for (int k = 0; k < 14; k++) c.rows[(size_t)posA * 14 + k] = c.rowA[(size_t)t * 14 + k];
    if (keepB)
      for (int k = 0; k < 14; k++) c.rows[(size_t)(nA + posB) * 14 + k] = c.rowB[(size_t)t * 14 + k];
    c.uv[2 * t] = keepA ? c.parA[t] : -1;
    c.uv[2 * t + 1] = keepA ? vA : -1;
    c.uv[2 * (W + t)] = keepB || joined ? c.parB[t] : -1;
    c.uv[2 * (W + t) + 1] = keepB ? vB : joined ? vA : -1;
    if (c.useA[t]) atomicAdd(&cnt[0], 1);
    if (oa == CCMP_RRTC_TRAPPED) atomicAdd(&cnt[1], 1);
    if (oa == CCMP_RRTC_ADVANCED) atomicAdd(&cnt[2], 1);
    if (oa == CCMP_RRTC_REACHED) atomicAdd(&cnt[3], 1);
    if (oa == CCMP_RRTC_UNSETTLED) atomicAdd(&cnt[4], 1);
    if (joined) atomicAdd(&cnt[5], 1);
    if (keepA && ob == CCMP_RRTC_CONNECT_NOTHING) atomicAdd(&cnt[6], 1);
  }
  // the smallest (gap, sample) of the cycle, then one strict compare with the state's
  const double g = keepA ? c.gapB[t] : __builtin_nan("");
  double bd = g == g ? g : __builtin_inf();
  int bi = g == g ? t : kEmptyIdx;
  best_reduce(bd, bi, ld, li); // (its barrier also orders the counts)
  if (t == 0) {
    ld[0] = bd;
    li[0] = bi;
  }
  __syncthreads();
  if (li[0] == t && ld[0] < state->best_gap) {
    const int32_t u = c.idxB[t];
    const int32_t b_end = keepB ? vB : u;
    state->best_gap = ld[0];
    state->best_a = c.a_is_start ? vA : b_end;
    state->best_b = c.a_is_start ? b_end : vA;
  }
  if (t != 0) return;
  ccmp_rrtc_counters *k = &state->counters;
  k->samples += W;
  k->projected += cnt[0];
  k->trapped += cnt[1];
  k->advanced += cnt[2];
  k->reached += cnt[3];
  k->unsettled += cnt[4];
  k->connect_reached += cnt[5];
  k->connect_added += nB;
  k->connect_nothing += cnt[6];
  k->vertices += nA + nB;
  k->edges += nA + nB + cnt[5];
  state->next_index += (uint64_t)W;
  c.counts[0] = nA + nB;
  c.counts[1] = nA + nB + cnt[5];
  c.counts[2] = nA;
  c.counts[3] = nB;
}

}  // namespace

namespace ccmp_launch {

hipError_t rrtc_nearest(const GraphStore &s, const int32_t *roots, int n_roots, const double *queries, size_t Q, unsigned int part, unsigned int partitions,
                        double *ws_d, int32_t *ws_i, int32_t *idx, double *dist, hipStream_t st)
{
  hipLaunchKernelGGL(rrtc_nearest_kernel, dim3((unsigned int)Q, partitions), dim3(kThreads), 0, st, s, roots, n_roots, queries, part, (int)partitions, ws_d,
                     ws_i, idx, dist);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || partitions == 1) return e;
  hipLaunchKernelGGL(rrtc_nearest_merge_kernel, dim3((unsigned int)Q), dim3(kThreads), 0, st, (int)partitions, ws_d, ws_i, idx, dist);
  return hipGetLastError();
}

hipError_t rrtc_edges(const GraphStore &s, const int32_t *idx, const double *rows, const uint8_t *f0, const uint8_t *f1, const uint8_t *f2, size_t E,
                      double *from, double *to, uint8_t *use, hipStream_t st)
{
  hipLaunchKernelGGL(rrtc_edges_kernel, dim3((unsigned int)((E + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, s, idx, rows, f0, f1, f2, (unsigned int)E,
                     from, to, use);
  return hipGetLastError();
}

hipError_t rrtc_pick(const RrtcPick &c, hipStream_t st)
{
  const size_t per = kThreads / kGroup;
  hipLaunchKernelGGL(rrtc_pick_kernel, dim3((unsigned int)((c.E + per - 1) / per)), dim3(kThreads), 0, st, c);
  return hipGetLastError();
}

hipError_t rrtc_commit(const GraphStore &s, ccmp_rrtc_state *state, const RrtcCommit &c, hipStream_t st)
{
  hipLaunchKernelGGL(rrtc_commit_kernel, dim3(1), dim3(kThreads), 0, st, s, state, c);
  return hipGetLastError();
}

}  // namespace ccmp_launch
