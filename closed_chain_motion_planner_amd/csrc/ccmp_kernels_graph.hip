// ccmp_kernels_graph.hip — the roadmap graph on the device: growTree's tail (ccmp_roadmap_commit), explicit edges, the component labels
// and closestFromGoal's vertex scan.  The decisions and their arithmetic are csrc/ccmp_graph.h, compiled here and, for the *_ref forms,
// in ccmp_roadmap.cpp: one text, the same bits.
//
// Commit, four launches on the call's stream:
//   graph_slot_kernel     the slot is the lane (Q k of them): kind, root flag, L[nbr], the edge weight, and for a failed slot with a last
//                         state the FK of that state, its pose and the two distances to the goal — the expensive part.
//   graph_query_kernel    the query is the lane: the rule's loop on the slots' flags -> masks, counts, the state.
//   graph_scan_kernel     ONE block: exclusive scan of the vertex and edge counts (a lane sums a contiguous run, the 256 partial sums
//                         are scanned in LDS, the lane walks its run again), the totals and the new edge floor.
//   graph_scatter_kernel  the slot is the lane again: rows, edges, labels (label[i] = i), new_index, mid_index.
// Explicit edges: graph_edge_flag_kernel -> graph_scan_kernel -> graph_edge_scatter_kernel (the weights).
//
// Components, two launches:
//   graph_hook_kernel     ONE block over the call's new edges.  A round chases both endpoints to their roots and does atomicMin of the
//                         smaller root into the larger root's label; a block barrier; repeat until no edge joins two roots.  label[x] <= x
//                         always, so a chase strictly descends; labels are compressed at entry and only roots are hooked, so a chain is
//                         at most (new edges) hops and every round that finds work removes at least one root: at most E_new + 1 rounds.
//                         Both loops carry those bounds.  The smallest index of a component ends as its only root whatever the arrival
//                         order of the atomics: the labels are a function of the edge set.
//   graph_compress_kernel multi-block, a launch of its own (stream order is the only ordering between blocks): label[i] = root(label[i]).
//                         A block may read a label another block has already shortened: both values lead to the same root.
// No grid barrier, no spin, no hand-off between blocks inside a launch.
//
// Closest: graph_closest_kernel, knn_pose_few_kernel's layout with lists of one — blocks over (partition, from), a lane takes the
// vertices t, t + 256, ... of the partition whose label is from's, the 256 bests are merged in LDS; several partitions leave theirs in the
// workspace and graph_closest_merge_kernel merges them.  (distance, index) is a total order: no launch shape changes the answer.
//
// Shortest paths (ccmp_path.h), three launches, one pair (src[f], dst[f]) per f < F, per-pair arrays d / hops / pred / stamp [F][N]:
//   graph_path_init_kernel     multi-block: +inf, INT_MAX, -1 and stamp -1 everywhere, the source's entries 0.
//   graph_path_sssp_kernel     ONE block per pair, up to 1024 lanes striding over the edge list, three phases separated by block barriers
//                              only.  Relaxation rounds: every edge in both directions, atomicMin on the distance's bits (distances are
//                              >= +0.0 and never NaN: the order of the bits is theirs); stamp[v] = the last round that lowered d[v], and
//                              round r skips an edge when neither endpoint was lowered in round r - 1 or later.  A vertex's last move in
//                              round r keeps stamp == r through the whole of round r + 1, where each of its edges is relaxed with the
//                              final value: a round without a move ends the phase at the fixed point, after at most N + 1 rounds (after
//                              round r every vertex whose cheapest path has <= r edges is final).  Hop rounds likewise: round r gives level
//                              r over tight edges from level r - 1.  Then one pass: atomicMin of u into pred[v] over the tree candidates
//                              (as unsigned: -1 is "none", above every vertex).  Both round loops carry the bound N + 1.  d, hops and stamp
//                              are read with agent-scope atomic loads: what an atomic left in L2 is the truth, never an L1 line.
//   graph_path_extract_kernel  one block per pair: lane 0 walks pred from dst (hops[dst] + 1 steps, the loop's bound) into path[f] front to
//                              back, then the lanes gather the joint and pose rows.
// The answer is a function of the edge set: no arrival order of the atomics, no block size changes a bit.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_graph.h"
#include "ccmp_launch.h"
#include "ccmp_path.h"

namespace {

using ccmp_launch::GraphCommit;
using ccmp_launch::GraphPath;
using ccmp_launch::GraphStore;
using ccmp_launch::GraphWork;
constexpr int kThreads = ccmp_launch::kGraphThreads;
constexpr int kPathThreads = ccmp_launch::kPathThreads;
constexpr int kEmptyIdx = 0x7fffffff; // no candidate yet: (+inf, kEmptyIdx), behind every vertex

__global__ __launch_bounds__(kThreads) void graph_iota_kernel(int32_t *__restrict__ labels, unsigned long long first, unsigned long long n)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) labels[first + i] = (int32_t)(first + i);
}

__global__ __launch_bounds__(kThreads) void graph_slot_kernel(const ccmp_consts K, int has_K, const GraphStore s, const GraphWork w, const GraphCommit c,
                                                              const ccmp::graph_roots R)
{
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= c.Q * (unsigned long long)c.k) return;
  const unsigned long long q = e / (unsigned long long)c.k;
  int32_t label = 0;
  double weight = 0.0, mid[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  const uint32_t f = ccmp::graph_slot_eval(K, has_K != 0, s.joints, s.poses, s.labels, (uint32_t)s.N, R, c.nbr_idx[e], c.edge_ok[e], c.n_states[e],
                                           c.max_states, c.states ? c.states + e * (unsigned long long)c.max_states * 14 : nullptr, c.new_joints + q * 14,
                                           c.goal, &label, &weight, mid);
  w.flags[e] = f;
  w.label[e] = label;
  w.weight[e] = weight;
#pragma unroll
  for (int i = 0; i < 8; i++) w.mid_pose[e * 8 + i] = mid[i];
}

__global__ __launch_bounds__(kThreads) void graph_query_kernel(const GraphWork w, const GraphCommit c)
{
  const unsigned long long q = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (q >= c.Q) return;
  const ccmp::graph_decision d = ccmp::graph_decide(w.flags + q * c.k, w.label + q * c.k, c.k, c.vertex_ok ? c.vertex_ok[q] != 0 : 1, c.keep_isolated);
  const int mids = ccmp::graph_popcount(d.mid), reached = ccmp::graph_popcount(d.reached);
  w.masks[q] = d.reached | d.mid << 16;
  w.cnt_v[q] = d.keep + mids;
  w.cnt_e[q] = reached + mids;
  w.hi[q] = mids ? d.keep + mids : reached ? 1 : 0; // 1 + the offset, among q's new vertices, of the last one that has an edge
  c.grow_state[q] = d.state;
}

// n items; cnt_v == nullptr: no vertices.  totals = {sum of cnt_v, sum of cnt_e, the edge floor}: the larger of floor_in and, over the
// items with hi > 0, of hi (hi_is_offset == 0) or N + base_v + hi.
__global__ __launch_bounds__(kThreads) void graph_scan_kernel(const GraphWork w, unsigned long long n, unsigned long long N, int hi_is_offset, int floor_in)
{
  __shared__ int sv[kThreads], se[kThreads], sf[kThreads];
  const int t = threadIdx.x;
  const unsigned long long per = (n + kThreads - 1) / kThreads, lo = per * t < n ? per * t : n, hi = lo + per < n ? lo + per : n;
  int av = 0, ae = 0;
  for (unsigned long long i = lo; i < hi; i++) { av += w.cnt_v ? w.cnt_v[i] : 0; ae += w.cnt_e[i]; }
  sv[t] = av;
  se[t] = ae;
  __syncthreads();
  for (int stride = 1; stride < kThreads; stride <<= 1) { // inclusive scan of the partial sums
    const int xv = t >= stride ? sv[t - stride] : 0, xe = t >= stride ? se[t - stride] : 0;
    __syncthreads();
    sv[t] += xv;
    se[t] += xe;
    __syncthreads();
  }
  int bv = sv[t] - av, be = se[t] - ae, fl = floor_in;
  for (unsigned long long i = lo; i < hi; i++) {
    w.base_v[i] = bv;
    w.base_e[i] = be;
    const int h = w.hi[i];
    if (h > 0) { const int cand = hi_is_offset ? (int)N + bv + h : h; fl = cand > fl ? cand : fl; }
    bv += w.cnt_v ? w.cnt_v[i] : 0;
    be += w.cnt_e[i];
  }
  sf[t] = fl;
  __syncthreads();
  for (int stride = kThreads / 2; stride >= 1; stride >>= 1) {
    if (t < stride) sf[t] = sf[t + stride] > sf[t] ? sf[t + stride] : sf[t];
    __syncthreads();
  }
  if (t == 0) { w.totals[0] = sv[kThreads - 1]; w.totals[1] = se[kThreads - 1]; w.totals[2] = sf[0]; w.totals[3] = 0; }
}

__global__ __launch_bounds__(kThreads) void graph_scatter_kernel(const GraphStore s, const GraphWork w, const GraphCommit c)
{
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= c.Q * (unsigned long long)c.k) return;
  const unsigned long long q = e / (unsigned long long)c.k;
  const int r = (int)(e % (unsigned long long)c.k);
  const uint32_t m = w.masks[q], reached = m & 0xffffu, mid = m >> 16, below = (1u << r) - 1u;
  const int keep = w.cnt_v[q] - ccmp::graph_popcount(mid);
  // rows N .. N + totals[0] - 1 and edges E .. E + totals[1] - 1: inside the worst case the host reserved
  const size_t vb = s.N + (size_t)w.base_v[q], eb = s.E + (size_t)w.base_e[q];
  if (r == 0) {
    c.new_index[q] = keep ? (int32_t)vb : -1;
    if (keep) {
#pragma unroll
      for (int i = 0; i < 14; i++) s.joints[vb * 14 + i] = c.new_joints[q * 14 + i];
#pragma unroll
      for (int i = 0; i < 8; i++) s.poses[vb * 8 + i] = i == 7 ? 0.0 : c.new_poses[q * 8 + i];
      s.labels[vb] = (int32_t)vb;
    }
  }
  const int32_t nbr = c.nbr_idx[e];
  int32_t mid_index = -1;
  if (reached >> r & 1u) {
    const size_t j = eb + (size_t)ccmp::graph_popcount(reached & below);
    s.uv[2 * j] = nbr;
    s.uv[2 * j + 1] = (int32_t)vb;
    s.w[j] = w.weight[e];
  } else if (mid >> r & 1u) {
    const int ord = ccmp::graph_popcount(mid & below);
    const size_t vi = vb + (size_t)keep + (size_t)ord, j = eb + (size_t)ccmp::graph_popcount(reached) + (size_t)ord;
    const double *last = c.states + (e * (unsigned long long)c.max_states + (unsigned long long)(c.n_states[e] - 1)) * 14; // a mid-stone: states given, 1 < n_states <= max_states
#pragma unroll
    for (int i = 0; i < 14; i++) s.joints[vi * 14 + i] = last[i];
#pragma unroll
    for (int i = 0; i < 8; i++) s.poses[vi * 8 + i] = w.mid_pose[e * 8 + i];
    s.labels[vi] = (int32_t)vi;
    s.uv[2 * j] = nbr;
    s.uv[2 * j + 1] = (int32_t)vi;
    s.w[j] = w.weight[e];
    mid_index = (int32_t)vi;
  }
  c.mid_index[e] = mid_index;
}

__global__ __launch_bounds__(kThreads) void graph_edge_flag_kernel(const GraphWork w, const int32_t *__restrict__ uv, unsigned long long n, unsigned int N)
{
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n) return;
  const int32_t u = uv[2 * e], v = uv[2 * e + 1];
  const bool valid = u >= 0 && v >= 0 && (unsigned int)u < N && (unsigned int)v < N && u != v;
  w.cnt_e[e] = valid;
  w.hi[e] = valid ? (u > v ? u : v) + 1 : 0;
}

__global__ __launch_bounds__(kThreads) void graph_edge_scatter_kernel(const GraphStore s, const GraphWork w, const int32_t *__restrict__ uv, unsigned long long n)
{
  const unsigned long long e = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (e >= n || !w.cnt_e[e]) return;
  const int32_t u = uv[2 * e], v = uv[2 * e + 1]; // both inside [0, N): the flag kernel's test
  const size_t j = s.E + (size_t)w.base_e[e];      // < E + n: reserved
  s.uv[2 * j] = u;
  s.uv[2 * j + 1] = v;
  s.w[j] = ccmp::graph_joint_dist(s.joints + (size_t)u * 14, s.joints + (size_t)v * 14);
}

// the root of x: label[r] == r; at most `hops` steps (a chain is never longer: see the head of the file)
__device__ __forceinline__ int32_t graph_root(const volatile int32_t *labels, int32_t x, unsigned int hops)
{
  for (unsigned int h = 0; h < hops; h++) {
    const int32_t l = labels[x];
    if (l == x) break;
    x = l; // l < x: descends, and l >= 0 stays inside the labels
  }
  return x;
}

__global__ __launch_bounds__(kThreads) void graph_hook_kernel(const GraphStore s, const int32_t *__restrict__ totals, unsigned int max_new)
{
  __shared__ int changed;
  const int t = threadIdx.x;
  unsigned int n = (unsigned int)totals[1];
  if (n > max_new) n = max_new;
  const int32_t *uv = s.uv + 2 * s.E;
  for (unsigned int round = 0; round <= n; round++) {
    if (t == 0) changed = 0;
    __syncthreads();
    for (unsigned int e = t; e < n; e += kThreads) {
      const int32_t ru = graph_root(s.labels, uv[2 * e], n + 2), rv = graph_root(s.labels, uv[2 * e + 1], n + 2);
      if (ru != rv) {
        atomicMin(&s.labels[ru > rv ? ru : rv], ru > rv ? rv : ru);
        changed = 1;
      }
    }
    __syncthreads(); // the round's hooks are visible to the block (one block: workgroup scope is all it takes)
    const int more = changed;
    __syncthreads();
    if (!more) break;
  }
}

// the grid covers n_max labels (the worst case the host reserved); the labels that exist are the N at entry and the totals[0] new ones
__global__ __launch_bounds__(kThreads) void graph_compress_kernel(int32_t *labels, unsigned long long N, const int32_t *__restrict__ totals,
                                                                  unsigned long long n_max, unsigned int max_new)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  unsigned long long n = N + (unsigned long long)totals[0];
  if (n > n_max) n = n_max;
  if (i >= n) return;
  const int32_t r = graph_root(labels, (int32_t)i, max_new + 2);
  if (r != (int32_t)i) labels[i] = r; // a root keeps label[r] == r: never written here
}

// the 256 bests in LDS -> lane 0's
__device__ __forceinline__ void best_merge(double *ld, int *li, int t)
{
  for (int stride = kThreads / 2; stride >= 1; stride >>= 1) {
    __syncthreads();
    if (t < stride && ccmp::graph_closer(ld[t + stride], li[t + stride], ld[t], li[t])) { ld[t] = ld[t + stride]; li[t] = li[t + stride]; }
  }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void graph_closest_kernel(const GraphStore s, const int32_t *__restrict__ from_idx, const double *__restrict__ target,
                                                                 unsigned int part, int P, double *ws_d, int32_t *ws_i, int32_t *idx, double *dist,
                                                                 double *from_dist)
{
  __shared__ double ld[kThreads];
  __shared__ int li[kThreads];
  const int t = threadIdx.x, p = blockIdx.x;
  const size_t f = blockIdx.y;
  const unsigned int N = (unsigned int)s.N;
  const int32_t from = from_idx[f];
  const bool known = from >= 0 && (unsigned int)from < N; // the same for every lane of the block
  double x[8];
#pragma unroll
  for (int c = 0; c < 7; c++) x[c] = target[c];
  x[7] = 0.0;
  double bd = __builtin_inf();
  int bi = kEmptyIdx;
  if (known) {
    const int32_t lab = s.labels[from];
    const unsigned int lo = (unsigned int)p * part, hi = lo + part < N ? lo + part : N;
    for (unsigned int j = lo + t; j < hi; j += kThreads) {
      if (s.labels[j] != lab) continue;
      const double d = ccmp_pose_dist(s.poses + (size_t)j * 8, x);
      if (ccmp::graph_closer(d, (int)j, bd, bi)) { bd = d; bi = (int)j; } // a NaN distance is below nothing
    }
  }
  ld[t] = bd;
  li[t] = bi;
  best_merge(ld, li, t);
  if (t != 0) return;
  if (P == 1) {
    idx[f] = li[0] == kEmptyIdx ? -1 : li[0];
    dist[f] = ld[0];
  } else {
    ws_d[f * (size_t)P + p] = ld[0];
    ws_i[f * (size_t)P + p] = li[0];
  }
  if (p == 0) from_dist[f] = known ? ccmp_pose_dist(s.poses + (size_t)from * 8, x) : __builtin_nan("");
}

__global__ __launch_bounds__(kThreads) void graph_closest_merge_kernel(int P, const double *__restrict__ ws_d, const int32_t *__restrict__ ws_i, int32_t *idx,
                                                                       double *dist)
{
  __shared__ double ld[kThreads];
  __shared__ int li[kThreads];
  const int t = threadIdx.x;
  const size_t f = blockIdx.x;
  ld[t] = t < P ? ws_d[f * (size_t)P + t] : __builtin_inf();
  li[t] = t < P ? ws_i[f * (size_t)P + t] : kEmptyIdx;
  best_merge(ld, li, t);
  if (t == 0) {
    idx[f] = li[0] == kEmptyIdx ? -1 : li[0];
    dist[f] = ld[0];
  }
}

// ---- shortest paths (ccmp_path.h) ---------------------------------------------------------------------------------------------------
using u64 = unsigned long long;
__device__ __forceinline__ u64 path_ld64(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t path_ld32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the grid: (blocks over the N vertices, F)
__global__ __launch_bounds__(kThreads) void graph_path_init_kernel(const GraphPath p, unsigned long long N)
{
  const unsigned long long i = (unsigned long long)blockIdx.x * kThreads + threadIdx.x, f = blockIdx.y;
  if (i >= N) return;
  const int32_t s = p.src[f];
  const bool source = s >= 0 && (unsigned long long)s == i; // (i < N: a source outside the store matches no lane, nothing is reached)
  const unsigned long long o = f * N + i;
  p.d[o] = source ? 0ull : ccmp::path_bits(__builtin_inf());
  p.hops[o] = source ? 0 : ccmp::kPathNoHops;
  p.pred[o] = -1;
  p.stamp[o] = source ? 0 : -1;
}

// one direction of one edge in relaxation round r; true: d[v] went down
__device__ __forceinline__ bool path_relax(u64 *d, int32_t *stamp, int32_t u, int32_t v, double w, int32_t r)
{
  double c;
  if (!ccmp::path_candidate(ccmp::path_from_bits(path_ld64(d + u)), w, &c)) return false;
  const u64 cb = ccmp::path_bits(c);
  if (cb >= path_ld64(d + v)) return false;
  if (atomicMin(d + v, cb) <= cb) return false; // another lane was there first with no more
  __hip_atomic_store(stamp + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

__global__ __launch_bounds__(kPathThreads) void graph_path_sssp_kernel(const GraphStore s, const GraphPath p)
{
  __shared__ int changed;
  const unsigned int t = threadIdx.x, nt = blockDim.x, N = (unsigned int)s.N, E = (unsigned int)s.E;
  const size_t f = blockIdx.x;
  u64 *d = p.d + f * N;
  int32_t *hops = p.hops + f * N, *pred = p.pred + f * N, *stamp = p.stamp + f * N;
  const int32_t max_rounds = N < 0x7ffffffeu ? (int32_t)N + 1 : 0x7ffffffe;
  int32_t relax_rounds = 0, hop_rounds = 0;
  for (int32_t r = 1; r <= max_rounds; r++) {
    if (t == 0) changed = 0;
    __syncthreads();
    for (unsigned int e = t; e < E; e += nt) {
      const int32_t u = s.uv[2 * e], v = s.uv[2 * e + 1];
      if ((unsigned int)u >= N || (unsigned int)v >= N) continue; // (the store's edges are inside it; this keeps every access in bounds)
      if (path_ld32(stamp + u) < r - 1 && path_ld32(stamp + v) < r - 1) continue;
      const double w = s.w[e];
      const bool a = path_relax(d, stamp, u, v, w, r), b = path_relax(d, stamp, v, u, w, r);
      if (a || b) changed = 1;
    }
    __syncthreads(); // the round's atomics are done and visible to the block (one block: workgroup scope is all it takes)
    const int more = changed;
    __syncthreads();
    relax_rounds = r;
    if (!more) break;
  }
  for (int32_t r = 1; r <= max_rounds; r++) {
    if (t == 0) changed = 0;
    __syncthreads();
    for (unsigned int e = t; e < E; e += nt) {
      const int32_t u = s.uv[2 * e], v = s.uv[2 * e + 1];
      if ((unsigned int)u >= N || (unsigned int)v >= N) continue;
      const int32_t hu = path_ld32(hops + u), hv = path_ld32(hops + v);
      if (hu != r - 1 && hv != r - 1) continue;
      const double w = s.w[e], du = ccmp::path_from_bits(path_ld64(d + u)), dv = ccmp::path_from_bits(path_ld64(d + v));
      if (hu == r - 1 && hv > r && ccmp::path_tight(du, w, dv)) { atomicMin(hops + v, r); changed = 1; }
      if (hv == r - 1 && hu > r && ccmp::path_tight(dv, w, du)) { atomicMin(hops + u, r); changed = 1; }
    }
    __syncthreads();
    const int more = changed;
    __syncthreads();
    hop_rounds = r;
    if (!more) break;
  }
  for (unsigned int e = t; e < E; e += nt) {
    const int32_t u = s.uv[2 * e], v = s.uv[2 * e + 1];
    if ((unsigned int)u >= N || (unsigned int)v >= N) continue;
    const int32_t hu = path_ld32(hops + u), hv = path_ld32(hops + v);
    const double w = s.w[e], du = ccmp::path_from_bits(path_ld64(d + u)), dv = ccmp::path_from_bits(path_ld64(d + v));
    if (ccmp::path_parent(du, hu, w, dv, hv)) atomicMin((unsigned int *)pred + v, (unsigned int)u);
    if (ccmp::path_parent(dv, hv, w, du, hu)) atomicMin((unsigned int *)pred + u, (unsigned int)v);
  }
  if (t == 0) { p.rounds[2 * f] = relax_rounds; p.rounds[2 * f + 1] = hop_rounds; }
}

// a launch of its own behind the sssp launch: plain loads see what its atomics left
__global__ __launch_bounds__(kThreads) void graph_path_extract_kernel(const GraphStore s, const GraphPath p)
{
  __shared__ int s_len;
  const int t = threadIdx.x;
  const size_t f = blockIdx.x;
  const unsigned int N = (unsigned int)s.N;
  int32_t *path = p.path + f * (size_t)p.max_len;
  if (t == 0) {
    const int32_t src = p.src[f], dst = p.dst[f];
    int32_t len = 0;
    double cost = __builtin_nan("");
    if (src >= 0 && dst >= 0 && (unsigned int)src < N && (unsigned int)dst < N) {
      const int32_t h = p.hops[f * N + dst];
      cost = ccmp::path_from_bits(p.d[f * N + dst]);
      len = h == ccmp::kPathNoHops ? 0 : h + 1;
      if (len <= p.max_len) {
        int32_t v = dst;
        for (int32_t i = len - 1; i >= 0 && (unsigned int)v < N; i--) { // hops[v] falls by one per step: exactly len steps
          path[i] = v;
          v = p.pred[f * N + v];
        }
      }
    }
    p.cost[f] = cost;
    p.path_len[f] = len;
    s_len = len <= p.max_len ? len : 0;
  }
  __syncthreads(); // lane 0's path entries are visible to the block
  const int len = s_len;
  if (p.path_joints)
    for (int i = t; i < len * 14; i += kThreads) {
      const unsigned int v = (unsigned int)path[i / 14];
      if (v < N) p.path_joints[(f * (size_t)p.max_len + (size_t)(i / 14)) * 14 + (size_t)(i % 14)] = s.joints[(size_t)v * 14 + (size_t)(i % 14)];
    }
  if (p.path_poses)
    for (int i = t; i < len * 8; i += kThreads) {
      const unsigned int v = (unsigned int)path[i / 8];
      if (v < N) p.path_poses[(f * (size_t)p.max_len + (size_t)(i / 8)) * 8 + (size_t)(i % 8)] = s.poses[(size_t)v * 8 + (size_t)(i % 8)];
    }
}

unsigned int blocks_of(size_t n) { return (unsigned int)((n + kThreads - 1) / kThreads); }

}  // namespace

namespace ccmp_launch {

hipError_t graph_iota(int32_t *labels, size_t first, size_t n, hipStream_t st)
{
  hipLaunchKernelGGL(graph_iota_kernel, dim3(blocks_of(n)), dim3(kThreads), 0, st, labels, (unsigned long long)first, (unsigned long long)n);
  return hipGetLastError();
}

hipError_t graph_commit(const GraphStore &s, const GraphWork &w, const GraphCommit &c, hipStream_t st)
{
  const size_t S = c.Q * (size_t)c.k;
  ccmp_consts K{};
  if (c.K) K = *c.K;
  hipLaunchKernelGGL(graph_slot_kernel, dim3(blocks_of(S)), dim3(kThreads), 0, st, K, c.K ? 1 : 0, s, w, c, *c.roots);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(graph_query_kernel, dim3(blocks_of(c.Q)), dim3(kThreads), 0, st, w, c);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(graph_scan_kernel, dim3(1), dim3(kThreads), 0, st, w, (unsigned long long)c.Q, (unsigned long long)s.N, 1, (int)s.floor);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(graph_scatter_kernel, dim3(blocks_of(S)), dim3(kThreads), 0, st, s, w, c);
  return hipGetLastError();
}

hipError_t graph_add_edges(const GraphStore &s, const GraphWork &w, const int32_t *uv, size_t E, hipStream_t st)
{
  hipLaunchKernelGGL(graph_edge_flag_kernel, dim3(blocks_of(E)), dim3(kThreads), 0, st, w, uv, (unsigned long long)E, (unsigned int)s.N);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  GraphWork we = w;
  we.cnt_v = nullptr;
  hipLaunchKernelGGL(graph_scan_kernel, dim3(1), dim3(kThreads), 0, st, we, (unsigned long long)E, (unsigned long long)s.N, 0, (int)s.floor);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(graph_edge_scatter_kernel, dim3(blocks_of(E)), dim3(kThreads), 0, st, s, w, uv, (unsigned long long)E);
  return hipGetLastError();
}

hipError_t graph_components(const GraphStore &s, const int32_t *totals, size_t n_after, size_t max_new, hipStream_t st)
{
  hipLaunchKernelGGL(graph_hook_kernel, dim3(1), dim3(kThreads), 0, st, s, totals, (unsigned int)max_new);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(graph_compress_kernel, dim3(blocks_of(n_after)), dim3(kThreads), 0, st, s.labels, (unsigned long long)s.N, totals,
                     (unsigned long long)n_after, (unsigned int)max_new);
  return hipGetLastError();
}

hipError_t graph_closest(const GraphStore &s, const int32_t *from_idx, size_t F, const double *target, unsigned int part, unsigned int partitions,
                         double *ws_d, int32_t *ws_i, int32_t *idx, double *dist, double *from_dist, hipStream_t st)
{
  hipLaunchKernelGGL(graph_closest_kernel, dim3(partitions, (unsigned int)F), dim3(kThreads), 0, st, s, from_idx, target, part, (int)partitions, ws_d, ws_i,
                     idx, dist, from_dist);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess || partitions == 1) return e;
  hipLaunchKernelGGL(graph_closest_merge_kernel, dim3((unsigned int)F), dim3(kThreads), 0, st, (int)partitions, ws_d, ws_i, idx, dist);
  return hipGetLastError();
}

hipError_t graph_paths(const GraphStore &s, const GraphPath &p, hipStream_t st)
{
  hipError_t e = hipSuccess;
  if (s.N > 0) {
    hipLaunchKernelGGL(graph_path_init_kernel, dim3(blocks_of(s.N), (unsigned int)p.F), dim3(kThreads), 0, st, p, (unsigned long long)s.N);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    size_t lanes = (s.E + 63) / 64 * 64; // a lane per edge up to the block's 1024
    lanes = lanes < 64 ? 64 : lanes > (size_t)kPathThreads ? (size_t)kPathThreads : lanes;
    hipLaunchKernelGGL(graph_path_sssp_kernel, dim3((unsigned int)p.F), dim3((unsigned int)lanes), 0, st, s, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(graph_path_extract_kernel, dim3((unsigned int)p.F), dim3(kThreads), 0, st, s, p);
  return hipGetLastError();
}

}  // namespace ccmp_launch
