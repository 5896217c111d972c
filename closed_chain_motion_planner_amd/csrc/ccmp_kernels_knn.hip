// ccmp_kernels_knn.hip — the connection step: brute-force FP64 k nearest neighbours over the joint vectors, and the gather that
// turns its result into the edges of a traversal call (ccmp_knn_batch / ccmp_connect_batch).
//
// The reference chooses the pairs it tries with connectionStrategy_(m), a KStrategy of DEFAULT_NEAREST_NEIGHBORS = 5 over tree_
// (src/planner/stefanBiPRM.cpp:292,390,457); the joint part of its metric is RealVectorStateSpace::distance over the 14 joints —
// oracle/ccmp_oracle.c: orc_distance, the serial chain dist = fma(diff_i, diff_i, dist), i = 0..13, then the correctly rounded
// square root (ccmp_detmath.h: ccmp_sqrt).  Ranking: ascending by (distance AFTER the square root, node index).  Two squared
// sums one ulp apart can round to the same distance, and then the lower index wins: the key is the rounded distance.
//
// Every list below — a thread's, a block's, a partition's — is "the KC smallest keys of the nodes it has seen", kept sorted.
// The key is a total order on the nodes (indices are unique), so the KC smallest of a union are the KC smallest of the parts'
// lists whichever way the parts were cut and merged: the result is a pure function of the inputs, the same for every tile size,
// partition count and grid.  No atomics.  A thread scans its nodes in increasing index, so a node enters its list only when its
// distance is STRICTLY below the list's worst; d2 < (worst distance)^2, rounded up, is a necessary condition for that and is all
// that most pairs cost beyond the 14 subtractions and 14 FMAs: the square root runs a handful of times per list.
//
//   knn_many_kernel   Q > kKnnFewMax.  One query per thread (its 14 joints and its list in registers), 256 queries per block; the
//                     block's partition of the nodes goes through LDS in tiles of 256 nodes (28 KB), every lane reading the same
//                     row at a time (a broadcast: no bank conflicts, 7 ds_read_b128 against 28 FP64 operations per node).
//   knn_few_kernel    Q <= kKnnFewMax (the planner inserting one milestone).  One block per (partition, query): thread t takes
//                     the nodes t, t + 256, ... of the partition straight from memory, then the 256 lists are merged pairwise in
//                     LDS (eight rounds), so a single query over 10^5..10^6 nodes is spread over the whole chip.
//   knn_merge_kernel  one block per query: the partitions' lists (context-owned workspace) -> the k best.  Skipped when there
//                     is one partition (the scan kernels then write the result themselves).
//   connect_gather_kernel / connect_fix_kernel   edge e = q * k + r: from = nodes[nbr_idx[q][r]], to = queries[q]; an empty
//                     slot gets from = to (a traversal that ends before its first Newton round) and is overwritten afterwards.
//
// The same two layouts on the reference's own tree metric, the SE3 distance between object poses (ccmp_pose.h; the roadmap store of
// ccmp_roadmap.cpp keeps one 64-byte pose row per node):
//   knn_pose_many_kernel  one query per thread, LDS tiles of 512 poses (32 KB).  distance = |dp| + rot with rot >= 0, so
//                         |dp|^2 < the list's bound is still a necessary condition for entry: a node costs two ds_read_b128 (x y | z qx),
//                         three subtractions and three FMAs; only a candidate reads the other half of its row and pays for the square
//                         root, the quaternion dot product and the atan.
//   knn_pose_few_kernel   one block per (partition, query), four 16-byte global loads per node.
//   knn_merge_kernel      unchanged: its lists do not depend on the metric.
//   pose_from_joints_kernel / pose_store_kernel / joints_fill_nan_kernel   what an append to the store runs (derived poses; given
//                         poses with the pad zeroed; the NaN joint rows of a pose-only vertex).
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_launch.h"
#include "ccmp_pose.h"

namespace {

constexpr int kThreads = ccmp_launch::kKnnThreads;
constexpr int kTile = ccmp_launch::kKnnTile;
constexpr int kRows = 2; // knn_many_kernel: tile rows per step of its node loop
static_assert(kTile % kRows == 0, "knn_many_kernel reads its tile kRows rows at a time");
constexpr int kEmptyIdx = 0x7fffffff; // an empty slot's key is (+inf, kEmptyIdx): behind every node, also one at distance +inf

__device__ __forceinline__ bool key_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// a thread's list: KC (distance, index) pairs in registers, sorted; every index below is a compile-time constant after unrolling
template <int KC>
struct List {
  double d[KC];
  int i[KC];
  double bound; // (worst distance)^2 rounded up: a node whose squared sum is not below it cannot improve the list
  __device__ __forceinline__ void clear()
  {
#pragma unroll
    for (int s = 0; s < KC; s++) { d[s] = __builtin_inf(); i[s] = kEmptyIdx; }
    bound = __builtin_inf();
  }
  __device__ __forceinline__ void insert(double dist, int idx) // (dist, idx) is known to be below the worst entry
  {
#pragma unroll
    for (int s = KC - 1; s >= 1; s--) { // from the back: entry s still holds its old value when it is looked at
      if (key_less(dist, idx, d[s - 1], i[s - 1])) { d[s] = d[s - 1]; i[s] = i[s - 1]; }
      else if (key_less(dist, idx, d[s], i[s])) { d[s] = dist; i[s] = idx; }
    }
    if (key_less(dist, idx, d[0], i[0])) { d[0] = dist; i[0] = idx; }
    // >= w^2 exactly (two roundings of 2^-53 against the factor; 2^-1000 covers a product that rounds in the subnormal range):
    // the square root is monotone, so sqrt(x) >= w for every x >= bound
    const double w = d[KC - 1];
    bound = (w * w) * (1.0 + 0x1p-51) + 0x1p-1000;
  }
  // one node, scanned in increasing index: d2 = its squared sum
  __device__ __forceinline__ void offer(double d2, int idx)
  {
    if (d2 < bound || d2 == __builtin_inf()) { // (NaN fails both: a non-finite coordinate on either side is never a neighbour)
      const double dist = ccmp_sqrt(d2);
      if (key_less(dist, idx, d[KC - 1], i[KC - 1])) insert(dist, idx);
    }
  }
};

// where a block's or a thread's finished list goes: the caller's arrays (one partition) or the workspace (several)
struct KnnOut {
  int32_t *nbr_idx;   // [Q][k]
  double *nbr_dist;   // [Q][k], nullable
  double *ws_d;       // [Q][P][KC]
  int32_t *ws_i;      // [Q][P][KC]
  int k, P;
};

template <int KC>
__device__ __forceinline__ void emit(const KnnOut &o, size_t q, int p, const double (&d)[KC], const int (&i)[KC])
{
  if (o.P == 1) {
#pragma unroll
    for (int s = 0; s < KC; s++)
      if (s < o.k) {
        o.nbr_idx[q * (size_t)o.k + s] = i[s] == kEmptyIdx ? -1 : i[s];
        if (o.nbr_dist) o.nbr_dist[q * (size_t)o.k + s] = d[s];
      }
  } else {
    const size_t base = (q * (size_t)o.P + (size_t)p) * KC;
#pragma unroll
    for (int s = 0; s < KC; s++) { o.ws_d[base + s] = d[s]; o.ws_i[base + s] = i[s]; }
  }
}

// which nodes a query may take: j < lim and j != excl (ccmp.h: CCMP_KNN_*)
__device__ __forceinline__ void eligibility(int mode, unsigned long long self, unsigned int N, unsigned int &lim, unsigned int &excl)
{
  lim = N;
  excl = 0xffffffffu;
  if (mode == 1 && self < N) excl = (unsigned int)self;
  if (mode == 2 && self < N) lim = (unsigned int)self;
}

// the lists of NT threads, in LDS as ld[t * KC + s] / li[t * KC + s], merged pairwise; thread 0 ends with the KC best in od / oi
template <int KC, int NT>
__device__ __forceinline__ void block_merge(double *ld, int *li, int t, double (&od)[KC], int (&oi)[KC])
{
  for (int stride = NT / 2; stride >= 1; stride >>= 1) {
    __syncthreads();
    if (t < stride) {
      const double *da = ld + t * KC, *db = ld + (t + stride) * KC;
      const int *ia = li + t * KC, *ib = li + (t + stride) * KC;
      int a = 0, b = 0; // a + b = s <= KC - 1 at every read: in bounds
#pragma unroll
      for (int s = 0; s < KC; s++) {
        const double xa = da[a], xb = db[b];
        const int ja = ia[a], jb = ib[b];
        const bool take_a = !key_less(xb, jb, xa, ja);
        od[s] = take_a ? xa : xb;
        oi[s] = take_a ? ja : jb;
        a += take_a;
        b += !take_a;
      }
    }
    __syncthreads();
    if (t < stride) {
#pragma unroll
      for (int s = 0; s < KC; s++) { ld[t * KC + s] = od[s]; li[t * KC + s] = oi[s]; }
    }
  }
}

template <int KC>
__global__ __launch_bounds__(kThreads) void knn_many_kernel(const double *__restrict__ nodes, unsigned int N, const double *__restrict__ queries,
                                                            unsigned long long Q, int mode, unsigned long long self_base, unsigned int part, KnnOut o)
{
  __shared__ __attribute__((aligned(16))) double tile[kTile * 14];
  const int t = threadIdx.x, p = blockIdx.y;
  const unsigned long long q = (unsigned long long)blockIdx.x * kThreads + t;
  const bool live = q < Q;
  double x[14];
#pragma unroll
  for (int c = 0; c < 14; c++) x[c] = live ? queries[q * 14 + c] : 0.0;
  unsigned int lim, excl;
  eligibility(mode, self_base + q, N, lim, excl);
  if (!live) lim = 0;
  List<KC> L;
  L.clear();
  const unsigned int lo = (unsigned int)p * part, hi = lo + part < N ? lo + part : N; // (lo + part <= 2^31 + part: no wrap)
  if (lim > hi) lim = hi;
  for (unsigned int base = lo; base < hi; base += kTile) {
    const unsigned int n = hi - base < (unsigned int)kTile ? hi - base : (unsigned int)kTile;
    __syncthreads(); // the previous tile has been read by everyone
    for (unsigned int w = t; w < n * 14; w += kThreads) tile[w] = nodes[(size_t)base * 14 + w];
    __syncthreads();
    // kRows rows at a time: as many independent chains in flight (four rows cost 60 registers more and a wavefront per SIMD).
    // Rows past n (the range's last tile) hold stale or unwritten LDS words — inside the array, since kTile is a multiple of
    // kRows — and are never offered: lim <= hi
    for (unsigned int r = 0; r < n; r += kRows) {
      double d2[kRows];
#pragma unroll
      for (int u = 0; u < kRows; u++) {
        const double2 *row = reinterpret_cast<const double2 *>(tile + (r + u) * 14); // 112-byte rows: 16-byte aligned
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 7; c++) {
          const double2 v = row[c];
          const double e0 = x[2 * c] - v.x;
          acc = CCMP_FMA(e0, e0, acc);
          const double e1 = x[2 * c + 1] - v.y;
          acc = CCMP_FMA(e1, e1, acc);
        }
        d2[u] = acc;
      }
#pragma unroll
      for (int u = 0; u < kRows; u++) {
        const unsigned int j = base + r + u;
        if (j < lim && j != excl) L.offer(d2[u], (int)j);
      }
    }
  }
  if (live) emit<KC>(o, q, p, L.d, L.i);
}

template <int KC>
__global__ __launch_bounds__(kThreads) void knn_few_kernel(const double *__restrict__ nodes, unsigned int N, const double *__restrict__ queries,
                                                           int mode, unsigned long long self_base, unsigned int part, KnnOut o)
{
  __shared__ double ld[kThreads * KC];
  __shared__ int li[kThreads * KC];
  const int t = threadIdx.x, p = blockIdx.x;
  const unsigned long long q = blockIdx.y;
  double x[14];
#pragma unroll
  for (int c = 0; c < 14; c++) x[c] = queries[q * 14 + c];
  unsigned int lim, excl;
  eligibility(mode, self_base + q, N, lim, excl);
  List<KC> L;
  L.clear();
  const unsigned int lo = (unsigned int)p * part, hi = lo + part < N ? lo + part : N;
  for (unsigned int j = lo + t; j < hi; j += kThreads) {
    const double *row = nodes + (size_t)j * 14;
    double v[14];
#pragma unroll
    for (int c = 0; c < 14; c++) v[c] = row[c];
    double d2 = 0.0;
#pragma unroll
    for (int c = 0; c < 14; c++) {
      const double e = x[c] - v[c];
      d2 = CCMP_FMA(e, e, d2);
    }
    if (j < lim && j != excl) L.offer(d2, (int)j);
  }
#pragma unroll
  for (int s = 0; s < KC; s++) { ld[t * KC + s] = L.d[s]; li[t * KC + s] = L.i[s]; }
  block_merge<KC, kThreads>(ld, li, t, L.d, L.i);
  if (t == 0) emit<KC>(o, q, p, L.d, L.i);
}

// the P <= NT lists of one query -> the k best
template <int KC, int NT>
__global__ __launch_bounds__(NT) void knn_merge_kernel(KnnOut o)
{
  __shared__ double ld[NT * KC];
  __shared__ int li[NT * KC];
  const int t = threadIdx.x;
  const size_t q = blockIdx.x;
  const size_t base = (q * (size_t)o.P + (size_t)t) * KC;
#pragma unroll
  for (int s = 0; s < KC; s++) {
    ld[t * KC + s] = t < o.P ? o.ws_d[base + s] : __builtin_inf();
    li[t * KC + s] = t < o.P ? o.ws_i[base + s] : kEmptyIdx;
  }
  double od[KC];
  int oi[KC];
  block_merge<KC, NT>(ld, li, t, od, oi);
  if (t == 0) {
    KnnOut one = o;
    one.P = 1;
    emit<KC>(one, q, 0, od, oi);
  }
}

// edge e = q * k + r of a connect call: 14 threads per edge
__global__ __launch_bounds__(256) void connect_gather_kernel(const double *__restrict__ nodes, const double *__restrict__ queries,
                                                             const int32_t *__restrict__ nbr_idx, unsigned long long E, int k, double *from, double *to)
{
  const unsigned long long w = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= E * 14) return;
  const unsigned long long e = w / 14, c = w % 14, q = e / (unsigned long long)k;
  const int32_t j = nbr_idx[e];
  const double target = queries[q * 14 + c];
  to[w] = target;
  from[w] = j < 0 ? target : nodes[(size_t)j * 14 + c];
}

// what an empty slot reports, written behind the traversal
__global__ __launch_bounds__(256) void connect_fix_kernel(const int32_t *__restrict__ nbr_idx, unsigned long long E, int32_t *n_states, uint8_t *ok,
                                                          int32_t *newton_iters, uint8_t *blocked, double *carry_out)
{
  const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= E || nbr_idx[e] >= 0) return;
  n_states[e] = 0;
  ok[e] = 0;
  if (newton_iters) newton_iters[e] = 0;
  if (blocked) blocked[e] = 0;
  if (carry_out) { carry_out[2 * e] = 0.0; carry_out[2 * e + 1] = 0.0; }
}

template <int KC>
hipError_t knn_launch(const ccmp_launch::KnnCall &c, const ccmp_launch::KnnShape &s, double *ws_d, int32_t *ws_i, hipStream_t st)
{
  const KnnOut o{c.nbr_idx, c.nbr_dist, ws_d, ws_i, c.k, (int)s.partitions};
  if (s.few)
    hipLaunchKernelGGL(knn_few_kernel<KC>, dim3(s.partitions, (unsigned int)c.Q), dim3(kThreads), 0, st, c.nodes, (unsigned int)c.N, c.queries, c.mode,
                       (unsigned long long)c.self_base, s.part, o);
  else
    hipLaunchKernelGGL(knn_many_kernel<KC>, dim3(s.groups, s.partitions), dim3(kThreads), 0, st, c.nodes, (unsigned int)c.N, c.queries,
                       (unsigned long long)c.Q, c.mode, (unsigned long long)c.self_base, s.part, o);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || s.partitions == 1) return e;
  if (s.partitions <= 64) hipLaunchKernelGGL((knn_merge_kernel<KC, 64>), dim3((unsigned int)c.Q), dim3(64), 0, st, o);
  else hipLaunchKernelGGL((knn_merge_kernel<KC, 256>), dim3((unsigned int)c.Q), dim3(256), 0, st, o);
  return hipGetLastError();
}

// ---- the object metric (ccmp_pose.h) --------------------------------------------------------------------------------------------
constexpr int kPoseTile = ccmp_launch::kKnnPoseTile;
static_assert(kPoseTile % kRows == 0, "knn_pose_many_kernel reads its tile kRows rows at a time");

// one node whose squared translation d2 passed no test yet, scanned in increasing index; lo = (z, qx), and row[2], row[3] = the
// rest of its quaternion.  fl(|dp| + rot) >= |dp| (rot >= 0, rounding is monotone), so List::bound filters on d2 as it does for the
// joint metric; a NaN d2 fails both tests, a NaN in the quaternions gives a NaN distance, which is below nothing.
template <int KC>
__device__ __forceinline__ void offer_pose(List<KC> &L, double d2, int idx, const double (&x)[7], double qx, const double2 *row)
{
  if (d2 < L.bound || d2 == __builtin_inf()) {
    const double2 v2 = row[2], v3 = row[3];
    const double dist = ccmp_sqrt(d2) + ccmp_pose_rot(x[3], x[4], x[5], x[6], qx, v2.x, v2.y, v3.x);
    if (key_less(dist, idx, L.d[KC - 1], L.i[KC - 1])) L.insert(dist, idx);
  }
}

template <int KC>
__global__ __launch_bounds__(kThreads) void knn_pose_many_kernel(const double *__restrict__ nodes, unsigned int N, const double *__restrict__ queries,
                                                                 unsigned long long Q, int mode, unsigned long long self_base, unsigned int part,
                                                                 KnnOut o)
{
  __shared__ __attribute__((aligned(16))) double tile[kPoseTile * 8];
  const int t = threadIdx.x, p = blockIdx.y;
  const unsigned long long q = (unsigned long long)blockIdx.x * kThreads + t;
  const bool live = q < Q;
  double x[7];
#pragma unroll
  for (int c = 0; c < 7; c++) x[c] = live ? queries[q * 8 + c] : 0.0;
  unsigned int lim, excl;
  eligibility(mode, self_base + q, N, lim, excl);
  if (!live) lim = 0;
  List<KC> L;
  L.clear();
  const unsigned int lo = (unsigned int)p * part, hi = lo + part < N ? lo + part : N;
  if (lim > hi) lim = hi;
  for (unsigned int base = lo; base < hi; base += kPoseTile) {
    const unsigned int n = hi - base < (unsigned int)kPoseTile ? hi - base : (unsigned int)kPoseTile;
    __syncthreads(); // the previous tile has been read by everyone
    {
      const double2 *src = reinterpret_cast<const double2 *>(nodes) + (size_t)base * 4; // the store's rows: 64 bytes, 16-byte aligned
      double2 *dst = reinterpret_cast<double2 *>(tile);
      for (unsigned int w = t; w < n * 4; w += kThreads) dst[w] = src[w]; // n <= kPoseTile: inside the tile; base + n <= N: inside the store
    }
    __syncthreads();
    // rows past n (the range's last tile) hold stale or unwritten LDS words, inside the array, and are never offered: lim <= hi
    for (unsigned int r = 0; r < n; r += kRows) {
      double d2[kRows], qx[kRows];
#pragma unroll
      for (int u = 0; u < kRows; u++) {
        const double2 *row = reinterpret_cast<const double2 *>(tile + (r + u) * 8);
        const double2 v0 = row[0], v1 = row[1];
        d2[u] = ccmp_pose_d2(x[0], x[1], x[2], v0.x, v0.y, v1.x);
        qx[u] = v1.y;
      }
#pragma unroll
      for (int u = 0; u < kRows; u++) {
        const unsigned int j = base + r + u;
        if (j < lim && j != excl) offer_pose<KC>(L, d2[u], (int)j, x, qx[u], reinterpret_cast<const double2 *>(tile + (r + u) * 8));
      }
    }
  }
  if (live) emit<KC>(o, q, p, L.d, L.i);
}

template <int KC>
__global__ __launch_bounds__(kThreads) void knn_pose_few_kernel(const double *__restrict__ nodes, unsigned int N, const double *__restrict__ queries,
                                                                int mode, unsigned long long self_base, unsigned int part, KnnOut o)
{
  __shared__ double ld[kThreads * KC];
  __shared__ int li[kThreads * KC];
  const int t = threadIdx.x, p = blockIdx.x;
  const unsigned long long q = blockIdx.y;
  double x[7];
#pragma unroll
  for (int c = 0; c < 7; c++) x[c] = queries[q * 8 + c];
  unsigned int lim, excl;
  eligibility(mode, self_base + q, N, lim, excl);
  List<KC> L;
  L.clear();
  const unsigned int lo = (unsigned int)p * part, hi = lo + part < N ? lo + part : N;
  for (unsigned int j = lo + t; j < hi; j += kThreads) {
    const double2 *row = reinterpret_cast<const double2 *>(nodes) + (size_t)j * 4;
    const double2 v0 = row[0], v1 = row[1];
    const double d2 = ccmp_pose_d2(x[0], x[1], x[2], v0.x, v0.y, v1.x);
    if (j < lim && j != excl) offer_pose<KC>(L, d2, (int)j, x, v1.y, row);
  }
#pragma unroll
  for (int s = 0; s < KC; s++) { ld[t * KC + s] = L.d[s]; li[t * KC + s] = L.i[s]; }
  block_merge<KC, kThreads>(ld, li, t, L.d, L.i);
  if (t == 0) emit<KC>(o, q, p, L.d, L.i);
}

// the pose of a joint state: compute_t_wo of the left arm (t_wo_kernel's arithmetic), then Eigen's Quaterniond(Matrix3d)
__global__ __launch_bounds__(64) void pose_from_joints_kernel(const ccmp_consts K, const double *__restrict__ joints, double *__restrict__ poses, size_t n)
{
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double x[7], Rw[9], pw[3], T[12], pose[8];
#pragma unroll
  for (int e = 0; e < 7; e++) x[e] = joints[i * 14 + e];
  ccmp::fk_arm(K, 0, x, Rw, pw);
  ccmp::mul33(Rw, K.t_o7i_R, T);
  T[9] = pw[0]; T[10] = pw[1]; T[11] = pw[2];
  ccmp::mulvec_acc(Rw, K.t_o7i_p, T + 9);
  ccmp_pose_of_t_wo(T, pose);
#pragma unroll
  for (int c = 0; c < 8; c++) poses[i * 8 + c] = pose[c];
}

// the caller's poses into the store: seven values and a zero pad
__global__ __launch_bounds__(256) void pose_store_kernel(const double *__restrict__ src, double *__restrict__ dst, size_t n)
{
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (w >= n * 8) return;
  dst[w] = (w & 7) == 7 ? 0.0 : src[w];
}

// the joint rows of pose-only vertices: NaN, never a neighbour under the joint metric
__global__ __launch_bounds__(256) void joints_fill_nan_kernel(double *__restrict__ dst, size_t words)
{
  const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (w < words) dst[w] = __builtin_nan("");
}

template <int KC>
hipError_t knn_pose_launch(const ccmp_launch::KnnCall &c, const ccmp_launch::KnnShape &s, double *ws_d, int32_t *ws_i, hipStream_t st)
{
  const KnnOut o{c.nbr_idx, c.nbr_dist, ws_d, ws_i, c.k, (int)s.partitions};
  if (s.few)
    hipLaunchKernelGGL(knn_pose_few_kernel<KC>, dim3(s.partitions, (unsigned int)c.Q), dim3(kThreads), 0, st, c.nodes, (unsigned int)c.N, c.queries, c.mode,
                       (unsigned long long)c.self_base, s.part, o);
  else
    hipLaunchKernelGGL(knn_pose_many_kernel<KC>, dim3(s.groups, s.partitions), dim3(kThreads), 0, st, c.nodes, (unsigned int)c.N, c.queries,
                       (unsigned long long)c.Q, c.mode, (unsigned long long)c.self_base, s.part, o);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || s.partitions == 1) return e;
  if (s.partitions <= 64) hipLaunchKernelGGL((knn_merge_kernel<KC, 64>), dim3((unsigned int)c.Q), dim3(64), 0, st, o);
  else hipLaunchKernelGGL((knn_merge_kernel<KC, 256>), dim3((unsigned int)c.Q), dim3(256), 0, st, o);
  return hipGetLastError();
}

}  // namespace

namespace ccmp_launch {

hipError_t knn(const KnnCall &c, const KnnShape &s, void *workspace, hipStream_t st)
{
  // workspace: distances [Q][P][KC] (doubles), then indices [Q][P][KC]
  double *ws_d = (double *)workspace;
  int32_t *ws_i = (int32_t *)(ws_d + c.Q * (size_t)s.partitions * (size_t)s.kc);
  switch (s.kc) {
    case 1: return knn_launch<1>(c, s, ws_d, ws_i, st);
    case 4: return knn_launch<4>(c, s, ws_d, ws_i, st);
    case 8: return knn_launch<8>(c, s, ws_d, ws_i, st);
    case 16: return knn_launch<16>(c, s, ws_d, ws_i, st);
  }
  return hipErrorInvalidValue;
}

hipError_t knn_pose(const KnnCall &c, const KnnShape &s, void *workspace, hipStream_t st)
{
  double *ws_d = (double *)workspace; // as knn(): distances [Q][P][KC], then indices
  int32_t *ws_i = (int32_t *)(ws_d + c.Q * (size_t)s.partitions * (size_t)s.kc);
  switch (s.kc) {
    case 1: return knn_pose_launch<1>(c, s, ws_d, ws_i, st);
    case 4: return knn_pose_launch<4>(c, s, ws_d, ws_i, st);
    case 8: return knn_pose_launch<8>(c, s, ws_d, ws_i, st);
    case 16: return knn_pose_launch<16>(c, s, ws_d, ws_i, st);
  }
  return hipErrorInvalidValue;
}

hipError_t pose_from_joints(const ccmp_consts *K, const double *joints, double *poses, size_t n, hipStream_t st)
{
  hipLaunchKernelGGL(pose_from_joints_kernel, dim3((unsigned int)((n + 63) / 64)), dim3(64), 0, st, *K, joints, poses, n);
  return hipGetLastError();
}

hipError_t pose_store(const double *src, double *dst, size_t n, hipStream_t st)
{
  hipLaunchKernelGGL(pose_store_kernel, dim3((unsigned int)((n * 8 + 255) / 256)), dim3(256), 0, st, src, dst, n);
  return hipGetLastError();
}

hipError_t joints_fill_nan(double *dst, size_t n, hipStream_t st)
{
  hipLaunchKernelGGL(joints_fill_nan_kernel, dim3((unsigned int)((n * 14 + 255) / 256)), dim3(256), 0, st, dst, n * 14);
  return hipGetLastError();
}

hipError_t connect_gather(const double *nodes, const double *queries, const int32_t *nbr_idx, size_t E, int k, double *from, double *to, hipStream_t st)
{
  const size_t blocks = (E * 14 + 255) / 256;
  hipLaunchKernelGGL(connect_gather_kernel, dim3((unsigned int)blocks), dim3(256), 0, st, nodes, queries, nbr_idx, (unsigned long long)E, k, from, to);
  return hipGetLastError();
}

hipError_t connect_fix(const int32_t *nbr_idx, size_t E, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out,
                       hipStream_t st)
{
  const size_t blocks = (E + 255) / 256;
  hipLaunchKernelGGL(connect_fix_kernel, dim3((unsigned int)blocks), dim3(256), 0, st, nbr_idx, (unsigned long long)E, n_states, ok, newton_iters, blocked,
                     carry_out);
  return hipGetLastError();
}

}  // namespace ccmp_launch
