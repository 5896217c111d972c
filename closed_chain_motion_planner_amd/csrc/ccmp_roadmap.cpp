// ccmp_roadmap.cpp — the device-resident roadmap store of the C ABI (include/ccmp.h: ccmp_roadmap_*) and the two host functions of the
// object metric.  A store is two device arrays, joints [cap][14] and poses [cap][8], and a size kept on the host; appends, reads and
// queries are launches and copies on the caller's stream, so stream order is the order of the calls.  The arithmetic lives in
// ccmp_pose.h (metric, pose of a t_wo) and ccmp_kernels_knn.hip (the k-NN kernels of both metrics, pose_from_joints_kernel); the
// checks and the gather -> traversal -> fix chain behind ccmp_roadmap_connect are ccmp_connect_batch's own (ccmp_api.cpp:
// ccmp_host::connect_checks / connect_edges), as is the workspace rule (ccmp_host::grow_buffer).
// The store also keeps the planner's graph: an edge list with weights and one component label per vertex, with the edge count and the
// edge floor as host state; growTree's tail (ccmp_roadmap_commit), explicit edges and closestFromGoal's scan are launches of
// ccmp_kernels_graph.hip, and their *_ref forms compile the same rule text here (ccmp_graph.h).  The planner's solution step, shortest
// paths on that graph (ccmp_path.h), is three more launches of the unit over a workspace the handle grows on first use; its *_ref form
// finds the distances by heap Dijkstra and the hops and predecessors from the same rule text.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <queue>
#include <utility>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_graph.h"
#include "ccmp_host.h"
#include "ccmp_ik.h"
#include "ccmp_launch.h"
#include "ccmp_path.h"
#include "ccmp_plan.h"
#include "ccmp_policy.h"
#include "ccmp_pose.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

struct ccmp_roadmap {
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  double *joints = nullptr; // [cap][14]
  double *poses = nullptr;  // [cap][8]
  size_t size = 0, cap = 0;
  double *qpose = nullptr;  // ccmp_roadmap_connect: the derived query poses [qpose_cap][8]
  size_t qpose_cap = 0;
  void *grow_ws = nullptr;  // ccmp_roadmap_grow: seeds [E][14] | the traversal's targets [Q][14] | its neighbours [E] (int32)
  size_t grow_ws_cap = 0;   // in edges
  // the graph (ccmp_graph.h): one label per vertex (allocated and moved with the rows), the edge list, and as host state the edge count
  // and the edge floor (1 + the largest endpoint of any edge: truncate never goes below it)
  int32_t *labels = nullptr; // [cap]
  int32_t *uv = nullptr;     // [cap_e][2]
  double *w = nullptr;       // [cap_e]
  size_t n_edges = 0, cap_e = 0, floor = 0;
  void *graph_ws = nullptr;  // commit / add_edges: ccmp_launch::GraphWork for graph_ws_cap slots
  size_t graph_ws_cap = 0;
  void *closest_ws = nullptr; // closest: the partitions' bests, distances [64][256] then indices (allocated with the store)
  void *path_ws = nullptr;    // shortest_paths: rounds [64][2] | d [F][N] (64-bit) | hops | pred | stamp [F][N] (int32); grown on first use
  size_t path_ws_cap = 0;     // in elements of F N, plus one
  size_t path_F = 0, path_N = 0; // the shape of the last call (what path_rounds and the host form's read-backs address)
};

namespace {

constexpr size_t kDefaultCapacity = 1024;

// Moves the store into a block of new_cap rows.  st != nullptr-able: the copy is ordered behind what `st` holds and `st` is waited
// for once before the old block goes; sync_device: the whole device is waited for first instead (ccmp_roadmap_reserve has no stream).
int regrow(ccmp_roadmap *rm, size_t new_cap, hipStream_t st, bool sync_device)
{
  if (new_cap > kMaxRows) return CCMP_EINVAL;
  ccmp_host::quiesce(rm->ctx);
  if (sync_device) HIP_TRY(hipDeviceSynchronize());
  double *nj = nullptr, *np = nullptr;
  int32_t *nl = nullptr;
  hipError_t e = hipMalloc((void **)&nj, new_cap * 14 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&np, new_cap * 8 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&nl, new_cap * sizeof(int32_t));
  if (e == hipSuccess && rm->size) e = hipMemcpyAsync(nl, rm->labels, rm->size * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && rm->size) e = hipMemcpyAsync(nj, rm->joints, rm->size * 14 * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && rm->size) e = hipMemcpyAsync(np, rm->poses, rm->size * 8 * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    if (nj) (void)hipFree(nj);
    if (np) (void)hipFree(np);
    if (nl) (void)hipFree(nl);
    return e == hipErrorOutOfMemory ? CCMP_ENOMEM : hip_fail(e, "ccmp_roadmap: growth");
  }
  if (rm->joints) (void)hipFree(rm->joints);
  if (rm->poses) (void)hipFree(rm->poses);
  if (rm->labels) (void)hipFree(rm->labels);
  rm->joints = nj;
  rm->poses = np;
  rm->labels = nl;
  rm->cap = new_cap;
  return CCMP_OK;
}

// the same for the edge block
int regrow_edges(ccmp_roadmap *rm, size_t new_cap, hipStream_t st)
{
  if (new_cap > kMaxRows) return CCMP_EINVAL;
  ccmp_host::quiesce(rm->ctx);
  int32_t *nuv = nullptr;
  double *nw = nullptr;
  hipError_t e = hipMalloc((void **)&nuv, new_cap * 2 * sizeof(int32_t));
  if (e == hipSuccess) e = hipMalloc((void **)&nw, new_cap * sizeof(double));
  if (e == hipSuccess && rm->n_edges) e = hipMemcpyAsync(nuv, rm->uv, rm->n_edges * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && rm->n_edges) e = hipMemcpyAsync(nw, rm->w, rm->n_edges * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    if (nuv) (void)hipFree(nuv);
    if (nw) (void)hipFree(nw);
    return e == hipErrorOutOfMemory ? CCMP_ENOMEM : hip_fail(e, "ccmp_roadmap: edge growth");
  }
  if (rm->uv) (void)hipFree(rm->uv);
  if (rm->w) (void)hipFree(rm->w);
  rm->uv = nuv;
  rm->w = nw;
  rm->cap_e = new_cap;
  return CCMP_OK;
}

// room for `rows` vertices and `edges` edges in all, before a graph call's first launch (at least doubling, as an append grows)
int graph_reserve(ccmp_roadmap *rm, size_t rows, size_t edges, hipStream_t st)
{
  if (rows > kMaxRows || edges > kMaxRows) return CCMP_EINVAL;
  if (rows > rm->cap) {
    const int rc = regrow(rm, rows > 2 * rm->cap ? rows : 2 * rm->cap > kMaxRows ? kMaxRows : 2 * rm->cap, st, false);
    if (rc != CCMP_OK) return rc;
  }
  if (edges > rm->cap_e) {
    const size_t twice = 2 * rm->cap_e > kMaxRows ? kMaxRows : 2 * rm->cap_e;
    const int rc = regrow_edges(rm, edges > twice ? edges : twice, st);
    if (rc != CCMP_OK) return rc;
  }
  return CCMP_OK;
}

ccmp_launch::GraphStore graph_store(const ccmp_roadmap *rm) { return ccmp_launch::GraphStore{rm->joints, rm->poses, rm->labels, rm->uv, rm->w, rm->size, rm->n_edges, rm->floor}; }

// the call's workspace for S slots (S >= the scan's items), cut out of rm->graph_ws
constexpr size_t kGraphSlotBytes = 8 + 64 + 4 + 4 + 6 * 4; // weight, mid_pose, flags, label, and masks .. base_e
int graph_work(ccmp_roadmap *rm, size_t S, ccmp_launch::GraphWork *w)
{
  const int rc = grow_buffer(rm->ctx, &rm->graph_ws, &rm->graph_ws_cap, S, S * kGraphSlotBytes + 64);
  if (rc != CCMP_OK) return rc;
  double *d = (double *)rm->graph_ws;
  w->weight = d;
  w->mid_pose = d + S;
  int32_t *i = (int32_t *)(d + 9 * S);
  w->flags = (uint32_t *)i;
  w->label = i + S;
  w->masks = (uint32_t *)(i + 2 * S);
  w->cnt_v = i + 3 * S;
  w->cnt_e = i + 4 * S;
  w->hi = i + 5 * S;
  w->base_v = i + 6 * S;
  w->base_e = i + 7 * S;
  w->totals = i + 8 * S; // 16 bytes of the 64 behind the arrays
  return CCMP_OK;
}

// what a commit checks before anything else (the store is there)
int commit_checks(size_t N, const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states, int max_states, const double *new_joints,
                  const double *new_poses, size_t Q, int k, const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index,
                  int32_t *grow_state)
{
  if (k < 1 || k > CCMP_KNN_MAX_K || n_roots < 0 || n_roots > CCMP_GRAPH_MAX_ROOTS || (flags & ~(unsigned int)CCMP_COMMIT_KEEP_ISOLATED)) return CCMP_EINVAL;
  if (n_roots > 0 && !roots) return CCMP_EINVAL;
  for (int i = 0; i < n_roots; i++)
    if (roots[i] < 0 || (size_t)roots[i] >= N) return CCMP_EINVAL;
  if (Q == 0) return CCMP_OK;
  if (max_states < 1 || !nbr_idx || !edge_ok || !n_states || !new_joints || !new_poses || !new_index || !mid_index || !grow_state) return CCMP_EINVAL;
  if (Q > kMaxRows / (size_t)(k + 1) || N > kMaxRows - Q * (size_t)(k + 1)) return CCMP_EINVAL;
  return CCMP_OK;
}

ccmp::graph_roots roots_of(const int32_t *roots, int n_roots)
{
  ccmp::graph_roots R{};
  for (int i = 0; i < n_roots; i++) R.v[i] = roots[i];
  R.n = n_roots;
  return R;
}

// the read-back that ends commit and add_edges: {vertices, edges, floor}
int graph_finish(ccmp_roadmap *rm, const int32_t *totals, hipStream_t st, size_t *vertices_added, size_t *edges_added)
{
  int32_t t[4] = {0, 0, 0, 0};
  { const int rc = read_back(t, totals, sizeof t, st); if (rc != CCMP_OK) return rc; }
  rm->size += (size_t)t[0];
  rm->n_edges += (size_t)t[1];
  rm->floor = (size_t)t[2];
  if (vertices_added) *vertices_added = (size_t)t[0];
  if (edges_added) *edges_added = (size_t)t[1];
  return CCMP_OK;
}

// cuts of the vertex range of a closest call: from N alone
void plan_closest(size_t N, unsigned int *part, unsigned int *partitions)
{
  size_t pt = 2048;
  if ((N + pt - 1) / pt > (size_t)ccmp_launch::kClosestMaxPartitions) {
    pt = (N + ccmp_launch::kClosestMaxPartitions - 1) / ccmp_launch::kClosestMaxPartitions;
    pt = (pt + 255) / 256 * 256;
  }
  *part = (unsigned int)pt;
  *partitions = N ? (unsigned int)((N + pt - 1) / pt) : 1;
}

// what every form of a shortest-path call checks first
int path_checks(const int32_t *src, const int32_t *dst, size_t F, int max_len, const double *cost, const int32_t *path_len, const int32_t *path)
{
  if (F > CCMP_PATH_MAX_PAIRS || max_len < 1 || !src || !dst || !cost || !path_len || !path) return CCMP_EINVAL;
  return CCMP_OK;
}

constexpr size_t kPathHeadBytes = CCMP_PATH_MAX_PAIRS * 2 * sizeof(int32_t); // the rounds, in front of the arrays
unsigned long long *path_d(const ccmp_roadmap *rm) { return (unsigned long long *)((char *)rm->path_ws + kPathHeadBytes); }
int32_t *path_pred(const ccmp_roadmap *rm) { return (int32_t *)(path_d(rm) + rm->path_F * rm->path_N) + rm->path_F * rm->path_N; }

int knn_checks(const ccmp_roadmap *rm, int metric, const void *queries, size_t Q, int k, int mode, const int32_t *nbr_idx)
{
  if (!rm) return no_handle();
  if (metric != CCMP_METRIC_JOINT && metric != CCMP_METRIC_OBJECT) return CCMP_EINVAL;
  if (k < 1 || k > CCMP_KNN_MAX_K || mode < CCMP_KNN_ALL || mode > CCMP_KNN_EARLIER || Q >= ((size_t)1 << 31)) return CCMP_EINVAL;
  if (Q > 0 && (!queries || !nbr_idx)) return CCMP_EINVAL;
  return CCMP_OK;
}

// the object metric's launches (arguments checked, Q > 0, the device current)
int knn_object(ccmp_roadmap *rm, const double *poses, size_t Q, int k, int mode, size_t self_base, int32_t *nbr_idx, double *nbr_dist, hipStream_t st)
{
  ccmp_ctx *ctx = rm->ctx;
  const ccmp_launch::KnnShape s = plan_knn_pose(ctx, Q, rm->size, k);
  { const int rc = grow_buffer(ctx, &ctx->knn_ws, &ctx->knn_ws_cap, s.workspace_bytes, s.workspace_bytes); if (rc != CCMP_OK) return rc; } // (a no-op behind ccmp_roadmap_connect, which sized it before its first launch)
  HIP_TRY(ccmp_launch::knn_pose(ccmp_launch::KnnCall{rm->poses, rm->size, poses, Q, k, mode, self_base, nbr_idx, nbr_dist}, s, ctx->knn_ws, st));
  return CCMP_OK;
}

}  // namespace

extern "C" {

double ccmp_pose_distance(const double a[8], const double b[8]) { return ccmp_pose_dist(a, b); }
void ccmp_pose_from_t_wo(const double t_wo[12], double pose[8]) { ccmp_pose_of_t_wo(t_wo, pose); }

ccmp_roadmap *ccmp_roadmap_create(ccmp_ctx *ctx, size_t capacity_hint)
{
  if (!ctx || capacity_hint > kMaxRows) return nullptr;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return nullptr;
  ccmp_roadmap *rm = new (std::nothrow) ccmp_roadmap();
  if (!rm) return nullptr;
  rm->ctx = ctx;
  rm->device = ctx->device;
  if (regrow(rm, capacity_hint ? capacity_hint : kDefaultCapacity, ctx->stream, false) != CCMP_OK) { delete rm; return nullptr; }
  if (regrow_edges(rm, capacity_hint ? capacity_hint : kDefaultCapacity, ctx->stream) != CCMP_OK ||
      hipMalloc(&rm->closest_ws, (size_t)CCMP_CLOSEST_MAX_FROM * ccmp_launch::kClosestMaxPartitions * (sizeof(double) + sizeof(int32_t))) != hipSuccess) {
    (void)hipGetLastError();
    ccmp_roadmap_destroy(rm);
    return nullptr;
  }
  return rm;
}

void ccmp_roadmap_destroy(ccmp_roadmap *rm)
{
  if (!rm) return;
  {
    DeviceGuard guard(rm->device);
    if (rm->ctx && ccmp_host::context_alive(rm->ctx)) ccmp_host::quiesce(rm->ctx);
    if (rm->joints) (void)hipFree(rm->joints);
    if (rm->poses) (void)hipFree(rm->poses);
    if (rm->qpose) (void)hipFree(rm->qpose);
    if (rm->grow_ws) (void)hipFree(rm->grow_ws);
    if (rm->labels) (void)hipFree(rm->labels);
    if (rm->uv) (void)hipFree(rm->uv);
    if (rm->w) (void)hipFree(rm->w);
    if (rm->graph_ws) (void)hipFree(rm->graph_ws);
    if (rm->closest_ws) (void)hipFree(rm->closest_ws);
    if (rm->path_ws) (void)hipFree(rm->path_ws);
  }
  delete rm;
}

size_t ccmp_roadmap_size(const ccmp_roadmap *rm) { return rm ? rm->size : 0; }

int ccmp_roadmap_reserve(ccmp_roadmap *rm, size_t n)
{
  if (!rm) return no_handle();
  if (n > kMaxRows) return CCMP_EINVAL;
  if (n <= rm->cap) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  return regrow(rm, n, rm->ctx->stream, true);
}

int ccmp_roadmap_append(ccmp_roadmap *rm, const ccmp_problem *p, const double *joints, const double *poses, size_t Q, size_t *first_index,
                        void *hip_stream)
{
  if (!rm) return no_handle();
  if (first_index) *first_index = rm->size;
  if (Q == 0) return CCMP_OK;
  if ((!joints && !poses) || Q > kMaxRows - rm->size) return CCMP_EINVAL;
  if (!poses) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; } // the poses are derived from the joints and the problem
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t need = rm->size + Q;
  if (need > rm->cap) {
    const int rc = regrow(rm, need > 2 * rm->cap ? need : 2 * rm->cap > kMaxRows ? kMaxRows : 2 * rm->cap, st, false);
    if (rc != CCMP_OK) return rc;
  }
  double *jrow = rm->joints + rm->size * 14, *prow = rm->poses + rm->size * 8; // rows size .. size + Q - 1 <= cap - 1
  if (joints) HIP_TRY(hipMemcpyAsync(jrow, joints, Q * 14 * sizeof(double), hipMemcpyDeviceToDevice, st));
  else HIP_TRY(ccmp_launch::joints_fill_nan(jrow, Q, st));
  if (poses) HIP_TRY(ccmp_launch::pose_store(poses, prow, Q, st));
  else {
    ccmp_consts K;
    ccmp_host::make_consts(*p, K);
    HIP_TRY(ccmp_launch::pose_from_joints(&K, jrow, prow, Q, st));
  }
  HIP_TRY(ccmp_launch::graph_iota(rm->labels, rm->size, Q, st)); // a new vertex is its own component
  rm->size = need;
  return CCMP_OK;
}

int ccmp_roadmap_set_joints(ccmp_roadmap *rm, size_t index, const double *joints, void *hip_stream)
{
  if (!rm) return no_handle();
  if (!joints || index >= rm->size) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  HIP_TRY(hipMemcpyAsync(rm->joints + index * 14, joints, 14 * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return CCMP_OK;
}

int ccmp_roadmap_truncate(ccmp_roadmap *rm, size_t n)
{
  if (!rm) return no_handle();
  if (n > rm->size || n < rm->floor) return CCMP_EINVAL; // a vertex with an edge stays (the reference removes only vertices without one)
  rm->size = n;
  return CCMP_OK;
}

int ccmp_roadmap_read(ccmp_roadmap *rm, size_t first, size_t count, double *joints_out, double *poses_out, void *hip_stream)
{
  if (!rm) return no_handle();
  if (first > rm->size || count > rm->size - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (joints_out) HIP_TRY(hipMemcpyAsync(joints_out, rm->joints + first * 14, count * 14 * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (poses_out) HIP_TRY(hipMemcpyAsync(poses_out, rm->poses + first * 8, count * 8 * sizeof(double), hipMemcpyDeviceToDevice, st));
  return CCMP_OK;
}

int ccmp_roadmap_knn(ccmp_roadmap *rm, int metric, const double *queries, size_t Q, int k, int mode, size_t self_base, int32_t *nbr_idx,
                     double *nbr_dist, void *hip_stream)
{
  { const int rc = knn_checks(rm, metric, queries, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  if (metric == CCMP_METRIC_JOINT) // the joint kernels over the store's joint rows: ccmp_knn_batch itself
    return ccmp_knn_batch(rm->ctx, rm->joints, rm->size, queries, Q, k, mode, self_base, nbr_idx, nbr_dist, hip_stream);
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  return knn_object(rm, queries, Q, k, mode, self_base, nbr_idx, nbr_dist, (hipStream_t)hip_stream);
}

// Neighbours by the store's metric, then ccmp_connect_batch's own chain on them (ccmp_host::connect_edges: gather, the traversal the
// caller would have run on the gathered pairs, the empty slots' values).  Everything is checked (ccmp_host::connect_checks: what
// ccmp_connect_batch checks) and every workspace has its size before the first launch.  One stream, no host synchronisation.
int ccmp_roadmap_connect(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, int metric, const double *query_joints,
                         const double *query_poses, size_t Q, int k, int mode, size_t self_base, int check_target, int max_states, int round_budget,
                         int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                         double *carry_out, void *hip_stream)
{
  { const int rc = knn_checks(rm, metric, query_joints, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  ccmp_ctx *ctx = rm->ctx;
  if (!p) return CCMP_EINVAL;
  if (Q == 0) { const int rc = problem_ok(p); return rc != CCMP_OK ? rc : (scene && (scene->device != ctx->device || std::isnan(margin)) ? CCMP_EINVAL : CCMP_OK); }
  { const int rc = connect_checks(ctx, p, scene, margin, max_states, states, n_states, ok, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t E = Q * (size_t)k;
  const bool object = metric == CCMP_METRIC_OBJECT;
  const ccmp_launch::KnnShape s = object ? plan_knn_pose(ctx, Q, rm->size, k) : plan_knn(ctx, Q, rm->size, k);
  { const int rc = grow_buffer(ctx, &ctx->knn_ws, &ctx->knn_ws_cap, s.workspace_bytes, s.workspace_bytes); if (rc != CCMP_OK) return rc; }
  { const int rc = grow_buffer(ctx, (void **)&ctx->connect_ws, &ctx->connect_ws_cap, E, E * 28 * sizeof(double)); if (rc != CCMP_OK) return rc; }
  if (object && !query_poses) {
    const int rc = grow_buffer(ctx, (void **)&rm->qpose, &rm->qpose_cap, Q, Q * 8 * sizeof(double));
    if (rc != CCMP_OK) return rc;
  }
  if (!object) {
    const int rc = ccmp_knn_batch(ctx, rm->joints, rm->size, query_joints, Q, k, mode, self_base, nbr_idx, nbr_dist, hip_stream);
    if (rc != CCMP_OK) return rc;
  } else {
    if (!query_poses) {
      ccmp_consts K;
      ccmp_host::make_consts(*p, K);
      HIP_TRY(ccmp_launch::pose_from_joints(&K, query_joints, rm->qpose, Q, st));
      query_poses = rm->qpose;
    }
    const int rc = knn_object(rm, query_poses, Q, k, mode, self_base, nbr_idx, nbr_dist, st);
    if (rc != CCMP_OK) return rc;
  }
  return connect_edges(ctx, p, scene, margin, rm->joints, query_joints, Q, k, check_target, max_states, round_budget, nbr_idx, states, n_states, ok,
                       newton_iters, blocked, carry_out, hip_stream);
}

// growTree's device part: the object-metric k-NN, the neighbours' joint rows as seed slots, the IK, then ccmp_roadmap_connect's own chain
// from each neighbour to the new state.  Every check runs and every workspace has its size before the first launch; one stream, no
// host synchronisation.  The traversal reads a copy of the neighbours in which a target without a state, and a neighbour without
// joints, are empty slots, and a copy of the new states in which a missing one is a row of zeros (never an endpoint: all its slots
// are empty): no NaN reaches a traversal kernel.
// vet: the IK is ccmp_pose_ik_vetted_batch's (csrc/ccmp_ik_vet.h) on the call's scene and margin, ik_clearance (nullable) its chosen states' clearances
static int grow_common(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts, const double *query_poses,
                       size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index, int check_target, int max_states,
                       int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok, int32_t *ik_which, double *states,
                       int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out, void *hip_stream, bool vet,
                       double *ik_clearance)
{
  { const int rc = knn_checks(rm, CCMP_METRIC_OBJECT, query_poses, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  ccmp_ctx *ctx = rm->ctx;
  if (!p || k > CCMP_IK_MAX_SEEDS) return CCMP_EINVAL;
  ccmp::ik_params P;
  { const int rc = ik_checks(p, opts, Q, k, &P); if (rc != CCMP_OK) return rc; }
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
  if (vet) { const int rc = ik_vet_checks(ctx, scene, margin); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  if (!q_new || !ik_ok || !ik_which) return CCMP_EINVAL;
  { const int rc = connect_checks(ctx, p, scene, margin, max_states, states, n_states, ok, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t E = Q * (size_t)k;
  const ccmp_launch::KnnShape s = plan_knn_pose(ctx, Q, rm->size, k);
  { const int rc = grow_buffer(ctx, &ctx->knn_ws, &ctx->knn_ws_cap, s.workspace_bytes, s.workspace_bytes); if (rc != CCMP_OK) return rc; }
  { const int rc = grow_buffer(ctx, (void **)&ctx->connect_ws, &ctx->connect_ws_cap, E, E * 28 * sizeof(double)); if (rc != CCMP_OK) return rc; }
  { const int rc = grow_buffer(ctx, &rm->grow_ws, &rm->grow_ws_cap, E, E * (28 * sizeof(double) + sizeof(int32_t))); if (rc != CCMP_OK) return rc; }
  { const int rc = vet ? ik_vetted_reserve(ctx, Q, k, P) : ik_reserve(ctx, ik_candidates(Q, k, P)); if (rc != CCMP_OK) return rc; }
  double *seeds = (double *)rm->grow_ws, *q_trav = seeds + E * 14; // Q <= E rows
  int32_t *masked = (int32_t *)(seeds + E * 28);
  { const int rc = knn_object(rm, query_poses, Q, k, mode, self_base, nbr_idx, nbr_dist, st); if (rc != CCMP_OK) return rc; }
  HIP_TRY(ccmp_launch::ik_gather_seeds(rm->joints, nbr_idx, E, seeds, st));
  {
    const int rc = vet ? ik_vetted_launches(ctx, p, P, query_poses, seeds, Q, k, rng_seed, first_index, scene, margin, q_new, ik_ok, ik_which, nullptr, nullptr,
                                            nullptr, nullptr, ik_clearance, st)
                       : ik_launches(ctx, p, P, query_poses, seeds, Q, k, rng_seed, first_index, q_new, ik_ok, ik_which, nullptr, nullptr, st);
    if (rc != CCMP_OK) return rc;
  }
  HIP_TRY(ccmp_launch::ik_grow_prepare(rm->joints, nbr_idx, ik_ok, q_new, Q, k, masked, q_trav, st));
  return connect_edges(ctx, p, scene, margin, rm->joints, q_trav, Q, k, check_target, max_states, round_budget, masked, states, n_states, ok, newton_iters,
                       blocked, carry_out, hip_stream);
}

int ccmp_roadmap_grow(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts, const double *query_poses,
                      size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index, int check_target, int max_states,
                      int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok, int32_t *ik_which, double *states,
                      int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out, void *hip_stream)
{
  return grow_common(rm, p, scene, margin, opts, query_poses, Q, k, mode, self_base, rng_seed, first_index, check_target, max_states, round_budget, nbr_idx,
                     nbr_dist, q_new, ik_ok, ik_which, states, n_states, ok, newton_iters, blocked, carry_out, hip_stream, false, nullptr);
}

// ccmp_roadmap_grow with the vetted IK in place of the plain one: the scene is required and serves the IK and the traversals under the one margin
int ccmp_roadmap_grow_vetted(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                             const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index, int check_target,
                             int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok, int32_t *ik_which,
                             double *ik_clearance, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out,
                             void *hip_stream)
{
  return grow_common(rm, p, scene, margin, opts, query_poses, Q, k, mode, self_base, rng_seed, first_index, check_target, max_states, round_budget, nbr_idx,
                     nbr_dist, q_new, ik_ok, ik_which, states, n_states, ok, newton_iters, blocked, carry_out, hip_stream, true, ik_clearance);
}

// the host form of set_joints (growTree hands over the result of its IK): synchronous on the context's stream
int ccmp_roadmap_set_joints_host(ccmp_roadmap *rm, size_t index, const double *joints)
{
  if (!rm) return no_handle();
  if (!joints || index >= rm->size) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(rm->ctx, __func__);
  sg.up(rm->joints + index * 14, joints, 14 * sizeof(double));
  return sg.finish(CCMP_OK);
}

// ---- host forms: synchronous on the context's stream; only the new rows / the queries go up.  Each one: its checks (before the device
// guard and before any buffer is touched), the pieces of the staging block, the uploads, the device-pointer form unless an upload
// failed, the downloads if it succeeded, and StagedCall::finish, which waits for the stream on every path ------------------------------
int ccmp_roadmap_append_host(ccmp_roadmap *rm, const ccmp_problem *p, const double *joints, const double *poses, size_t Q, size_t *first_index)
{
  if (!rm) return no_handle();
  if (first_index) *first_index = rm->size;
  if (Q == 0) return CCMP_OK;
  if ((!joints && !poses) || Q > kMaxRows - rm->size) return CCMP_EINVAL;
  if (!poses) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  StagedCall sg(ctx, __func__);
  const size_t jb = Q * 14 * sizeof(double), pb = Q * 8 * sizeof(double);
  const size_t off_j = sg.add(joints ? jb : 0), off_p = sg.add(poses ? pb : 0); // an absent array is a piece of no bytes
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_j, joints, jb);
  sg.up(off_p, poses, pb);
  int rc = CCMP_OK;
  if (sg.copy_ok()) rc = ccmp_roadmap_append(rm, p, sg.at<const double>(off_j, joints), sg.at<const double>(off_p, poses), Q, first_index, ctx->stream);
  return sg.finish(rc);
}

int ccmp_roadmap_read_host(ccmp_roadmap *rm, size_t first, size_t count, double *joints_out, double *poses_out)
{
  if (!rm) return no_handle();
  if (first > rm->size || count > rm->size - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(rm->ctx, __func__);
  sg.down(joints_out, rm->joints + first * 14, count * 14 * sizeof(double));
  sg.down(poses_out, rm->poses + first * 8, count * 8 * sizeof(double));
  return sg.finish(CCMP_OK);
}

int ccmp_roadmap_knn_host(ccmp_roadmap *rm, int metric, const double *queries, size_t Q, int k, int mode, size_t self_base, int32_t *nbr_idx,
                          double *nbr_dist)
{
  { const int rc = knn_checks(rm, metric, queries, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  const size_t S = Q * (size_t)k, qb = Q * (metric == CCMP_METRIC_JOINT ? 14 : 8) * sizeof(double);
  StagedCall sg(ctx, __func__);
  const size_t off_q = sg.add(qb), off_d = sg.add(S * sizeof(double) + S * sizeof(int32_t)); // distances then indices, one piece
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_q, queries, qb);
  double *d_dev = sg.at<double>(off_d);
  int32_t *i_dev = (int32_t *)(d_dev + S);
  int rc = CCMP_OK;
  if (sg.copy_ok()) rc = ccmp_roadmap_knn(rm, metric, sg.at<const double>(off_q), Q, k, mode, self_base, i_dev, nbr_dist ? d_dev : nullptr, ctx->stream);
  // with distances both arrays come down in one copy, into a bounce vector (no room for it: CCMP_ENOMEM, after the wait); without, the
  // indices alone
  std::vector<char> back;
  if (rc == CCMP_OK && nbr_dist) {
    try { back.resize(S * (sizeof(double) + sizeof(int32_t))); } catch (...) { rc = CCMP_ENOMEM; }
  }
  if (rc == CCMP_OK) {
    if (nbr_dist) sg.down(back.data(), d_dev, back.size());
    else sg.down(nbr_idx, i_dev, S * sizeof(int32_t));
  }
  rc = sg.finish(rc);
  if (rc != CCMP_OK) return rc;
  if (nbr_dist) {
    memcpy(nbr_dist, back.data(), S * sizeof(double));
    memcpy(nbr_idx, back.data() + S * sizeof(double), S * sizeof(int32_t));
  }
  return CCMP_OK;
}

int ccmp_roadmap_connect_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, int metric,
                              const double *query_joints, const double *query_poses, size_t Q, int k, int mode, size_t self_base, int check_target,
                              int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok,
                              int32_t *newton_iters, uint8_t *blocked, double *carry_out)
{
  { const int rc = knn_checks(rm, metric, query_joints, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (!p) return CCMP_EINVAL;
  if (Q == 0) return CCMP_OK;
  { const int rc = connect_checks(rm->ctx, p, scene, margin, max_states, states, n_states, ok, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; } // before any buffer is touched
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  const size_t E = Q * (size_t)k, jb = Q * 14 * sizeof(double), pb = Q * 8 * sizeof(double), sb = E * (size_t)max_states * 14 * sizeof(double);
  StagedCall sg(ctx, __func__);
  const size_t off_j = sg.add(jb), off_p = sg.add(query_poses ? pb : 0), off_i = sg.add(E * sizeof(int32_t)), off_d = sg.add(E * sizeof(double)),
               off_st = sg.add(sb), off_n = sg.add(E * sizeof(int32_t)), off_ok = sg.add(E), off_it = sg.add(E * sizeof(int32_t)), off_bl = sg.add(E),
               off_co = sg.add(E * 2 * sizeof(double));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_j, query_joints, jb);
  sg.up(off_p, query_poses, pb);
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ccmp_roadmap_connect(rm, p, scene, margin, metric, sg.at<const double>(off_j), sg.at<const double>(off_p, query_poses), Q, k, mode, self_base,
                              check_target, max_states, round_budget, sg.at<int32_t>(off_i), sg.at<double>(off_d, nbr_dist), sg.at<double>(off_st),
                              sg.at<int32_t>(off_n), sg.at<uint8_t>(off_ok), sg.at<int32_t>(off_it, newton_iters), sg.at<uint8_t>(off_bl, blocked),
                              sg.at<double>(off_co, carry_out), ctx->stream);
  if (rc == CCMP_OK) {
    sg.down(nbr_idx, off_i, E * sizeof(int32_t));
    sg.down(nbr_dist, off_d, E * sizeof(double));
    sg.down(states, off_st, sb);
    sg.down(n_states, off_n, E * sizeof(int32_t));
    sg.down(ok, off_ok, E);
    sg.down(newton_iters, off_it, E * sizeof(int32_t));
    sg.down(blocked, off_bl, E);
    sg.down(carry_out, off_co, E * 2 * sizeof(double));
  }
  return sg.finish(rc);
}

static int grow_host_common(const char *entry, ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                            const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index,
                            int check_target, int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok,
                            int32_t *ik_which, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out,
                            bool vet, double *ik_clearance)
{
  { const int rc = knn_checks(rm, CCMP_METRIC_OBJECT, query_poses, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (!p || k > CCMP_IK_MAX_SEEDS) return CCMP_EINVAL;
  { ccmp::ik_params P; const int rc = ik_checks(p, opts, Q, k, &P); if (rc != CCMP_OK) return rc; }
  if (vet) { const int rc = ik_vet_checks(rm->ctx, scene, margin); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  if (!q_new || !ik_ok || !ik_which) return CCMP_EINVAL;
  { const int rc = connect_checks(rm->ctx, p, scene, margin, max_states, states, n_states, ok, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; } // before any buffer is touched
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  const size_t E = Q * (size_t)k, pb = Q * 8 * sizeof(double), sb = E * (size_t)max_states * 14 * sizeof(double);
  StagedCall sg(ctx, entry);
  const size_t off_p = sg.add(pb), off_i = sg.add(E * sizeof(int32_t)), off_d = sg.add(E * sizeof(double)), off_q = sg.add(Q * 14 * sizeof(double)),
               off_io = sg.add(Q), off_iw = sg.add(Q * sizeof(int32_t)), off_st = sg.add(sb), off_n = sg.add(E * sizeof(int32_t)), off_ok = sg.add(E),
               off_it = sg.add(E * sizeof(int32_t)), off_bl = sg.add(E), off_co = sg.add(E * 2 * sizeof(double)), off_ic = sg.add(ik_clearance ? Q * sizeof(double) : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_p, query_poses, pb);
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = grow_common(rm, p, scene, margin, opts, sg.at<const double>(off_p), Q, k, mode, self_base, rng_seed, first_index, check_target, max_states,
                     round_budget, sg.at<int32_t>(off_i), sg.at<double>(off_d, nbr_dist), sg.at<double>(off_q), sg.at<uint8_t>(off_io),
                     sg.at<int32_t>(off_iw), sg.at<double>(off_st), sg.at<int32_t>(off_n), sg.at<uint8_t>(off_ok), sg.at<int32_t>(off_it, newton_iters),
                     sg.at<uint8_t>(off_bl, blocked), sg.at<double>(off_co, carry_out), ctx->stream, vet, sg.at<double>(off_ic, ik_clearance));
  if (rc == CCMP_OK) {
    sg.down(nbr_idx, off_i, E * sizeof(int32_t));
    sg.down(nbr_dist, off_d, E * sizeof(double));
    sg.down(q_new, off_q, Q * 14 * sizeof(double));
    sg.down(ik_ok, off_io, Q);
    sg.down(ik_which, off_iw, Q * sizeof(int32_t));
    sg.down(states, off_st, sb);
    sg.down(n_states, off_n, E * sizeof(int32_t));
    sg.down(ok, off_ok, E);
    sg.down(newton_iters, off_it, E * sizeof(int32_t));
    sg.down(blocked, off_bl, E);
    sg.down(carry_out, off_co, E * 2 * sizeof(double));
    sg.down(ik_clearance, off_ic, Q * sizeof(double));
  }
  return sg.finish(rc);
}

int ccmp_roadmap_grow_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                           const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index,
                           int check_target, int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok,
                           int32_t *ik_which, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out)
{
  return grow_host_common(__func__, rm, p, scene, margin, opts, query_poses, Q, k, mode, self_base, rng_seed, first_index, check_target, max_states,
                          round_budget, nbr_idx, nbr_dist, q_new, ik_ok, ik_which, states, n_states, ok, newton_iters, blocked, carry_out, false, nullptr);
}

int ccmp_roadmap_grow_vetted_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                                  const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index,
                                  int check_target, int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok,
                                  int32_t *ik_which, double *ik_clearance, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters,
                                  uint8_t *blocked, double *carry_out)
{
  return grow_host_common(__func__, rm, p, scene, margin, opts, query_poses, Q, k, mode, self_base, rng_seed, first_index, check_target, max_states,
                          round_budget, nbr_idx, nbr_dist, q_new, ik_ok, ik_which, states, n_states, ok, newton_iters, blocked, carry_out, true, ik_clearance);
}

// ---- the graph: edges, components, growTree's tail, closestFromGoal's scan (ccmp_graph.h) ------------------------------------------------
double ccmp_joint_distance(const double a[14], const double b[14]) { return ccmp::graph_joint_dist(a, b); }

int ccmp_graph_labels_ref(const int32_t *uv, size_t E, size_t N, int32_t *labels)
{
  if (N > kMaxRows || (N > 0 && !labels) || (E > 0 && !uv)) return CCMP_EINVAL;
  for (size_t e = 0; e < E; e++) // what ccmp_roadmap_add_edges_host refuses: an endpoint that is no vertex, a loop
    if (uv[2 * e] < 0 || (size_t)uv[2 * e] >= N || uv[2 * e + 1] < 0 || (size_t)uv[2 * e + 1] >= N || uv[2 * e] == uv[2 * e + 1]) return CCMP_EINVAL;
  for (size_t i = 0; i < N; i++) labels[i] = (int32_t)i;
  auto find = [&](int32_t x) { while (labels[x] != x) { labels[x] = labels[labels[x]]; x = labels[x]; } return x; };
  for (size_t e = 0; e < E; e++) {
    const int32_t a = find(uv[2 * e]), b = find(uv[2 * e + 1]);
    if (a != b) labels[a > b ? a : b] = a > b ? b : a; // the smaller root stays: a root is the smallest index of its tree
  }
  for (size_t i = 0; i < N; i++) labels[i] = find((int32_t)i);
  return CCMP_OK;
}

size_t ccmp_roadmap_num_edges(const ccmp_roadmap *rm) { return rm ? rm->n_edges : 0; }

int ccmp_roadmap_commit(ccmp_roadmap *rm, const ccmp_problem *p, const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states,
                        const double *states, int max_states, const double *new_joints, const double *new_poses, const uint8_t *vertex_ok, size_t Q, int k,
                        const double *goal_pose, const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index,
                        int32_t *grow_state, size_t *vertices_added, size_t *edges_added, void *hip_stream)
{
  if (!rm) return no_handle();
  if (vertices_added) *vertices_added = 0;
  if (edges_added) *edges_added = 0;
  { const int rc = commit_checks(rm->size, nbr_idx, edge_ok, n_states, max_states, new_joints, new_poses, Q, k, roots, n_roots, flags, new_index, mid_index, grow_state); if (rc != CCMP_OK) return rc; }
  const bool mids = states && goal_pose;
  if (mids) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  const size_t S = Q * (size_t)k;
  if (rm->n_edges > kMaxRows - S) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  { const int rc = graph_reserve(rm, rm->size + Q + S, rm->n_edges + S, st); if (rc != CCMP_OK) return rc; } // the worst case, before the first launch
  ccmp_launch::GraphWork w;
  { const int rc = graph_work(rm, S, &w); if (rc != CCMP_OK) return rc; }
  ccmp_consts K{};
  if (mids) ccmp_host::make_consts(*p, K);
  const ccmp::graph_roots R = roots_of(roots, n_roots);
  ccmp_launch::GraphCommit c{mids ? &K : nullptr, nbr_idx, edge_ok, n_states, states, max_states, new_joints, new_poses, vertex_ok, Q, k, {0, 0, 0, 0, 0, 0, 0, 0},
                             mids ? 1 : 0, &R, (flags & CCMP_COMMIT_KEEP_ISOLATED) ? 1 : 0, new_index, mid_index, grow_state};
  if (mids) memcpy(c.goal, goal_pose, 7 * sizeof(double));
  const ccmp_launch::GraphStore gs = graph_store(rm);
  HIP_TRY(ccmp_launch::graph_commit(gs, w, c, st));
  HIP_TRY(ccmp_launch::graph_components(gs, w.totals, rm->size + Q + S, S, st));
  return graph_finish(rm, w.totals, st, vertices_added, edges_added);
}

int ccmp_roadmap_commit_ref(const ccmp_problem *p, const double *store_joints, const double *store_poses, const int32_t *labels, size_t N,
                            const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states, const double *states, int max_states,
                            const double *new_joints, const double *new_poses, const uint8_t *vertex_ok, size_t Q, int k, const double *goal_pose,
                            const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index, int32_t *grow_state,
                            double *rows_joints, double *rows_poses, int32_t *edges_uv, double *edges_w, size_t *vertices_added, size_t *edges_added)
{
  if (vertices_added) *vertices_added = 0;
  if (edges_added) *edges_added = 0;
  if (N > 0 && (!store_joints || !store_poses || !labels)) return CCMP_EINVAL;
  { const int rc = commit_checks(N, nbr_idx, edge_ok, n_states, max_states, new_joints, new_poses, Q, k, roots, n_roots, flags, new_index, mid_index, grow_state); if (rc != CCMP_OK) return rc; }
  const bool mids = states && goal_pose;
  if (mids) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  if (!rows_joints || !rows_poses || !edges_uv || !edges_w) return CCMP_EINVAL;
  ccmp_consts K{};
  if (mids) ccmp_host::make_consts(*p, K);
  const ccmp::graph_roots R = roots_of(roots, n_roots);
  double goal[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (mids) memcpy(goal, goal_pose, 7 * sizeof(double));
  size_t nv = 0, ne = 0;
  for (size_t q = 0; q < Q; q++) {
    uint32_t f[CCMP_KNN_MAX_K];
    int32_t lab[CCMP_KNN_MAX_K];
    double wgt[CCMP_KNN_MAX_K], mid[CCMP_KNN_MAX_K][8];
    for (int r = 0; r < k; r++) {
      const size_t e = q * (size_t)k + (size_t)r;
      lab[r] = 0;
      wgt[r] = 0.0;
      f[r] = ccmp::graph_slot_eval(K, mids, store_joints, store_poses, labels, (uint32_t)N, R, nbr_idx[e], edge_ok[e], n_states[e], max_states,
                                   states ? states + e * (size_t)max_states * 14 : nullptr, new_joints + q * 14, goal, &lab[r], &wgt[r], mid[r]);
    }
    const ccmp::graph_decision d = ccmp::graph_decide(f, lab, k, vertex_ok ? vertex_ok[q] != 0 : 1, (flags & CCMP_COMMIT_KEEP_ISOLATED) ? 1 : 0);
    grow_state[q] = d.state;
    const size_t t = N + nv;
    new_index[q] = d.keep ? (int32_t)t : -1;
    if (d.keep) {
      memcpy(rows_joints + nv * 14, new_joints + q * 14, 14 * sizeof(double));
      memcpy(rows_poses + nv * 8, new_poses + q * 8, 7 * sizeof(double));
      rows_poses[nv * 8 + 7] = 0.0;
      nv++;
    }
    for (int r = 0; r < k; r++)
      if (d.reached >> r & 1u) {
        edges_uv[2 * ne] = nbr_idx[q * (size_t)k + r];
        edges_uv[2 * ne + 1] = (int32_t)t;
        edges_w[ne++] = wgt[r];
      }
    for (int r = 0; r < k; r++) {
      const size_t e = q * (size_t)k + (size_t)r;
      mid_index[e] = -1;
      if (!(d.mid >> r & 1u)) continue;
      memcpy(rows_joints + nv * 14, states + (e * (size_t)max_states + (size_t)(n_states[e] - 1)) * 14, 14 * sizeof(double));
      memcpy(rows_poses + nv * 8, mid[r], 8 * sizeof(double));
      mid_index[e] = (int32_t)(N + nv);
      edges_uv[2 * ne] = nbr_idx[e];
      edges_uv[2 * ne + 1] = (int32_t)(N + nv);
      edges_w[ne++] = wgt[r];
      nv++;
    }
  }
  if (vertices_added) *vertices_added = nv;
  if (edges_added) *edges_added = ne;
  return CCMP_OK;
}

int ccmp_roadmap_add_edges(ccmp_roadmap *rm, const int32_t *uv, size_t E, size_t *rejected, void *hip_stream)
{
  if (!rm) return no_handle();
  if (rejected) *rejected = 0;
  if (E == 0) return CCMP_OK;
  if (!uv || E > kMaxRows || rm->n_edges > kMaxRows - E) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  { const int rc = graph_reserve(rm, rm->size, rm->n_edges + E, st); if (rc != CCMP_OK) return rc; }
  ccmp_launch::GraphWork w;
  { const int rc = graph_work(rm, E, &w); if (rc != CCMP_OK) return rc; }
  const ccmp_launch::GraphStore gs = graph_store(rm);
  HIP_TRY(ccmp_launch::graph_add_edges(gs, w, uv, E, st));
  HIP_TRY(ccmp_launch::graph_components(gs, w.totals, rm->size, E, st));
  size_t added = 0;
  { const int rc = graph_finish(rm, w.totals, st, nullptr, &added); if (rc != CCMP_OK) return rc; }
  if (rejected) *rejected = E - added;
  return CCMP_OK;
}

int ccmp_roadmap_read_edges(ccmp_roadmap *rm, size_t first, size_t count, int32_t *uv_out, double *w_out, void *hip_stream)
{
  if (!rm) return no_handle();
  if (first > rm->n_edges || count > rm->n_edges - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (uv_out) HIP_TRY(hipMemcpyAsync(uv_out, rm->uv + first * 2, count * 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (w_out) HIP_TRY(hipMemcpyAsync(w_out, rm->w + first, count * sizeof(double), hipMemcpyDeviceToDevice, st));
  return CCMP_OK;
}

int ccmp_roadmap_read_labels(ccmp_roadmap *rm, size_t first, size_t count, int32_t *labels_out, void *hip_stream)
{
  if (!rm) return no_handle();
  if (first > rm->size || count > rm->size - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  if (!labels_out) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  HIP_TRY(hipMemcpyAsync(labels_out, rm->labels + first, count * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return CCMP_OK;
}

int ccmp_roadmap_closest(ccmp_roadmap *rm, const int32_t *from_idx, size_t F, const double *target_pose, int32_t *idx, double *dist, double *from_dist,
                         void *hip_stream)
{
  if (!rm) return no_handle();
  if (F == 0) return CCMP_OK;
  if (F > CCMP_CLOSEST_MAX_FROM || !from_idx || !target_pose || !idx || !dist || !from_dist) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  unsigned int part, partitions;
  plan_closest(rm->size, &part, &partitions);
  double *ws_d = (double *)rm->closest_ws;
  int32_t *ws_i = (int32_t *)(ws_d + (size_t)CCMP_CLOSEST_MAX_FROM * ccmp_launch::kClosestMaxPartitions);
  HIP_TRY(ccmp_launch::graph_closest(graph_store(rm), from_idx, F, target_pose, part, partitions, ws_d, ws_i, idx, dist, from_dist, (hipStream_t)hip_stream));
  return CCMP_OK;
}

int ccmp_roadmap_closest_ref(const double *store_poses, const int32_t *labels, size_t N, const int32_t *from_idx, size_t F, const double *target_pose,
                             int32_t *idx, double *dist, double *from_dist)
{
  if (F == 0) return CCMP_OK;
  if (F > CCMP_CLOSEST_MAX_FROM || N > kMaxRows || !store_poses || !labels || !from_idx || !target_pose || !idx || !dist || !from_dist) return CCMP_EINVAL;
  for (size_t f = 0; f < F; f++)
    if (from_idx[f] < 0 || (size_t)from_idx[f] >= N) return CCMP_EINVAL;
  double x[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  memcpy(x, target_pose, 7 * sizeof(double));
  for (size_t f = 0; f < F; f++) {
    const int32_t lab = labels[from_idx[f]];
    double bd = __builtin_inf();
    int32_t bi = 0x7fffffff;
    for (size_t j = 0; j < N; j++) {
      if (labels[j] != lab) continue;
      const double d = ccmp_pose_dist(store_poses + j * 8, x);
      if (ccmp::graph_closer(d, (int32_t)j, bd, bi)) { bd = d; bi = (int32_t)j; }
    }
    idx[f] = bi == 0x7fffffff ? -1 : bi;
    dist[f] = bd;
    from_dist[f] = ccmp_pose_dist(store_poses + (size_t)from_idx[f] * 8, x);
  }
  return CCMP_OK;
}

// ---- host forms of the graph's entries: synchronous on the context's stream --------------------------------------------------------------
int ccmp_roadmap_commit_host(ccmp_roadmap *rm, const ccmp_problem *p, const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states,
                             const double *states, int max_states, const double *new_joints, const double *new_poses, const uint8_t *vertex_ok, size_t Q,
                             int k, const double *goal_pose, const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index,
                             int32_t *grow_state, size_t *vertices_added, size_t *edges_added)
{
  if (!rm) return no_handle();
  if (vertices_added) *vertices_added = 0;
  if (edges_added) *edges_added = 0;
  { const int rc = commit_checks(rm->size, nbr_idx, edge_ok, n_states, max_states, new_joints, new_poses, Q, k, roots, n_roots, flags, new_index, mid_index, grow_state); if (rc != CCMP_OK) return rc; }
  if (states && goal_pose) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  const size_t S = Q * (size_t)k, sb = states ? S * (size_t)max_states * 14 * sizeof(double) : 0;
  StagedCall sg(ctx, __func__);
  const size_t off_i = sg.add(S * sizeof(int32_t)), off_ok = sg.add(S), off_n = sg.add(S * sizeof(int32_t)), off_st = sg.add(sb), off_j = sg.add(Q * 14 * sizeof(double)),
               off_p = sg.add(Q * 8 * sizeof(double)), off_v = sg.add(vertex_ok ? Q : 0), off_ni = sg.add(Q * sizeof(int32_t)), off_mi = sg.add(S * sizeof(int32_t)),
               off_gs = sg.add(Q * sizeof(int32_t));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_i, nbr_idx, S * sizeof(int32_t));
  sg.up(off_ok, edge_ok, S);
  sg.up(off_n, n_states, S * sizeof(int32_t));
  sg.up(off_st, states, sb);
  sg.up(off_j, new_joints, Q * 14 * sizeof(double));
  sg.up(off_p, new_poses, Q * 8 * sizeof(double));
  sg.up(off_v, vertex_ok, Q);
  int rc = CCMP_OK;
  if (sg.copy_ok()) // vertices_added and edges_added (zeroed above, before the checks) are the device form's to fill
    rc = ccmp_roadmap_commit(rm, p, sg.at<const int32_t>(off_i), sg.at<const uint8_t>(off_ok), sg.at<const int32_t>(off_n), sg.at<const double>(off_st, states),
                             max_states, sg.at<const double>(off_j), sg.at<const double>(off_p), sg.at<const uint8_t>(off_v, vertex_ok), Q, k, goal_pose, roots,
                             n_roots, flags, sg.at<int32_t>(off_ni), sg.at<int32_t>(off_mi), sg.at<int32_t>(off_gs), vertices_added, edges_added, ctx->stream);
  if (rc == CCMP_OK) {
    sg.down(new_index, off_ni, Q * sizeof(int32_t));
    sg.down(mid_index, off_mi, S * sizeof(int32_t));
    sg.down(grow_state, off_gs, Q * sizeof(int32_t));
  }
  return sg.finish(rc);
}

int ccmp_roadmap_add_edges_host(ccmp_roadmap *rm, const int32_t *uv, size_t E)
{
  if (!rm) return no_handle();
  if (E == 0) return CCMP_OK;
  if (!uv || E > kMaxRows || rm->n_edges > kMaxRows - E) return CCMP_EINVAL;
  for (size_t e = 0; e < E; e++)
    if (uv[2 * e] < 0 || uv[2 * e + 1] < 0 || (size_t)uv[2 * e] >= rm->size || (size_t)uv[2 * e + 1] >= rm->size || uv[2 * e] == uv[2 * e + 1]) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  StagedCall sg(ctx, __func__);
  const size_t off = sg.add(E * 2 * sizeof(int32_t));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off, uv, E * 2 * sizeof(int32_t));
  int rc = CCMP_OK;
  if (sg.copy_ok()) rc = ccmp_roadmap_add_edges(rm, sg.at<const int32_t>(off), E, nullptr, ctx->stream);
  return sg.finish(rc);
}

int ccmp_roadmap_read_edges_host(ccmp_roadmap *rm, size_t first, size_t count, int32_t *uv_out, double *w_out)
{
  if (!rm) return no_handle();
  if (first > rm->n_edges || count > rm->n_edges - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(rm->ctx, __func__);
  sg.down(uv_out, rm->uv + first * 2, count * 2 * sizeof(int32_t));
  sg.down(w_out, rm->w + first, count * sizeof(double));
  return sg.finish(CCMP_OK);
}

int ccmp_roadmap_read_labels_host(ccmp_roadmap *rm, size_t first, size_t count, int32_t *labels_out)
{
  if (!rm) return no_handle();
  if (first > rm->size || count > rm->size - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  if (!labels_out) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(rm->ctx, __func__);
  sg.down(labels_out, rm->labels + first, count * sizeof(int32_t));
  return sg.finish(CCMP_OK);
}

int ccmp_roadmap_closest_host(ccmp_roadmap *rm, const int32_t *from_idx, size_t F, const double *target_pose, int32_t *idx, double *dist,
                              double *from_dist)
{
  if (!rm) return no_handle();
  if (F == 0) return CCMP_OK;
  if (F > CCMP_CLOSEST_MAX_FROM || !from_idx || !target_pose || !idx || !dist || !from_dist) return CCMP_EINVAL;
  for (size_t f = 0; f < F; f++)
    if (from_idx[f] < 0 || (size_t)from_idx[f] >= rm->size) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  StagedCall sg(ctx, __func__);
  const size_t off_f = sg.add(F * sizeof(int32_t)), off_t = sg.add(8 * sizeof(double)), off_i = sg.add(F * sizeof(int32_t)), off_d = sg.add(F * sizeof(double)),
               off_fd = sg.add(F * sizeof(double));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_f, from_idx, F * sizeof(int32_t));
  sg.up(off_t, target_pose, 7 * sizeof(double)); // the target is 7 doubles, its piece a pose row of 8
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ccmp_roadmap_closest(rm, sg.at<const int32_t>(off_f), F, sg.at<const double>(off_t), sg.at<int32_t>(off_i), sg.at<double>(off_d), sg.at<double>(off_fd),
                              ctx->stream);
  if (rc == CCMP_OK) {
    sg.down(idx, off_i, F * sizeof(int32_t));
    sg.down(dist, off_d, F * sizeof(double));
    sg.down(from_dist, off_fd, F * sizeof(double));
  }
  return sg.finish(rc);
}

// ---- shortest paths: the planner's solution step (ccmp_path.h) ---------------------------------------------------------------------------
int ccmp_roadmap_shortest_paths(ccmp_roadmap *rm, const int32_t *src, const int32_t *dst, size_t F, int max_len, double *cost, int32_t *path_len,
                                int32_t *path, double *path_joints, double *path_poses, double *dist_out, int32_t *pred_out, void *hip_stream)
{
  if (!rm) return no_handle();
  if (F == 0) return CCMP_OK;
  { const int rc = path_checks(src, dst, F, max_len, cost, path_len, path); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t N = rm->size, n = F * N;
  { const int rc = grow_buffer(rm->ctx, &rm->path_ws, &rm->path_ws_cap, n + 1, kPathHeadBytes + n * (sizeof(double) + 3 * sizeof(int32_t))); if (rc != CCMP_OK) return rc; }
  rm->path_F = F;
  rm->path_N = N;
  ccmp_launch::GraphPath gp{};
  gp.src = src;
  gp.dst = dst;
  gp.F = (int)F;
  gp.rounds = (int32_t *)rm->path_ws;
  gp.d = path_d(rm);
  gp.hops = (int32_t *)(gp.d + n);
  gp.pred = gp.hops + n;
  gp.stamp = gp.pred + n;
  gp.max_len = max_len;
  gp.cost = cost;
  gp.path_len = path_len;
  gp.path = path;
  gp.path_joints = path_joints;
  gp.path_poses = path_poses;
  if (N == 0) HIP_TRY(hipMemsetAsync(gp.rounds, 0, kPathHeadBytes, st));
  HIP_TRY(ccmp_launch::graph_paths(graph_store(rm), gp, st));
  if (dist_out && n) HIP_TRY(hipMemcpyAsync(dist_out, gp.d, n * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (pred_out && n) HIP_TRY(hipMemcpyAsync(pred_out, gp.pred, n * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return CCMP_OK;
}

int ccmp_roadmap_path_rounds_host(ccmp_roadmap *rm, size_t F, int32_t *rounds)
{
  if (!rm) return no_handle();
  if (F == 0) return CCMP_OK;
  if (!rounds || !rm->path_ws || F > rm->path_F) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(rm->ctx, __func__);
  sg.down(rounds, rm->path_ws, F * 2 * sizeof(int32_t));
  return sg.finish(CCMP_OK);
}

int ccmp_roadmap_shortest_paths_host(ccmp_roadmap *rm, const int32_t *src, const int32_t *dst, size_t F, int max_len, double *cost, int32_t *path_len,
                                     int32_t *path, double *path_joints, double *path_poses, double *dist_out, int32_t *pred_out)
{
  if (!rm) return no_handle();
  if (F == 0) return CCMP_OK;
  { const int rc = path_checks(src, dst, F, max_len, cost, path_len, path); if (rc != CCMP_OK) return rc; }
  for (size_t f = 0; f < F; f++)
    if (src[f] < 0 || (size_t)src[f] >= rm->size || dst[f] < 0 || (size_t)dst[f] >= rm->size) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  const size_t L = (size_t)max_len;
  StagedCall sg(ctx, __func__);
  const size_t off_s = sg.add(F * sizeof(int32_t)), off_d = sg.add(F * sizeof(int32_t)), off_c = sg.add(F * sizeof(double)), off_l = sg.add(F * sizeof(int32_t)),
               off_p = sg.add(F * L * sizeof(int32_t)), off_j = sg.add(path_joints ? F * L * 14 * sizeof(double) : 0),
               off_o = sg.add(path_poses ? F * L * 8 * sizeof(double) : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_s, src, F * sizeof(int32_t));
  sg.up(off_d, dst, F * sizeof(int32_t));
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ccmp_roadmap_shortest_paths(rm, sg.at<const int32_t>(off_s), sg.at<const int32_t>(off_d), F, max_len, sg.at<double>(off_c), sg.at<int32_t>(off_l),
                                     sg.at<int32_t>(off_p), sg.at<double>(off_j, path_joints), sg.at<double>(off_o, path_poses), nullptr, nullptr, ctx->stream);
  // The download has two phases, each ended by a wait: the costs and lengths (and the distances and predecessors, straight from the
  // workspace), then of every path that fitted its entries alone, chosen by the lengths just read.  A path that did not fit leaves the
  // caller's arrays as they were.
  const size_t n = F * rm->size;
  if (rc == CCMP_OK) {
    sg.down(cost, off_c, F * sizeof(double));
    sg.down(path_len, off_l, F * sizeof(int32_t));
    sg.down(dist_out, path_d(rm), n * sizeof(double));
    sg.down(pred_out, path_pred(rm), n * sizeof(int32_t));
  }
  rc = sg.finish(rc);
  if (rc != CCMP_OK) return rc;
  for (size_t f = 0; f < F; f++) {
    const size_t len = path_len[f] > 0 && path_len[f] <= max_len ? (size_t)path_len[f] : 0;
    sg.down(path + f * L, off_p + f * L * sizeof(int32_t), len * sizeof(int32_t));
    if (path_joints) sg.down(path_joints + f * L * 14, off_j + f * L * 14 * sizeof(double), len * 14 * sizeof(double));
    if (path_poses) sg.down(path_poses + f * L * 8, off_o + f * L * 8 * sizeof(double), len * 8 * sizeof(double));
  }
  return sg.finish(CCMP_OK);
}

int ccmp_graph_shortest_paths_ref(const int32_t *uv, const double *w, size_t E, size_t N, const int32_t *src, const int32_t *dst, size_t F, int max_len,
                                  double *cost, int32_t *path_len, int32_t *path, double *dist_out, int32_t *pred_out)
{
  if (F == 0) return CCMP_OK;
  { const int rc = path_checks(src, dst, F, max_len, cost, path_len, path); if (rc != CCMP_OK) return rc; }
  if (N > kMaxRows || E > kMaxRows || (E > 0 && (!uv || !w))) return CCMP_EINVAL;
  for (size_t e = 0; e < E; e++) // what ccmp_roadmap_add_edges_host refuses
    if (uv[2 * e] < 0 || (size_t)uv[2 * e] >= N || uv[2 * e + 1] < 0 || (size_t)uv[2 * e + 1] >= N || uv[2 * e] == uv[2 * e + 1]) return CCMP_EINVAL;
  for (size_t f = 0; f < F; f++)
    if (src[f] < 0 || (size_t)src[f] >= N || dst[f] < 0 || (size_t)dst[f] >= N) return CCMP_EINVAL;
  try {
    // the adjacency: the half-edges of vertex v are adj[first[v] .. first[v + 1])
    std::vector<size_t> first(N + 1, 0);
    for (size_t e = 0; e < E; e++) { first[(size_t)uv[2 * e] + 1]++; first[(size_t)uv[2 * e + 1] + 1]++; }
    for (size_t v = 0; v < N; v++) first[v + 1] += first[v];
    std::vector<std::pair<int32_t, double>> adj(2 * E);
    {
      std::vector<size_t> at(first.begin(), first.end() - 1);
      for (size_t e = 0; e < E; e++) {
        adj[at[(size_t)uv[2 * e]]++] = {uv[2 * e + 1], w[e]};
        adj[at[(size_t)uv[2 * e + 1]]++] = {uv[2 * e], w[e]};
      }
    }
    std::vector<double> d(N);
    std::vector<int32_t> hops(N), pred(N), level, next;
    using Item = std::pair<double, int32_t>;
    for (size_t f = 0; f < F; f++) {
      const int32_t s = src[f], t = dst[f];
      // distances: heap Dijkstra with lazy deletion
      std::fill(d.begin(), d.end(), __builtin_inf());
      std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
      d[(size_t)s] = 0.0;
      heap.push({0.0, s});
      while (!heap.empty()) {
        const Item top = heap.top();
        heap.pop();
        const size_t u = (size_t)top.second;
        if (top.first != d[u]) continue;
        for (size_t h = first[u]; h < first[u + 1]; h++) {
          double c;
          const size_t v = (size_t)adj[h].first;
          if (ccmp::path_candidate(d[u], adj[h].second, &c) && c < d[v]) { d[v] = c; heap.push({c, (int32_t)v}); }
        }
      }
      // hops: breadth first over the tight edges
      std::fill(hops.begin(), hops.end(), ccmp::kPathNoHops);
      std::fill(pred.begin(), pred.end(), -1);
      hops[(size_t)s] = 0;
      level.assign(1, s);
      for (int32_t r = 1; !level.empty(); r++) {
        next.clear();
        for (const int32_t u : level)
          for (size_t h = first[(size_t)u]; h < first[(size_t)u + 1]; h++) {
            const size_t v = (size_t)adj[h].first;
            if (hops[v] == ccmp::kPathNoHops && ccmp::path_tight(d[(size_t)u], adj[h].second, d[v])) { hops[v] = r; next.push_back((int32_t)v); }
          }
        level.swap(next);
      }
      // predecessors: the smallest tree candidate
      for (size_t v = 0; v < N; v++)
        for (size_t h = first[v]; h < first[v + 1]; h++) {
          const int32_t u = adj[h].first;
          if (ccmp::path_parent(d[(size_t)u], hops[(size_t)u], adj[h].second, d[v], hops[v]) && (pred[v] < 0 || u < pred[v])) pred[v] = u;
        }
      cost[f] = d[(size_t)t];
      const int32_t len = hops[(size_t)t] == ccmp::kPathNoHops ? 0 : hops[(size_t)t] + 1;
      path_len[f] = len;
      if (len <= max_len) {
        int32_t v = t;
        for (int32_t i = len - 1; i >= 0 && v >= 0; i--) { path[f * (size_t)max_len + (size_t)i] = v; v = pred[(size_t)v]; }
      }
      if (dist_out) memcpy(dist_out + f * N, d.data(), N * sizeof(double));
      if (pred_out) memcpy(pred_out + f * N, pred.data(), N * sizeof(int32_t));
    }
  } catch (const std::bad_alloc &) {
    return CCMP_ENOMEM;
  }
  return CCMP_OK;
}

}  // extern "C"

// what the planner's loop (ccmp_plan.cpp; declared in ccmp_plan.h) needs of a store: its arrays as they stand, and its context
namespace ccmp_host {
void roadmap_arrays(const ccmp_roadmap *rm, ccmp_launch::GraphStore *out) { *out = graph_store(rm); }
ccmp_ctx *roadmap_ctx(const ccmp_roadmap *rm) { return rm->ctx; }
}  // namespace ccmp_host
