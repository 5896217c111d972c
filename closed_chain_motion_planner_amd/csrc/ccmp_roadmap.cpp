// ccmp_roadmap.cpp — the device-resident roadmap store of the C ABI (include/ccmp.h: ccmp_roadmap_*) and the two host functions of the
// object metric.  A store is two device arrays, joints [cap][14] and poses [cap][8], and a size kept on the host; appends, reads and
// queries are launches and copies on the caller's stream, so stream order is the order of the calls.  The arithmetic lives in
// ccmp_pose.h (metric, pose of a t_wo) and ccmp_kernels_knn.hip (the k-NN kernels of both metrics, pose_from_joints_kernel); the
// checks and the gather -> traversal -> fix chain behind ccmp_roadmap_connect are ccmp_connect_batch's own (ccmp_api.cpp:
// ccmp_host::connect_checks / connect_edges), as is the workspace rule (ccmp_host::grow_buffer).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_host.h"
#include "ccmp_ik.h"
#include "ccmp_launch.h"
#include "ccmp_policy.h"
#include "ccmp_pose.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"

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
};

namespace {

constexpr size_t kDefaultCapacity = 1024;
constexpr size_t kMaxNodes = ((size_t)1 << 31) - 1; // indices are int32

// what an entry point answers when it is given no store: a store needs a context and a context needs a device, so on a machine
// without one that is the reason (CCMP_ENODEV); with a device a NULL store is an argument error
int no_store()
{
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return CCMP_ENODEV; }
  return CCMP_EINVAL;
}

// Moves the store into a block of new_cap rows.  st != nullptr-able: the copy is ordered behind what `st` holds and `st` is waited
// for once before the old block goes; sync_device: the whole device is waited for first instead (ccmp_roadmap_reserve has no stream).
int regrow(ccmp_roadmap *rm, size_t new_cap, hipStream_t st, bool sync_device)
{
  if (new_cap > kMaxNodes) return CCMP_EINVAL;
  ccmp_host::quiesce(rm->ctx);
  if (sync_device) HIP_TRY(hipDeviceSynchronize());
  double *nj = nullptr, *np = nullptr;
  hipError_t e = hipMalloc((void **)&nj, new_cap * 14 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void **)&np, new_cap * 8 * sizeof(double));
  if (e == hipSuccess && rm->size) e = hipMemcpyAsync(nj, rm->joints, rm->size * 14 * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && rm->size) e = hipMemcpyAsync(np, rm->poses, rm->size * 8 * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    if (nj) (void)hipFree(nj);
    if (np) (void)hipFree(np);
    return e == hipErrorOutOfMemory ? CCMP_ENOMEM : hip_fail(e, "ccmp_roadmap: growth");
  }
  if (rm->joints) (void)hipFree(rm->joints);
  if (rm->poses) (void)hipFree(rm->poses);
  rm->joints = nj;
  rm->poses = np;
  rm->cap = new_cap;
  return CCMP_OK;
}

int knn_checks(const ccmp_roadmap *rm, int metric, const void *queries, size_t Q, int k, int mode, const int32_t *nbr_idx)
{
  if (!rm) return no_store();
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

// a host call's scratch on the device: the context's staging block, cut into 256-byte aligned pieces
struct Stage {
  ccmp_ctx *ctx;
  size_t total = 0;
  explicit Stage(ccmp_ctx *c) : ctx(c) {}
  size_t add(size_t bytes) { const size_t off = total; total = (total + bytes + 255) & ~(size_t)255; return off; }
  int alloc() { return ensure_stage(ctx, total ? total : 256); }
  char *at(size_t off) const { return (char *)ctx->stage + off; }
};

}  // namespace

extern "C" {

double ccmp_pose_distance(const double a[8], const double b[8]) { return ccmp_pose_dist(a, b); }
void ccmp_pose_from_t_wo(const double t_wo[12], double pose[8]) { ccmp_pose_of_t_wo(t_wo, pose); }

ccmp_roadmap *ccmp_roadmap_create(ccmp_ctx *ctx, size_t capacity_hint)
{
  if (!ctx || capacity_hint > kMaxNodes) return nullptr;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return nullptr;
  ccmp_roadmap *rm = new (std::nothrow) ccmp_roadmap();
  if (!rm) return nullptr;
  rm->ctx = ctx;
  rm->device = ctx->device;
  if (regrow(rm, capacity_hint ? capacity_hint : kDefaultCapacity, ctx->stream, false) != CCMP_OK) { delete rm; return nullptr; }
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
  }
  delete rm;
}

size_t ccmp_roadmap_size(const ccmp_roadmap *rm) { return rm ? rm->size : 0; }

int ccmp_roadmap_reserve(ccmp_roadmap *rm, size_t n)
{
  if (!rm) return no_store();
  if (n > kMaxNodes) return CCMP_EINVAL;
  if (n <= rm->cap) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  return regrow(rm, n, rm->ctx->stream, true);
}

int ccmp_roadmap_append(ccmp_roadmap *rm, const ccmp_problem *p, const double *joints, const double *poses, size_t Q, size_t *first_index,
                        void *hip_stream)
{
  if (!rm) return no_store();
  if (first_index) *first_index = rm->size;
  if (Q == 0) return CCMP_OK;
  if ((!joints && !poses) || Q > kMaxNodes - rm->size) return CCMP_EINVAL;
  if (!poses) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; } // the poses are derived from the joints and the problem
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t need = rm->size + Q;
  if (need > rm->cap) {
    const int rc = regrow(rm, need > 2 * rm->cap ? need : 2 * rm->cap > kMaxNodes ? kMaxNodes : 2 * rm->cap, st, false);
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
  rm->size = need;
  return CCMP_OK;
}

int ccmp_roadmap_set_joints(ccmp_roadmap *rm, size_t index, const double *joints, void *hip_stream)
{
  if (!rm) return no_store();
  if (!joints || index >= rm->size) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  HIP_TRY(hipMemcpyAsync(rm->joints + index * 14, joints, 14 * sizeof(double), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
  return CCMP_OK;
}

int ccmp_roadmap_truncate(ccmp_roadmap *rm, size_t n)
{
  if (!rm) return no_store();
  if (n > rm->size) return CCMP_EINVAL;
  rm->size = n;
  return CCMP_OK;
}

int ccmp_roadmap_read(ccmp_roadmap *rm, size_t first, size_t count, double *joints_out, double *poses_out, void *hip_stream)
{
  if (!rm) return no_store();
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
int ccmp_roadmap_grow(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts, const double *query_poses,
                      size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index, int check_target, int max_states,
                      int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok, int32_t *ik_which, double *states,
                      int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out, void *hip_stream)
{
  { const int rc = knn_checks(rm, CCMP_METRIC_OBJECT, query_poses, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  ccmp_ctx *ctx = rm->ctx;
  if (!p || k > CCMP_IK_MAX_SEEDS) return CCMP_EINVAL;
  ccmp::ik_params P;
  { const int rc = ik_checks(p, opts, Q, k, &P); if (rc != CCMP_OK) return rc; }
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
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
  { const int rc = ik_reserve(ctx, ik_candidates(Q, k, P)); if (rc != CCMP_OK) return rc; }
  double *seeds = (double *)rm->grow_ws, *q_trav = seeds + E * 14; // Q <= E rows
  int32_t *masked = (int32_t *)(seeds + E * 28);
  { const int rc = knn_object(rm, query_poses, Q, k, mode, self_base, nbr_idx, nbr_dist, st); if (rc != CCMP_OK) return rc; }
  HIP_TRY(ccmp_launch::ik_gather_seeds(rm->joints, nbr_idx, E, seeds, st));
  { const int rc = ik_launches(ctx, p, P, query_poses, seeds, Q, k, rng_seed, first_index, q_new, ik_ok, ik_which, nullptr, nullptr, st); if (rc != CCMP_OK) return rc; }
  HIP_TRY(ccmp_launch::ik_grow_prepare(rm->joints, nbr_idx, ik_ok, q_new, Q, k, masked, q_trav, st));
  return connect_edges(ctx, p, scene, margin, rm->joints, q_trav, Q, k, check_target, max_states, round_budget, masked, states, n_states, ok, newton_iters,
                       blocked, carry_out, hip_stream);
}

// the host form of set_joints (growTree hands over the result of its IK): synchronous on the context's stream
int ccmp_roadmap_set_joints_host(ccmp_roadmap *rm, size_t index, const double *joints)
{
  if (!rm) return no_store();
  if (!joints || index >= rm->size) return CCMP_EINVAL;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = rm->ctx->stream;
  const hipError_t e = hipMemcpyAsync(rm->joints + index * 14, joints, 14 * sizeof(double), hipMemcpyHostToDevice, st);
  const hipError_t es = hipStreamSynchronize(st);
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
}

// ---- host forms: synchronous on the context's stream; only the new rows / the queries go up ---------------------------------------
int ccmp_roadmap_append_host(ccmp_roadmap *rm, const ccmp_problem *p, const double *joints, const double *poses, size_t Q, size_t *first_index)
{
  if (!rm) return no_store();
  if (first_index) *first_index = rm->size;
  if (Q == 0) return CCMP_OK;
  if ((!joints && !poses) || Q > kMaxNodes - rm->size) return CCMP_EINVAL;
  if (!poses) { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  Stage sg(ctx);
  const size_t jb = Q * 14 * sizeof(double), pb = Q * 8 * sizeof(double);
  const size_t off_j = sg.add(joints ? jb : 0), off_p = sg.add(poses ? pb : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  if (joints) HIP_TRY(hipMemcpyAsync(sg.at(off_j), joints, jb, hipMemcpyHostToDevice, ctx->stream));
  if (poses) HIP_TRY(hipMemcpyAsync(sg.at(off_p), poses, pb, hipMemcpyHostToDevice, ctx->stream));
  const int rc = ccmp_roadmap_append(rm, p, joints ? (const double *)sg.at(off_j) : nullptr, poses ? (const double *)sg.at(off_p) : nullptr, Q, first_index,
                                     ctx->stream);
  const hipError_t e = hipStreamSynchronize(ctx->stream); // also on the error path: the staging block must be quiet
  if (rc != CCMP_OK) return rc;
  HIP_TRY(e);
  return CCMP_OK;
}

int ccmp_roadmap_read_host(ccmp_roadmap *rm, size_t first, size_t count, double *joints_out, double *poses_out)
{
  if (!rm) return no_store();
  if (first > rm->size || count > rm->size - first) return CCMP_EINVAL;
  if (count == 0) return CCMP_OK;
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = rm->ctx->stream;
  hipError_t e = hipSuccess;
  if (joints_out) e = hipMemcpyAsync(joints_out, rm->joints + first * 14, count * 14 * sizeof(double), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess && poses_out) e = hipMemcpyAsync(poses_out, rm->poses + first * 8, count * 8 * sizeof(double), hipMemcpyDeviceToHost, st);
  const hipError_t es = hipStreamSynchronize(st);
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
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
  Stage sg(ctx);
  const size_t off_q = sg.add(qb);
  const size_t off_d = sg.total; // distances then indices, one block: one download
  sg.add(S * sizeof(double) + S * sizeof(int32_t));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  HIP_TRY(hipMemcpyAsync(sg.at(off_q), queries, qb, hipMemcpyHostToDevice, ctx->stream));
  double *d_dev = (double *)sg.at(off_d);
  int32_t *i_dev = (int32_t *)(d_dev + S);
  int rc = ccmp_roadmap_knn(rm, metric, (const double *)sg.at(off_q), Q, k, mode, self_base, i_dev, nbr_dist ? d_dev : nullptr, ctx->stream);
  hipError_t e = hipSuccess;
  std::vector<char> back;
  if (rc == CCMP_OK) {
    if (nbr_dist) {
      try { back.resize(S * (sizeof(double) + sizeof(int32_t))); } catch (...) { rc = CCMP_ENOMEM; }
      if (rc == CCMP_OK) e = hipMemcpyAsync(back.data(), d_dev, back.size(), hipMemcpyDeviceToHost, ctx->stream);
    } else e = hipMemcpyAsync(nbr_idx, i_dev, S * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
  }
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(e);
  HIP_TRY(es);
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
  hipStream_t st = ctx->stream;
  const size_t E = Q * (size_t)k, jb = Q * 14 * sizeof(double), pb = Q * 8 * sizeof(double), sb = E * (size_t)max_states * 14 * sizeof(double);
  Stage sg(ctx);
  const size_t off_j = sg.add(jb), off_p = sg.add(query_poses ? pb : 0), off_i = sg.add(E * sizeof(int32_t)), off_d = sg.add(E * sizeof(double)),
               off_st = sg.add(sb), off_n = sg.add(E * sizeof(int32_t)), off_ok = sg.add(E), off_it = sg.add(E * sizeof(int32_t)), off_bl = sg.add(E),
               off_co = sg.add(E * 2 * sizeof(double));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  HIP_TRY(hipMemcpyAsync(sg.at(off_j), query_joints, jb, hipMemcpyHostToDevice, st));
  if (query_poses) HIP_TRY(hipMemcpyAsync(sg.at(off_p), query_poses, pb, hipMemcpyHostToDevice, st));
  const int rc = ccmp_roadmap_connect(rm, p, scene, margin, metric, (const double *)sg.at(off_j), query_poses ? (const double *)sg.at(off_p) : nullptr, Q, k,
                                      mode, self_base, check_target, max_states, round_budget, (int32_t *)sg.at(off_i),
                                      nbr_dist ? (double *)sg.at(off_d) : nullptr, (double *)sg.at(off_st), (int32_t *)sg.at(off_n), (uint8_t *)sg.at(off_ok),
                                      newton_iters ? (int32_t *)sg.at(off_it) : nullptr, blocked ? (uint8_t *)sg.at(off_bl) : nullptr,
                                      carry_out ? (double *)sg.at(off_co) : nullptr, st);
  hipError_t e = hipSuccess;
  auto down = [&](void *dst, size_t off, size_t n) { if (dst && e == hipSuccess) e = hipMemcpyAsync(dst, sg.at(off), n, hipMemcpyDeviceToHost, st); };
  if (rc == CCMP_OK) {
    down(nbr_idx, off_i, E * sizeof(int32_t));
    down(nbr_dist, off_d, E * sizeof(double));
    down(states, off_st, sb);
    down(n_states, off_n, E * sizeof(int32_t));
    down(ok, off_ok, E);
    down(newton_iters, off_it, E * sizeof(int32_t));
    down(blocked, off_bl, E);
    down(carry_out, off_co, E * 2 * sizeof(double));
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
}

int ccmp_roadmap_grow_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                           const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index,
                           int check_target, int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok,
                           int32_t *ik_which, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out)
{
  { const int rc = knn_checks(rm, CCMP_METRIC_OBJECT, query_poses, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (!p || k > CCMP_IK_MAX_SEEDS) return CCMP_EINVAL;
  { ccmp::ik_params P; const int rc = ik_checks(p, opts, Q, k, &P); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  if (!q_new || !ik_ok || !ik_which) return CCMP_EINVAL;
  { const int rc = connect_checks(rm->ctx, p, scene, margin, max_states, states, n_states, ok, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; } // before any buffer is touched
  DeviceGuard guard(rm->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = rm->ctx;
  hipStream_t st = ctx->stream;
  const size_t E = Q * (size_t)k, pb = Q * 8 * sizeof(double), sb = E * (size_t)max_states * 14 * sizeof(double);
  Stage sg(ctx);
  const size_t off_p = sg.add(pb), off_i = sg.add(E * sizeof(int32_t)), off_d = sg.add(E * sizeof(double)), off_q = sg.add(Q * 14 * sizeof(double)),
               off_io = sg.add(Q), off_iw = sg.add(Q * sizeof(int32_t)), off_st = sg.add(sb), off_n = sg.add(E * sizeof(int32_t)), off_ok = sg.add(E),
               off_it = sg.add(E * sizeof(int32_t)), off_bl = sg.add(E), off_co = sg.add(E * 2 * sizeof(double));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  HIP_TRY(hipMemcpyAsync(sg.at(off_p), query_poses, pb, hipMemcpyHostToDevice, st));
  const int rc = ccmp_roadmap_grow(rm, p, scene, margin, opts, (const double *)sg.at(off_p), Q, k, mode, self_base, rng_seed, first_index, check_target, max_states,
                                   round_budget, (int32_t *)sg.at(off_i), nbr_dist ? (double *)sg.at(off_d) : nullptr, (double *)sg.at(off_q),
                                   (uint8_t *)sg.at(off_io), (int32_t *)sg.at(off_iw), (double *)sg.at(off_st), (int32_t *)sg.at(off_n), (uint8_t *)sg.at(off_ok),
                                   newton_iters ? (int32_t *)sg.at(off_it) : nullptr, blocked ? (uint8_t *)sg.at(off_bl) : nullptr,
                                   carry_out ? (double *)sg.at(off_co) : nullptr, st);
  hipError_t e = hipSuccess;
  auto down = [&](void *dst, size_t off, size_t n) { if (dst && e == hipSuccess) e = hipMemcpyAsync(dst, sg.at(off), n, hipMemcpyDeviceToHost, st); };
  if (rc == CCMP_OK) {
    down(nbr_idx, off_i, E * sizeof(int32_t));
    down(nbr_dist, off_d, E * sizeof(double));
    down(q_new, off_q, Q * 14 * sizeof(double));
    down(ik_ok, off_io, Q);
    down(ik_which, off_iw, Q * sizeof(int32_t));
    down(states, off_st, sb);
    down(n_states, off_n, E * sizeof(int32_t));
    down(ok, off_ok, E);
    down(newton_iters, off_it, E * sizeof(int32_t));
    down(blocked, off_bl, E);
    down(carry_out, off_co, E * 2 * sizeof(double));
  }
  const hipError_t es = hipStreamSynchronize(st);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
}

}  // extern "C"
