// ccmp_rrtc.cpp — RRT-Connect on the roadmap store in the C ABI (include/ccmp.h: ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree): the
// reference's other planner as one resumable handle, a sibling of ccmp_plan.  The handle owns a state block on the device
// (ccmp_rrtc_state) and one block of call buffers sized at creation for `width` samples; a cycle is the sequence of include/ccmp.h over
// the library's own entry points (ccmp_sample_project_batch, ccmp_joint_valid_batch, ccmp_clearance_batch, ccmp_geodesic_batch_ex /
// ccmp_geodesic_scene_batch, ccmp_roadmap_append, ccmp_roadmap_add_edges) on the context's stream, with the kernels of
// ccmp_kernels_rrtc.hip between them: the samples, the lists and the picks never cross to the host.  What the host reads per cycle: the
// commit kernel's 16 bytes of counts, add_edges' own read-back and the state block once at the end.  The state block's reads, open's
// upload, the run loop with its solution test and the head of the report are ccmp_planner.h's, shared with ccmp_plan.cpp; the handle and
// the list of its arrays are there too.  The *_ref forms at the end compile the rule text of ccmp_rrtc.h (the solution test:
// ccmp_plan.h) for the host.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_graph.h"
#include "ccmp_launch.h"
#include "ccmp_plan.h"
#include "ccmp_planner.h"
#include "ccmp_policy.h"
#include "ccmp_resident.h"
#include "ccmp_rrtc.h"
#include "ccmp_scene.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

// the layouts the Python binding restates (closed_chain_motion_planner_amd/_lib.py)
static_assert(sizeof(ccmp_rrtc_opts) == 32 && sizeof(ccmp_rrtc_counters) == 48 && sizeof(ccmp_rrtc_state) == 160 && sizeof(ccmp_rrtc_report) == 104,
              "ccmp_rrtc_* layout");

namespace {

// what every form of a nearest-in-tree call checks first
int nearest_checks(int n_roots, const int32_t *roots, const double *queries, size_t Q, const int32_t *idx, const double *dist)
{
  if (n_roots < 0 || n_roots > CCMP_RRTC_MAX_ROOTS || Q >= ((size_t)1 << 31)) return CCMP_EINVAL;
  if ((n_roots > 0 && !roots) || (Q > 0 && (!queries || !idx || !dist))) return CCMP_EINVAL;
  return CCMP_OK;
}

// the launches of a checked call (Q > 0, the device current)
int nearest_launch(ccmp_roadmap *rm, const int32_t *roots, int n_roots, const double *queries, size_t Q, int32_t *idx, double *dist, hipStream_t st)
{
  ccmp_ctx *ctx = roadmap_ctx(rm);
  ccmp_launch::GraphStore gs;
  roadmap_arrays(rm, &gs);
  unsigned int part, partitions;
  plan_rrtc_nearest(ctx, Q, gs.N, &part, &partitions);
  const size_t cells = partitions > 1 ? Q * (size_t)partitions : 0, bytes = cells * (sizeof(double) + sizeof(int32_t));
  { const int rc = grow_buffer(ctx, &ctx->knn_ws, &ctx->knn_ws_cap, bytes, bytes); if (rc != CCMP_OK) return rc; }
  double *ws_d = (double *)ctx->knn_ws;
  int32_t *ws_i = (int32_t *)(ws_d + cells);
  HIP_TRY(ccmp_launch::rrtc_nearest(gs, roots, n_roots, queries, Q, part, partitions, ws_d, ws_i, idx, dist, st));
  return CCMP_OK;
}

// one traversal per row: from [W] -> to [W] into the handle's lists
int traverse(ccmp_rrtc *pl)
{
  const size_t W = (size_t)pl->o.width;
  hipStream_t st = pl->ctx->stream;
  if (pl->scene)
    return ccmp_geodesic_scene_batch(pl->ctx, &pl->p, pl->scene, pl->margin, pl->from, pl->to, W, pl->o.max_states, pl->states, pl->n_states, pl->ok, pl->iters,
                                     pl->blocked, nullptr, nullptr, pl->carry, pl->o.round_budget, 0, st);
  return ccmp_geodesic_batch_ex(pl->ctx, &pl->p, pl->from, pl->to, W, pl->o.max_states, pl->states, pl->n_states, pl->ok, pl->iters, nullptr, pl->carry,
                                pl->o.round_budget, 0, st);
}

// steps 1 to 4 of a cycle; step 5, the solution test, is the run loop's
int cycle(ccmp_rrtc *pl)
{
  hipStream_t st = pl->ctx->stream;
  const ccmp_rrtc_opts &o = pl->o;
  const ccmp_rrtc_state &h = pl->host;
  const size_t W = (size_t)o.width;
  const bool a_is_start = (h.cycle & 1) == 0;
  int32_t *d_starts = dev_starts(pl->state), *d_goals = dev_goals(pl->state);
  const int32_t *rootsA = a_is_start ? d_starts : d_goals, *rootsB = a_is_start ? d_goals : d_starts;
  const int nA = a_is_start ? h.n_starts : h.n_goals, nB = a_is_start ? h.n_goals : h.n_starts;
  // 1. samples
  int rc = ccmp_sample_project_batch(pl->ctx, &pl->p, pl->seed, h.next_index, pl->samples, pl->s_ok, nullptr, nullptr, W, st);
  if (rc != CCMP_OK) return rc;
  if ((rc = ccmp_joint_valid_batch(pl->ctx, &pl->p, pl->samples, pl->jv, W, st)) != CCMP_OK) return rc;
  if (pl->scene && (rc = ccmp_clearance_batch(pl->ctx, &pl->p, pl->scene, pl->samples, nullptr, W, pl->margin, pl->clear, nullptr, pl->free_, st)) != CCMP_OK)
    return rc;
  // 2. extension of tree A
  ccmp_launch::GraphStore gs;
  roadmap_arrays(pl->rm, &gs);
  if ((rc = nearest_launch(pl->rm, rootsA, nA, pl->samples, W, pl->idxA, pl->dist, st)) != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::rrtc_edges(gs, pl->idxA, pl->samples, pl->s_ok, pl->jv, pl->scene ? pl->free_ : nullptr, W, pl->from, pl->to, pl->use, st));
  if ((rc = traverse(pl)) != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::rrtc_pick(ccmp_launch::RrtcPick{0, pl->states, pl->n_states, pl->ok, pl->use, pl->samples, pl->dist, pl->idxA, W, o.max_states, o.range,
                                                        pl->outA, pl->rixA, pl->rowA, pl->parA, pl->madeA, nullptr},
                                 st));
  // 3. connection from tree B (the store is as at cycle entry: nothing is committed yet)
  if ((rc = nearest_launch(pl->rm, rootsB, nB, pl->rowA, W, pl->idxB, pl->dist, st)) != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::rrtc_edges(gs, pl->idxB, pl->rowA, pl->madeA, nullptr, nullptr, W, pl->from, pl->to, pl->jv, st)); // (jv is free again: step 3's use)
  if ((rc = traverse(pl)) != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::rrtc_pick(ccmp_launch::RrtcPick{1, pl->states, pl->n_states, pl->ok, pl->jv, pl->rowA, nullptr, pl->idxB, W, o.max_states, o.range,
                                                        pl->outB, pl->rixB, pl->rowB, pl->parB, nullptr, pl->gapB},
                                 st));
  // 4. commit
  HIP_TRY(ccmp_launch::rrtc_commit(gs, pl->state,
                                   ccmp_launch::RrtcCommit{o.width, a_is_start ? 1 : 0, pl->use, pl->outA, pl->parA, pl->rowA, pl->outB, pl->parB, pl->idxB,
                                                           pl->rowB, pl->gapB, pl->rows, pl->uv, pl->counts},
                                   st));
  int32_t cnt[4] = {0, 0, 0, 0};
  if ((rc = read_back(cnt, pl->counts, sizeof cnt, st)) != CCMP_OK) return rc;
  if (cnt[0] < 0 || (size_t)cnt[0] > 2 * W || cnt[1] < 0 || (size_t)cnt[1] > 2 * W) return CCMP_EINVAL; // (cannot happen: the kernel counts flags)
  if ((rc = ccmp_roadmap_append(pl->rm, &pl->p, pl->rows, nullptr, (size_t)cnt[0], nullptr, st)) != CCMP_OK) return rc;
  if (cnt[1] > 0 && (rc = ccmp_roadmap_add_edges(pl->rm, pl->uv, 2 * W, nullptr, st)) != CCMP_OK) return rc;
  return CCMP_OK;
}

struct RrtcLoop {
  static bool terminal(int status) { return status == CCMP_RRTC_SOLVED; }
  static bool full(const ccmp_rrtc *pl) { return ccmp::rrtc_full(ccmp_roadmap_size(pl->rm), pl->o.width, pl->o.max_vertices); }
  static int cycle(ccmp_rrtc *pl) { return ::cycle(pl); }
  static void report(const ccmp_rrtc *pl, int cycles_run, ccmp_rrtc_report *out)
  {
    if (!report_head(pl, cycles_run, out)) return;
    const ccmp_rrtc_state &s = pl->host;
    out->best_a = s.best_a;
    out->best_b = s.best_b;
    out->best_gap = s.best_gap;
    out->counters = s.counters;
  }
};

int opts_ok(const ccmp_rrtc_opts *o)
{
  if (o->width < 1 || o->width > CCMP_PLAN_MAX_WIDTH || o->width > ccmp_launch::kRrtcThreads || o->max_states < 2 || o->round_budget < 0) return CCMP_EINVAL;
  if (!std::isfinite(o->range) || !(o->range > 0.0) || o->max_vertices > (uint64_t)INT32_MAX) return CCMP_EINVAL;
  return CCMP_OK;
}

}  // namespace

extern "C" {

void ccmp_rrtc_default_opts(ccmp_rrtc_opts *o)
{
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->width = 32;
  o->max_states = 64;
  o->round_budget = 0;
  o->range = 0.1;
  o->max_vertices = (uint64_t)INT32_MAX;
}

int ccmp_rrtc_create(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_rrtc_opts *opts, const int32_t *starts,
                     int n_starts, const int32_t *goals, int n_goals, uint64_t rng_seed, uint64_t first_index, ccmp_rrtc **out)
{
  if (out) *out = nullptr;
  if (!rm) return no_handle();
  if (!p || !opts || !starts || !goals || !out) return CCMP_EINVAL;
  { const int rc = opts_ok(opts); if (rc != CCMP_OK) return rc; }
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (n_starts < 1 || n_starts > CCMP_PLAN_MAX_STARTS || n_goals < 1 || n_goals > CCMP_PLAN_MAX_GOALS) return CCMP_EINVAL;
  const size_t size0 = ccmp_roadmap_size(rm);
  for (int i = 0; i < n_starts; i++)
    if (starts[i] < 0 || (size_t)starts[i] >= size0) return CCMP_EINVAL;
  for (int i = 0; i < n_goals; i++)
    if (goals[i] < 0 || (size_t)goals[i] >= size0) return CCMP_EINVAL;
  ccmp_ctx *ctx = roadmap_ctx(rm);
  if (std::isnan(margin)) return CCMP_EINVAL;
  if (scene && scene->device != ctx->device) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_rrtc *pl = new (std::nothrow) ccmp_rrtc();
  if (!pl) return CCMP_ENOMEM;
  pl->rm = rm;
  pl->p = *p;
  pl->scene = scene;
  pl->margin = scene ? margin : 0.0;
  pl->o = *opts;
  pl->seed = rng_seed;
  ResultBlock rb; // the one block: ccmp_planner.h's list
  { const int rc = rb.alloc_pieces(pl, ctx, __func__); if (rc != CCMP_OK) { delete pl; return rc; } }

  ccmp_rrtc_state &h = pl->host;
  memset(&h, 0, sizeof h);
  h.n_starts = n_starts;
  h.n_goals = n_goals;
  for (int i = 0; i < CCMP_PLAN_MAX_STARTS; i++) h.starts[i] = i < n_starts ? starts[i] : -1;
  for (int i = 0; i < CCMP_PLAN_MAX_GOALS; i++) h.goals[i] = i < n_goals ? goals[i] : -1;
  h.status = CCMP_RRTC_OPEN;
  h.next_index = first_index;
  h.solved_start = h.solved_goal = h.best_a = h.best_b = -1;
  h.best_gap = __builtin_inf();
  auto fail = [&](int code) { ccmp_rrtc_destroy(pl); return code; };
  { const int rc = planner_upload(pl, {}, __func__); if (rc != CCMP_OK) return fail(rc); }
  { const int rc = solution_test(pl, 0); if (rc != CCMP_OK) return fail(rc); }
  *out = pl;
  return CCMP_OK;
}

int ccmp_rrtc_run(ccmp_rrtc *pl, int max_cycles, ccmp_rrtc_report *out) { return planner_run<RrtcLoop>(pl, max_cycles, out); }

int ccmp_rrtc_state_read(ccmp_rrtc *pl, ccmp_rrtc_state *out) { return planner_state_read(pl, out); }

void ccmp_rrtc_destroy(ccmp_rrtc *pl) { result_destroy(pl); }

int ccmp_roadmap_nearest_in_tree(ccmp_roadmap *rm, const int32_t *roots, int n_roots, const double *queries, size_t Q, int32_t *idx, double *dist,
                                 void *hip_stream)
{
  if (!rm) return no_handle();
  { const int rc = nearest_checks(n_roots, roots, queries, Q, idx, dist); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  DeviceGuard guard(ccmp_ctx_device(roadmap_ctx(rm)));
  if (!guard.ok) return CCMP_ENODEV;
  return nearest_launch(rm, roots, n_roots, queries, Q, idx, dist, (hipStream_t)hip_stream);
}

int ccmp_roadmap_nearest_in_tree_host(ccmp_roadmap *rm, const int32_t *roots, int n_roots, const double *queries, size_t Q, int32_t *idx, double *dist)
{
  if (!rm) return no_handle();
  { const int rc = nearest_checks(n_roots, roots, queries, Q, idx, dist); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  const size_t size = ccmp_roadmap_size(rm);
  for (int i = 0; i < n_roots; i++)
    if (roots[i] < 0 || (size_t)roots[i] >= size) return CCMP_EINVAL;
  ccmp_ctx *ctx = roadmap_ctx(rm);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(ctx, __func__);
  const size_t off_r = sg.add(CCMP_RRTC_MAX_ROOTS * sizeof(int32_t)), off_q = sg.add(Q * 14 * sizeof(double)), off_i = sg.add(Q * sizeof(int32_t)),
               off_d = sg.add(Q * sizeof(double));
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_r, roots, (size_t)n_roots * sizeof(int32_t));
  sg.up(off_q, queries, Q * 14 * sizeof(double));
  int rc = CCMP_OK;
  if (sg.copy_ok()) rc = nearest_launch(rm, sg.at<const int32_t>(off_r), n_roots, sg.at<const double>(off_q), Q, sg.at<int32_t>(off_i), sg.at<double>(off_d), ctx->stream);
  if (rc == CCMP_OK) {
    sg.down(idx, off_i, Q * sizeof(int32_t));
    sg.down(dist, off_d, Q * sizeof(double));
  }
  return sg.finish(rc);
}

int ccmp_roadmap_nearest_in_tree_ref(const double *store_joints, const int32_t *labels, size_t N, const int32_t *roots, int n_roots, const double *queries,
                                     size_t Q, int32_t *idx, double *dist)
{
  { const int rc = nearest_checks(n_roots, roots, queries, Q, idx, dist); if (rc != CCMP_OK) return rc; }
  if (N > kMaxRows || (N > 0 && (!store_joints || !labels))) return CCMP_EINVAL;
  for (int i = 0; i < n_roots; i++)
    if (roots[i] < 0 || (size_t)roots[i] >= N) return CCMP_EINVAL;
  int32_t lab[CCMP_RRTC_MAX_ROOTS];
  const int nl = ccmp::rrtc_root_labels(roots, n_roots, labels, N, lab);
  for (size_t q = 0; q < Q; q++) {
    double bd = __builtin_inf();
    int32_t bi = 0x7fffffff;
    for (size_t j = 0; nl > 0 && j < N; j++) {
      if (!ccmp::rrtc_in_tree(labels[j], lab)) continue;
      const double d = ccmp::graph_joint_dist(store_joints + j * 14, queries + q * 14);
      if (ccmp::graph_closer(d, (int32_t)j, bd, bi)) { bd = d; bi = (int32_t)j; }
    }
    idx[q] = bi == 0x7fffffff ? -1 : bi;
    dist[q] = bd;
  }
  return CCMP_OK;
}

int ccmp_rrtc_nearest_shape(const ccmp_ctx *ctx, size_t Q, size_t N, unsigned int *part, unsigned int *partitions)
{
  if (!part || !partitions || Q >= ((size_t)1 << 31) || N > kMaxRows) return CCMP_EINVAL;
  plan_rrtc_nearest(ctx ? ctx : &default_ctx(), Q, N, part, partitions);
  return CCMP_OK;
}

int ccmp_rrtc_pick_ref(int mode, const double *states, const int32_t *n_states, const uint8_t *ok, const uint8_t *use, const double *to, const double *d,
                       size_t E, int max_states, double range, int32_t *outcome, int32_t *row_index, double *row, double *gap)
{
  if ((mode != 0 && mode != 1) || max_states < 1 || E > kMaxRows) return CCMP_EINVAL;
  if (E == 0) return CCMP_OK;
  if (!states || !n_states || !ok || !to || !outcome || !row_index || !row || (mode == 0 && !d)) return CCMP_EINVAL;
  for (size_t e = 0; e < E; e++) {
    const uint8_t u = use ? use[e] : 1;
    const int32_t ns = n_states[e];
    const int m = u != 1 ? 0 : ns < 0 ? 0 : ns > max_states ? max_states : ns;
    const double *st = states + e * (size_t)max_states * 14, *tgt = to + e * 14;
    int32_t o, r = -1;
    double g = __builtin_nan("");
    if (mode == 0) {
      ccmp::rrtc_arc a;
      ccmp::rrtc_arc_begin(&a);
      for (int i = 1; i < m; i++) ccmp::rrtc_arc_step(&a, i, ccmp::graph_joint_dist(st + (size_t)(i - 1) * 14, st + (size_t)i * 14), range);
      o = u == 0 ? CCMP_RRTC_NONE : ccmp::rrtc_extend(m > 0 ? ns : 0, max_states, ok[e], d[e], range, &a, &r);
    } else {
      if (m > 0) g = ccmp::graph_joint_dist(st + (size_t)(m - 1) * 14, tgt);
      o = u == 0 ? CCMP_RRTC_NONE : ccmp::rrtc_connect(m > 0 ? ns : 0, max_states, ok[e], g, &r);
    }
    const bool reached = mode == 0 && o == CCMP_RRTC_REACHED;
    for (int c = 0; c < 14; c++) row[e * 14 + c] = reached ? tgt[c] : (r >= 0 && r < m) ? st[(size_t)r * 14 + c] : 0.0;
    outcome[e] = o;
    row_index[e] = r;
    if (gap) gap[e] = g;
  }
  return CCMP_OK;
}

int ccmp_rrtc_pick_batch(ccmp_ctx *ctx, int mode, const double *states, const int32_t *n_states, const uint8_t *ok, const uint8_t *use, const double *to,
                         const double *d, size_t E, int max_states, double range, int32_t *outcome, int32_t *row_index, double *row, double *gap,
                         void *hip_stream)
{
  if (!ctx) return no_handle();
  if ((mode != 0 && mode != 1) || max_states < 1 || E > kMaxRows) return CCMP_EINVAL;
  if (E == 0) return CCMP_OK;
  if (!states || !n_states || !ok || !to || !outcome || !row_index || !row || (mode == 0 && !d)) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  HIP_TRY(ccmp_launch::rrtc_pick(ccmp_launch::RrtcPick{mode, states, n_states, ok, use, to, d, nullptr, E, max_states, range, outcome, row_index, row, nullptr,
                                                        nullptr, gap},
                                 (hipStream_t)hip_stream));
  return CCMP_OK;
}

int ccmp_rrtc_connected_ref(const int32_t *labels, size_t N, ccmp_rrtc_state *state)
{
  if (!state || (N > 0 && !labels) || state->n_starts < 0 || state->n_starts > CCMP_PLAN_MAX_STARTS || state->n_goals < 0 ||
      state->n_goals > CCMP_PLAN_MAX_GOALS)
    return CCMP_EINVAL;
  ccmp::first_connected(state, labels, N);
  return CCMP_OK;
}

}  // extern "C"
