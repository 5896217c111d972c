// ccmp_plan.cpp — the planner's loop on the roadmap store in the C ABI (include/ccmp.h: ccmp_plan_*): stefanBiPRM::solve as one resumable
// handle.  The handle owns a state block on the device (ccmp_plan_state) and one block of call buffers sized at creation for `width`
// candidates; a cycle is the sequence of include/ccmp.h over the store's own entry points (ccmp_object_propose_batch, ccmp_roadmap_grow /
// _grow_vetted, ccmp_roadmap_commit, ccmp_roadmap_closest, ccmp_object_valid_batch, ccmp_pose_ik_batch / _vetted_batch,
// ccmp_roadmap_connect) on the context's stream, with the kernels of ccmp_kernels_plan.hip between them: the store, the edge list, the
// labels and the candidates' arrays never cross to the host.  What the host reads: the commits' own counts, 16 bytes after the IK of a
// check that ran (which of the three branches have a vertex to add: the branches that do not are not launched), and the state block
// once at the end of a cycle.  What every planner handle on the store does alike — the state block's reads, open's upload, the run loop,
// the solution test, the head of the report — is ccmp_planner.h's, shared with ccmp_rrtc.cpp; the handle and the list of its arrays are
// there too.  The *_ref forms at the end compile the rule text of ccmp_plan.h for the host.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_ik.h"
#include "ccmp_launch.h"
#include "ccmp_plan.h"
#include "ccmp_planner.h"
#include "ccmp_pose.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

// the layouts the Python binding restates (closed_chain_motion_planner_amd/_lib.py)
static_assert(sizeof(ccmp_plan_opts) == 96 && sizeof(ccmp_plan_counters) == 48 && sizeof(ccmp_plan_state) == 240 && sizeof(ccmp_plan_report) == 112, "ccmp_plan_* layout");

namespace {

// addMilestone of Q rows (joints [Q][14], pose [Q][8], device rows): the object-metric k-NN and checkMotion from every neighbour (knn;
// without it the caller has emptied the slots), then the commit under `flags`
int connect_commit(ccmp_plan *pl, const double *joints, const double *pose, size_t Q, int flags, bool knn = true)
{
  hipStream_t st = pl->ctx->stream;
  const int k = pl->o.k;
  if (knn) {
    const int rc = ccmp_roadmap_connect(pl->rm, &pl->p, pl->scene, pl->scene ? pl->margin : 0.0, CCMP_METRIC_OBJECT, joints, pose, Q, k, CCMP_KNN_ALL, 0, 1,
                                        pl->o.max_states, 0, pl->nbr_idx, pl->nbr_dist, pl->states, pl->n_states, pl->ok, pl->iters, pl->blocked, pl->carry, st);
    if (rc != CCMP_OK) return rc;
  }
  return ccmp_roadmap_commit(pl->rm, nullptr, pl->nbr_idx, pl->ok, pl->n_states, nullptr, INT_MAX, joints, pose, nullptr, Q, k, nullptr, nullptr, 0, flags,
                             pl->new_index, pl->mid_index, pl->grow_state, nullptr, nullptr, st);
}

// startgoalMilestone of one vertex (joints [14], pose [8], device rows): connect_commit, which keeps it even without an edge, and the
// push onto starts (which == 0) or goals (1).  On an empty store the slots are empty without a launch of the k-NN.
int milestone(ccmp_plan *pl, const double *joints, const double *pose, int which)
{
  hipStream_t st = pl->ctx->stream;
  const size_t k = (size_t)pl->o.k;
  const bool empty = ccmp_roadmap_size(pl->rm) == 0;
  if (empty) {
    HIP_TRY(hipMemsetAsync(pl->nbr_idx, 0xff, k * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(pl->ok, 0, k, st));
    HIP_TRY(hipMemsetAsync(pl->n_states, 0, k * sizeof(int32_t), st));
  }
  const int rc = connect_commit(pl, joints, pose, 1, CCMP_COMMIT_KEEP_ISOLATED, !empty);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::plan_push(pl->state, which, pl->new_index, st));
  return CCMP_OK;
}

// T IK targets with one seed slot each, the vetted form when the handle has a scene
int solve_ik(ccmp_plan *pl, const double *targets, const double *seeds, size_t T, uint64_t first_index, double *q, uint8_t *ok, int32_t *which, double *clear)
{
  hipStream_t st = pl->ctx->stream;
  if (pl->scene)
    return ccmp_pose_ik_vetted_batch(pl->ctx, &pl->p, &pl->ik, targets, seeds, T, 1, pl->seed, first_index, pl->scene, pl->margin, q, ok, which, nullptr, nullptr,
                                     nullptr, nullptr, clear, st);
  return ccmp_pose_ik_batch(pl->ctx, &pl->p, &pl->ik, targets, seeds, T, 1, pl->seed, first_index, q, ok, which, nullptr, nullptr, st);
}

int growth(ccmp_plan *pl)
{
  hipStream_t st = pl->ctx->stream;
  const ccmp_plan_opts &o = pl->o;
  const size_t W = (size_t)o.width;
  const uint64_t first = pl->host.next_index;
  HIP_TRY(ccmp_launch::plan_front(pl->state, pl->from, W, st));
  int rc = ccmp_object_propose_batch(pl->ctx, pl->obj, pl->from, pl->d_goal_pose, 0, W, o.t, o.sigma, o.lo, o.hi, o.attempts, pl->seed, first, o.inflate, pl->prop,
                                     pl->which, nullptr, nullptr, st);
  if (rc != CCMP_OK) return rc;
  if (pl->scene)
    rc = ccmp_roadmap_grow_vetted(pl->rm, &pl->p, pl->scene, pl->margin, &pl->ik, pl->prop, W, o.k, CCMP_KNN_ALL, 0, pl->seed, first, 0, o.max_states, 0,
                                  pl->nbr_idx, pl->nbr_dist, pl->q_new, pl->ik_ok, pl->ik_which, pl->ik_clear, pl->states, pl->n_states, pl->ok, pl->iters,
                                  pl->blocked, pl->carry, st);
  else
    rc = ccmp_roadmap_grow(pl->rm, &pl->p, nullptr, 0.0, &pl->ik, pl->prop, W, o.k, CCMP_KNN_ALL, 0, pl->seed, first, 0, o.max_states, 0, pl->nbr_idx,
                           pl->nbr_dist, pl->q_new, pl->ik_ok, pl->ik_which, pl->states, pl->n_states, pl->ok, pl->iters, pl->blocked, pl->carry, st);
  if (rc != CCMP_OK) return rc;
  rc = ccmp_roadmap_commit(pl->rm, &pl->p, pl->nbr_idx, pl->ok, pl->n_states, pl->states, o.max_states, pl->q_new, pl->prop, pl->ik_ok, W, o.k, pl->goal_pose,
                           pl->host.starts, pl->host.n_starts, 0, pl->new_index, pl->mid_index, pl->grow_state, nullptr, nullptr, st);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::plan_tally(pl->state, pl->which, pl->ik_ok, pl->new_index, pl->mid_index, pl->grow_state, W, o.k, 0, st));
  return CCMP_OK;
}

int check(ccmp_plan *pl)
{
  hipStream_t st = pl->ctx->stream;
  const ccmp_plan_opts &o = pl->o;
  const ccmp_plan_state &h = pl->host;
  const size_t size = ccmp_roadmap_size(pl->rm);
  if (!ccmp::plan_gate(size, h.size_at_check) || h.n_goals < 1 || h.n_starts < 1) return CCMP_OK;
  const uint64_t first = h.next_index; // growth has advanced the device's copy and this one alike (run())
  ccmp_launch::GraphStore gs;
  roadmap_arrays(pl->rm, &gs);
  int rc = ccmp_roadmap_closest(pl->rm, dev_starts(pl->state), (size_t)h.n_starts, gs.poses + (size_t)h.goals[0] * 8, pl->a_idx, pl->a_dist, pl->a_from, st);
  if (rc != CCMP_OK) return rc;
  rc = ccmp_roadmap_closest(pl->rm, dev_goals(pl->state), (size_t)h.n_goals, gs.poses + (size_t)h.starts[0] * 8, pl->b_idx, pl->b_dist, pl->b_from, st);
  if (rc != CCMP_OK) return rc;
  ccmp_launch::PlanCheck c{pl->a_idx, pl->a_dist, pl->a_from, pl->b_idx, pl->b_dist, pl->b_from, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0},
                           pl->targets, pl->seeds, pl->trig};
  memcpy(c.goal, pl->goal_pose, 7 * sizeof(double));
  memcpy(c.start, pl->start_pose, 7 * sizeof(double));
  HIP_TRY(ccmp_launch::plan_check(gs, pl->state, c, st));
  rc = ccmp_object_valid_batch(pl->ctx, pl->obj, pl->targets + 8 * ccmp::kPlanLadderRow, CCMP_PLAN_LADDER, o.inflate, pl->valid, nullptr, st);
  if (rc != CCMP_OK) return rc;
  rc = solve_ik(pl, pl->targets, pl->seeds, ccmp::kPlanTargets, first, pl->ikq, pl->ik11_ok, pl->ik11_which, pl->ik11_clear);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::plan_prefix(pl->state, pl->trig, pl->valid, pl->ik11_ok, pl->vertex_ok, pl->summary, st));
  int32_t sum[4] = {0, 0, 0, 0};
  if ((rc = read_back(sum, pl->summary, sizeof sum, st)) != CCMP_OK) return rc;
  if (sum[1]) { rc = milestone(pl, pl->ikq + 14 * ccmp::kPlanGoalRow, pl->d_goal_pose, 1); if (rc != CCMP_OK) return rc; }
  if (sum[0] > 0 && sum[0] <= CCMP_PLAN_LADDER) { // addMilestone of the prefix, one batch
    const size_t L = (size_t)sum[0];
    const double *lj = pl->ikq + 14 * ccmp::kPlanLadderRow, *lp = pl->targets + 8 * ccmp::kPlanLadderRow;
    if ((rc = connect_commit(pl, lj, lp, L, 0)) != CCMP_OK) return rc;
    HIP_TRY(ccmp_launch::plan_tally(pl->state, nullptr, nullptr, pl->new_index, nullptr, nullptr, L, o.k, 1, st));
  }
  if (sum[2]) { rc = milestone(pl, pl->ikq + 14 * ccmp::kPlanStartRow, pl->d_start_pose, 0); if (rc != CCMP_OK) return rc; }
  return CCMP_OK;
}

bool finite3(const double *v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

int opts_ok(const ccmp_plan_opts *o)
{
  if (o->width < 1 || o->width > CCMP_PLAN_MAX_WIDTH || o->k < 1 || o->k > CCMP_IK_MAX_SEEDS || o->k > CCMP_KNN_MAX_K) return CCMP_EINVAL;
  if (o->attempts < 1 || o->attempts > CCMP_OBJECT_MAX_ATTEMPTS || o->max_states < 1) return CCMP_EINVAL;
  if (!std::isfinite(o->t) || !std::isfinite(o->sigma) || !std::isfinite(o->inflate) || o->sigma < 0.0 || o->inflate < 0.0) return CCMP_EINVAL;
  if (!finite3(o->lo) || !finite3(o->hi)) return CCMP_EINVAL;
  for (int i = 0; i < 3; i++)
    if (o->lo[i] > o->hi[i]) return CCMP_EINVAL;
  if (o->max_vertices > (uint64_t)INT32_MAX) return CCMP_EINVAL;
  return CCMP_OK;
}

// ccmp_planner.h's run loop on this planner: a cycle is growth then check, the solution test is the loop's
struct PlanLoop {
  static bool terminal(int status) { return status == CCMP_PLAN_SOLVED || status == CCMP_PLAN_INVALID_GOAL; }
  static bool full(const ccmp_plan *pl) { return ccmp::plan_full(ccmp_roadmap_size(pl->rm), pl->o.width, pl->o.k, pl->o.max_vertices); }
  static int cycle(ccmp_plan *pl)
  {
    const int rc = growth(pl);
    if (rc != CCMP_OK) return rc;
    pl->host.next_index += (uint64_t)pl->o.width; // what plan_tally_kernel did to the device's copy
    return check(pl);
  }
  static void report(const ccmp_plan *pl, int cycles_run, ccmp_plan_report *out)
  {
    if (!report_head(pl, cycles_run, out)) return;
    const ccmp_plan_state &s = pl->host;
    out->nearest = s.nearest;
    out->prev_from_goal = s.prev_from_goal;
    out->prev_from_start = s.prev_from_start;
    out->counters = s.counters;
  }
};

}  // namespace

extern "C" {

void ccmp_plan_default_opts(ccmp_plan_opts *o)
{
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->width = 32;
  o->k = 5;
  o->attempts = 2;
  o->max_states = 64;
  o->t = 0.3;
  o->sigma = 0.2;
  o->inflate = 0.0;
  for (int i = 0; i < 3; i++) { o->lo[i] = -1e30; o->hi[i] = 1e30; }
  o->max_vertices = (uint64_t)INT32_MAX;
}

int ccmp_plan_create(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_object *object, const ccmp_scene *scene, double margin, const ccmp_ik_opts *ik_opts,
                     const ccmp_plan_opts *opts, const double *goal_joints, uint64_t rng_seed, uint64_t first_index, ccmp_plan **out)
{
  if (out) *out = nullptr;
  if (!rm) return no_handle();
  if (!p || !object || !opts || !out) return CCMP_EINVAL;
  { const int rc = opts_ok(opts); if (rc != CCMP_OK) return rc; }
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  ccmp_ctx *ctx = roadmap_ctx(rm);
  ccmp_ik_opts ik;
  ccmp_ik_opts_default(&ik);
  if (ik_opts) ik = *ik_opts;
  { ccmp::ik_params P; const int rc = ik_checks(p, &ik, (size_t)(opts->width > ccmp::kPlanTargets ? opts->width : ccmp::kPlanTargets), opts->k, &P); if (rc != CCMP_OK) return rc; }
  if (object_device(object) != ctx->device) return CCMP_EINVAL;
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
  if (goal_joints)
    for (int i = 0; i < 14; i++)
      if (!std::isfinite(goal_joints[i])) return CCMP_EINVAL;
  const size_t size0 = ccmp_roadmap_size(rm);
  if (opts->max_vertices < size0 || opts->max_vertices - size0 < 2) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_plan *pl = new (std::nothrow) ccmp_plan();
  if (!pl) return CCMP_ENOMEM;
  pl->rm = rm;
  pl->ctx = ctx;
  pl->device = ctx->device;
  pl->p = *p;
  pl->obj = object;
  pl->scene = scene;
  pl->margin = scene ? margin : 0.0;
  pl->ik = ik;
  pl->o = *opts;
  pl->seed = rng_seed;
  {
    double t[12];
    memcpy(t, p->obj_start_R, 9 * sizeof(double));
    memcpy(t + 9, p->obj_start_p, 3 * sizeof(double));
    ccmp_pose_of_t_wo(t, pl->start_pose);
    memcpy(t, p->obj_goal_R, 9 * sizeof(double));
    memcpy(t + 9, p->obj_goal_p, 3 * sizeof(double));
    ccmp_pose_of_t_wo(t, pl->goal_pose);
    pl->start_pose[7] = pl->goal_pose[7] = 0.0;
  }
  ResultBlock rb; // the one block: ccmp_planner.h's list
  { const int rc = rb.alloc_pieces(pl, ctx, __func__); if (rc != CCMP_OK) { delete pl; return rc; } }

  hipStream_t st = ctx->stream;
  ccmp_plan_state &h = pl->host;
  memset(&h, 0, sizeof h);
  h.nearest = h.sprevious = h.solved_start = h.solved_goal = -1;
  h.status = CCMP_PLAN_OPEN;
  h.next_index = first_index;
  h.prev_from_goal = h.prev_from_start = ccmp_pose_dist(pl->start_pose, pl->goal_pose);
  memcpy(h.nearest_pose, pl->start_pose, sizeof h.nearest_pose);
  int rc = CCMP_OK;
  auto fail = [&](int code) { ccmp_plan_destroy(pl); return code; };
  rc = planner_upload(pl, {{pl->d_start_pose, pl->start_pose, 64}, {pl->d_goal_pose, pl->goal_pose, 64}, {pl->d_start_joint, p->start_joint, 112},
                           {pl->d_goal_joint, goal_joints, 112}}, __func__);
  if (rc != CCMP_OK) return fail(rc);
  if ((rc = milestone(pl, pl->d_start_joint, pl->d_start_pose, 0)) != CCMP_OK) return fail(rc);
  bool have_goal = true;
  if (!goal_joints) { // sampleCalibGoal(t_wo_goal) seeded from the start state
    rc = solve_ik(pl, pl->d_goal_pose, pl->d_start_joint, 1, first_index, pl->d_goal_joint, pl->ik11_ok, pl->ik11_which, pl->ik11_clear);
    if (rc != CCMP_OK) return fail(rc);
    uint8_t solved = 0;
    const hipError_t e = hipMemcpyAsync(&solved, pl->ik11_ok, 1, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e != hipSuccess || es != hipSuccess) return fail(hip_fail(e != hipSuccess ? e : es, __func__));
    have_goal = solved != 0;
  }
  if (have_goal && (rc = milestone(pl, pl->d_goal_joint, pl->d_goal_pose, 1)) != CCMP_OK) return fail(rc);
  if ((rc = read_state(pl)) != CCMP_OK) return fail(rc);
  h.next_index = first_index + 1;
  h.nearest = h.n_starts > 0 ? h.starts[0] : -1;
  h.sprevious = h.n_goals > 0 ? h.goals[0] : -1;
  h.size_at_check = (int32_t)ccmp_roadmap_size(rm);
  if (!have_goal) h.status = CCMP_PLAN_INVALID_GOAL;
  if ((rc = write_state(pl)) != CCMP_OK) return fail(rc);
  if (have_goal && (rc = solution_test(pl, 0)) != CCMP_OK) return fail(rc);
  *out = pl;
  return CCMP_OK;
}

int ccmp_plan_run(ccmp_plan *pl, int max_cycles, ccmp_plan_report *out) { return planner_run<PlanLoop>(pl, max_cycles, out); }

int ccmp_plan_state_read(ccmp_plan *pl, ccmp_plan_state *out) { return planner_state_read(pl, out); }

void ccmp_plan_destroy(ccmp_plan *pl) { result_destroy(pl); }

int ccmp_plan_check_ref(ccmp_plan_state *state, size_t size, const int32_t *a_idx, const double *a_dist, const double *a_from, const int32_t *b_idx,
                        const double *b_dist, const double *b_from, const double *store_poses, int32_t triggers[4])
{
  if (!state || !triggers || state->n_starts < 0 || state->n_starts > CCMP_PLAN_MAX_STARTS || state->n_goals < 0 || state->n_goals > CCMP_PLAN_MAX_GOALS ||
      size > (size_t)INT32_MAX)
    return CCMP_EINVAL;
  if (state->n_starts > 0 && (!a_idx || !a_dist || !a_from)) return CCMP_EINVAL;
  if (state->n_goals > 0 && (!b_idx || !b_dist || !b_from)) return CCMP_EINVAL;
  ccmp::plan_check(state, size, a_idx, a_dist, a_from, b_idx, b_dist, b_from, triggers);
  if (triggers[1] && store_poses) memcpy(state->nearest_pose, store_poses + (size_t)triggers[3] * 8, 8 * sizeof(double));
  return CCMP_OK;
}

int ccmp_plan_prefix_ref(const uint8_t valid[9], const uint8_t ik_ok[9], uint8_t vertex_ok[9], int32_t *prefix_len)
{
  if (!valid || !ik_ok || !vertex_ok) return CCMP_EINVAL;
  const int n = ccmp::plan_prefix(valid, ik_ok, vertex_ok);
  if (prefix_len) *prefix_len = n;
  return CCMP_OK;
}

int ccmp_plan_connected_ref(const int32_t *labels, size_t N, ccmp_plan_state *state)
{
  if (!state || (N > 0 && !labels) || state->n_starts < 0 || state->n_starts > CCMP_PLAN_MAX_STARTS || state->n_goals < 0 ||
      state->n_goals > CCMP_PLAN_MAX_GOALS)
    return CCMP_EINVAL;
  ccmp::first_connected(state, labels, N);
  return CCMP_OK;
}

}  // extern "C"
