// ccmp_plan.cpp — the planner's loop on the roadmap store in the C ABI (include/ccmp.h: ccmp_plan_*): stefanBiPRM::solve as one resumable
// handle.  The handle owns a state block on the device (ccmp_plan_state) and one block of call buffers sized at creation for `width`
// candidates; a cycle is the sequence of include/ccmp.h over the store's own entry points (ccmp_object_propose_batch, ccmp_roadmap_grow /
// _grow_vetted, ccmp_roadmap_commit, ccmp_roadmap_closest, ccmp_object_valid_batch, ccmp_pose_ik_batch / _vetted_batch,
// ccmp_roadmap_connect) on the context's stream, with the kernels of ccmp_kernels_plan.hip between them: the store, the edge list, the
// labels and the candidates' arrays never cross to the host.  What the host reads: the commits' own counts, 16 bytes after the IK of a
// check that ran (which of the three branches have a vertex to add: the branches that do not are not launched), and the state block
// once at the end of a cycle.  The *_ref forms at the end compile the rule text of ccmp_plan.h for the host.
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
#include "ccmp_pose.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

// the layouts the Python binding restates (closed_chain_motion_planner_amd/_lib.py)
static_assert(sizeof(ccmp_plan_opts) == 96 && sizeof(ccmp_plan_counters) == 48 && sizeof(ccmp_plan_state) == 240 && sizeof(ccmp_plan_report) == 112, "ccmp_plan_* layout");

struct ccmp_plan {
  ccmp_roadmap *rm = nullptr;
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  ccmp_problem p;
  const ccmp_object *obj = nullptr;
  const ccmp_scene *scene = nullptr;
  double margin = 0.0;
  ccmp_ik_opts ik;
  ccmp_plan_opts o;
  uint64_t seed = 0;
  double start_pose[8], goal_pose[8];
  ccmp_plan_state host; // the state block as last read
  void *block = nullptr;
  // the pieces of `block`
  ccmp_plan_state *state;
  double *d_start_pose, *d_goal_pose, *d_start_joint, *d_goal_joint;
  double *from, *prop, *nbr_dist, *q_new, *ik_clear, *states, *carry;
  int32_t *which, *nbr_idx, *ik_which, *n_states, *iters, *new_index, *mid_index, *grow_state;
  uint8_t *ik_ok, *ok, *blocked;
  int32_t *a_idx, *b_idx, *trig, *summary, *ik11_which;
  double *a_dist, *a_from, *b_dist, *b_from, *targets, *seeds, *ikq, *ik11_clear;
  uint8_t *valid, *vertex_ok, *ik11_ok;
};

namespace {

void report_of(const ccmp_plan *pl, int cycles_run, ccmp_plan_report *out)
{
  if (!out) return;
  const ccmp_plan_state &s = pl->host;
  memset(out, 0, sizeof *out);
  out->status = s.status;
  out->cycles_run = cycles_run;
  out->cycles_total = s.cycle;
  out->size = ccmp_roadmap_size(pl->rm);
  out->edges = ccmp_roadmap_num_edges(pl->rm);
  out->solved_start = s.solved_start;
  out->solved_goal = s.solved_goal;
  out->nearest = s.nearest;
  out->prev_from_goal = s.prev_from_goal;
  out->prev_from_start = s.prev_from_start;
  out->counters = s.counters;
}

int read_state(ccmp_plan *pl)
{
  const hipError_t e = hipMemcpyAsync(&pl->host, pl->state, sizeof(ccmp_plan_state), hipMemcpyDeviceToHost, pl->ctx->stream);
  const hipError_t es = hipStreamSynchronize(pl->ctx->stream);
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
}

int write_state(ccmp_plan *pl)
{
  HIP_TRY(hipMemcpyAsync(pl->state, &pl->host, sizeof(ccmp_plan_state), hipMemcpyHostToDevice, pl->ctx->stream));
  HIP_TRY(hipStreamSynchronize(pl->ctx->stream));
  return CCMP_OK;
}

// startgoalMilestone of one vertex (joints [14], pose [8], device rows): the object-metric k-NN and checkMotion from every neighbour,
// the commit that keeps it even without an edge, and the push onto starts (which == 0) or goals (1).  On an empty store the slots are
// empty without a launch of the k-NN.
int milestone(ccmp_plan *pl, const double *joints, const double *pose, int which)
{
  hipStream_t st = pl->ctx->stream;
  const int k = pl->o.k;
  if (ccmp_roadmap_size(pl->rm) == 0) {
    HIP_TRY(hipMemsetAsync(pl->nbr_idx, 0xff, (size_t)k * sizeof(int32_t), st));
    HIP_TRY(hipMemsetAsync(pl->ok, 0, (size_t)k, st));
    HIP_TRY(hipMemsetAsync(pl->n_states, 0, (size_t)k * sizeof(int32_t), st));
  } else {
    const int rc = ccmp_roadmap_connect(pl->rm, &pl->p, pl->scene, pl->scene ? pl->margin : 0.0, CCMP_METRIC_OBJECT, joints, pose, 1, k, CCMP_KNN_ALL, 0, 1,
                                        pl->o.max_states, 0, pl->nbr_idx, pl->nbr_dist, pl->states, pl->n_states, pl->ok, pl->iters, pl->blocked, pl->carry, st);
    if (rc != CCMP_OK) return rc;
  }
  const int rc = ccmp_roadmap_commit(pl->rm, nullptr, pl->nbr_idx, pl->ok, pl->n_states, nullptr, INT_MAX, joints, pose, nullptr, 1, k, nullptr, nullptr, 0,
                                     CCMP_COMMIT_KEEP_ISOLATED, pl->new_index, pl->mid_index, pl->grow_state, nullptr, nullptr, st);
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
  int32_t *d_starts = (int32_t *)((char *)pl->state + offsetof(ccmp_plan_state, starts));
  int32_t *d_goals = (int32_t *)((char *)pl->state + offsetof(ccmp_plan_state, goals));
  int rc = ccmp_roadmap_closest(pl->rm, d_starts, (size_t)h.n_starts, gs.poses + (size_t)h.goals[0] * 8, pl->a_idx, pl->a_dist, pl->a_from, st);
  if (rc != CCMP_OK) return rc;
  rc = ccmp_roadmap_closest(pl->rm, d_goals, (size_t)h.n_goals, gs.poses + (size_t)h.starts[0] * 8, pl->b_idx, pl->b_dist, pl->b_from, st);
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
  {
    const hipError_t e = hipMemcpyAsync(sum, pl->summary, sizeof sum, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    HIP_TRY(e);
    HIP_TRY(es);
  }
  if (sum[1]) { rc = milestone(pl, pl->ikq + 14 * ccmp::kPlanGoalRow, pl->d_goal_pose, 1); if (rc != CCMP_OK) return rc; }
  if (sum[0] > 0 && sum[0] <= CCMP_PLAN_LADDER) { // addMilestone of the prefix, one batch
    const size_t L = (size_t)sum[0];
    const double *lj = pl->ikq + 14 * ccmp::kPlanLadderRow, *lp = pl->targets + 8 * ccmp::kPlanLadderRow;
    rc = ccmp_roadmap_connect(pl->rm, &pl->p, pl->scene, pl->scene ? pl->margin : 0.0, CCMP_METRIC_OBJECT, lj, lp, L, o.k, CCMP_KNN_ALL, 0, 1, o.max_states, 0,
                              pl->nbr_idx, pl->nbr_dist, pl->states, pl->n_states, pl->ok, pl->iters, pl->blocked, pl->carry, st);
    if (rc != CCMP_OK) return rc;
    rc = ccmp_roadmap_commit(pl->rm, nullptr, pl->nbr_idx, pl->ok, pl->n_states, nullptr, INT_MAX, lj, lp, nullptr, L, o.k, nullptr, nullptr, 0, 0, pl->new_index,
                             pl->mid_index, pl->grow_state, nullptr, nullptr, st);
    if (rc != CCMP_OK) return rc;
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
  // the one block: the state, the fixed rows, the growth step's arrays for Qm queries, the check's
  const size_t W = (size_t)opts->width, k = (size_t)opts->k, ms = (size_t)opts->max_states;
  const size_t Qm = W > (size_t)ccmp::kPlanTargets ? W : (size_t)ccmp::kPlanTargets, E = Qm * k;
  ResultBlock rb;
  const size_t o_state = rb.take(sizeof(ccmp_plan_state)), o_sp = rb.take(64), o_gp = rb.take(64), o_sj = rb.take(112), o_gj = rb.take(112),
               o_from = rb.take(Qm * 64), o_prop = rb.take(Qm * 64), o_which = rb.take(Qm * 4), o_ni = rb.take(E * 4), o_nd = rb.take(E * 8),
               o_qn = rb.take(Qm * 112), o_io = rb.take(Qm), o_iw = rb.take(Qm * 4), o_ic = rb.take(Qm * 8), o_st = rb.take(E * ms * 112), o_ns = rb.take(E * 4),
               o_ok = rb.take(E), o_it = rb.take(E * 4), o_bl = rb.take(E), o_ca = rb.take(E * 16), o_new = rb.take(Qm * 4), o_mid = rb.take(E * 4),
               o_gs = rb.take(Qm * 4), o_ai = rb.take(32), o_ad = rb.take(64), o_af = rb.take(64), o_bi = rb.take(32), o_bd = rb.take(64), o_bf = rb.take(64),
               o_tg = rb.take(ccmp::kPlanTargets * 64), o_sd = rb.take(ccmp::kPlanTargets * 112), o_tr = rb.take(16), o_su = rb.take(16), o_va = rb.take(16),
               o_vo = rb.take(16), o_iq = rb.take(ccmp::kPlanTargets * 112), o_i11 = rb.take(16), o_w11 = rb.take(ccmp::kPlanTargets * 4),
               o_c11 = rb.take(ccmp::kPlanTargets * 8);
  { const int rc = rb.alloc(pl, ctx, __func__); if (rc != CCMP_OK) { delete pl; return rc; } }
  pl->state = rb.at<ccmp_plan_state>(o_state);
  pl->d_start_pose = rb.at<double>(o_sp); pl->d_goal_pose = rb.at<double>(o_gp); pl->d_start_joint = rb.at<double>(o_sj); pl->d_goal_joint = rb.at<double>(o_gj);
  pl->from = rb.at<double>(o_from); pl->prop = rb.at<double>(o_prop); pl->which = rb.at<int32_t>(o_which); pl->nbr_idx = rb.at<int32_t>(o_ni);
  pl->nbr_dist = rb.at<double>(o_nd); pl->q_new = rb.at<double>(o_qn); pl->ik_ok = rb.at<uint8_t>(o_io); pl->ik_which = rb.at<int32_t>(o_iw);
  pl->ik_clear = rb.at<double>(o_ic); pl->states = rb.at<double>(o_st); pl->n_states = rb.at<int32_t>(o_ns); pl->ok = rb.at<uint8_t>(o_ok);
  pl->iters = rb.at<int32_t>(o_it); pl->blocked = rb.at<uint8_t>(o_bl); pl->carry = rb.at<double>(o_ca); pl->new_index = rb.at<int32_t>(o_new);
  pl->mid_index = rb.at<int32_t>(o_mid); pl->grow_state = rb.at<int32_t>(o_gs); pl->a_idx = rb.at<int32_t>(o_ai); pl->a_dist = rb.at<double>(o_ad);
  pl->a_from = rb.at<double>(o_af); pl->b_idx = rb.at<int32_t>(o_bi); pl->b_dist = rb.at<double>(o_bd); pl->b_from = rb.at<double>(o_bf);
  pl->targets = rb.at<double>(o_tg); pl->seeds = rb.at<double>(o_sd); pl->trig = rb.at<int32_t>(o_tr); pl->summary = rb.at<int32_t>(o_su);
  pl->valid = rb.at<uint8_t>(o_va); pl->vertex_ok = rb.at<uint8_t>(o_vo); pl->ikq = rb.at<double>(o_iq); pl->ik11_ok = rb.at<uint8_t>(o_i11);
  pl->ik11_which = rb.at<int32_t>(o_w11); pl->ik11_clear = rb.at<double>(o_c11);

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
  quiesce(ctx);
  {
    hipError_t e = hipDeviceSynchronize(); // appends on any stream before this call are seen
    if (e == hipSuccess) e = hipMemcpyAsync(pl->state, &h, sizeof h, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->d_start_pose, pl->start_pose, 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->d_goal_pose, pl->goal_pose, 64, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(pl->d_start_joint, p->start_joint, 112, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && goal_joints) e = hipMemcpyAsync(pl->d_goal_joint, goal_joints, 112, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(hip_fail(e, __func__));
  }
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
  if (have_goal) {
    ccmp_launch::GraphStore gs;
    roadmap_arrays(rm, &gs);
    const hipError_t e = ccmp_launch::plan_connected(gs, pl->state, 0, st);
    if (e != hipSuccess) return fail(hip_fail(e, __func__));
    if ((rc = read_state(pl)) != CCMP_OK) return fail(rc);
  }
  *out = pl;
  return CCMP_OK;
}

int ccmp_plan_run(ccmp_plan *pl, int max_cycles, ccmp_plan_report *out)
{
  if (!pl) return no_handle();
  if (max_cycles < 0) return CCMP_EINVAL;
  ccmp_plan_state &h = pl->host;
  if (h.status == CCMP_PLAN_SOLVED || h.status == CCMP_PLAN_INVALID_GOAL || max_cycles == 0) { report_of(pl, 0, out); return CCMP_OK; } // no cycle: the report as it stands
  DeviceGuard guard(pl->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = pl->ctx->stream;
  quiesce(pl->ctx);
  HIP_TRY(hipDeviceSynchronize());
  int ran = 0, status = CCMP_PLAN_BUDGET;
  for (; ran < max_cycles; ran++) {
    if (ccmp::plan_full(ccmp_roadmap_size(pl->rm), pl->o.width, pl->o.k, pl->o.max_vertices)) { status = CCMP_PLAN_FULL; break; }
    { const int rc = growth(pl); if (rc != CCMP_OK) return rc; }
    h.next_index += (uint64_t)pl->o.width; // what plan_tally_kernel did to the device's copy
    { const int rc = check(pl); if (rc != CCMP_OK) return rc; }
    ccmp_launch::GraphStore gs;
    roadmap_arrays(pl->rm, &gs);
    HIP_TRY(ccmp_launch::plan_connected(gs, pl->state, 1, st));
    { const int rc = read_state(pl); if (rc != CCMP_OK) return rc; }
    if (h.status == CCMP_PLAN_SOLVED) { status = CCMP_PLAN_SOLVED; ran++; break; }
  }
  if (h.status != status) { // BUDGET / FULL: the loop's own verdicts, kept in the block too
    h.status = status;
    const int rc = write_state(pl);
    if (rc != CCMP_OK) return rc;
  }
  report_of(pl, ran, out);
  return CCMP_OK;
}

int ccmp_plan_state_read(ccmp_plan *pl, ccmp_plan_state *out)
{
  if (!pl) return no_handle();
  if (!out) return CCMP_EINVAL;
  DeviceGuard guard(pl->device);
  if (!guard.ok) return CCMP_ENODEV;
  const int rc = read_state(pl);
  if (rc != CCMP_OK) return rc;
  *out = pl->host;
  return CCMP_OK;
}

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
  if (state->status == CCMP_PLAN_SOLVED) return CCMP_OK;
  for (int s = 0; s < state->n_starts; s++)
    for (int g = 0; g < state->n_goals; g++)
      if (ccmp::plan_pair_connected(state, s, g, labels, N)) { ccmp::plan_solved(state, s, g); return CCMP_OK; }
  return CCMP_OK;
}

}  // extern "C"
