/* ccmp_planner.h — what a resumable planner handle on a roadmap store shares (ccmp_plan.cpp, ccmp_rrtc.cpp).  Host only, hidden, C++
 * linkage, nothing of the C ABI (as the path units' share in ccmp_stage.h).  A handle H has the fields rm, ctx, device, block, `host` (the
 * state block as last read) and `state` (the device's); the state type is one that ccmp_plan.h's solution test takes.  A planner adds
 * its checks, its open and a traits struct L for planner_run: terminal(status) — a status no cycle follows —, full(H *) — the FULL rule,
 * asked before every cycle —, cycle(H *) — the cycle's body without the solution test — and report(H *, cycles_run, out). */
#ifndef CCMP_PLANNER_H
#define CCMP_PLANNER_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>
#include <initializer_list>

#include "ccmp_launch.h"
#include "ccmp_plan.h"
#include "ccmp_rrtc.h"
#include "ccmp_stage.h"

/* ---- the two handles on this skeleton, each with the one list of its block's arrays (ccmp_stage.h: ResultBlock::alloc_pieces) */
/* ccmp_plan.cpp's handle */
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

  /* the one block, in this order: the state, the fixed rows, the growth step's arrays for Qm queries of k slots, the check's.  B is
   * ccmp_stage.h's ResultBlock: piece(pointer, elements). */
  template <class B> void pieces(B &b)
  {
    const size_t T = (size_t)ccmp::kPlanTargets, Qm = (size_t)o.width > T ? (size_t)o.width : T, E = Qm * (size_t)o.k, ms = (size_t)o.max_states;
    b.piece(state, 1);
    b.piece(d_start_pose, 8); b.piece(d_goal_pose, 8); b.piece(d_start_joint, 14); b.piece(d_goal_joint, 14);
    b.piece(from, Qm * 8); b.piece(prop, Qm * 8); b.piece(which, Qm); b.piece(nbr_idx, E); b.piece(nbr_dist, E);
    b.piece(q_new, Qm * 14); b.piece(ik_ok, Qm); b.piece(ik_which, Qm); b.piece(ik_clear, Qm);
    b.piece(states, E * ms * 14); b.piece(n_states, E); b.piece(ok, E); b.piece(iters, E); b.piece(blocked, E); b.piece(carry, E * 2);
    b.piece(new_index, Qm); b.piece(mid_index, E); b.piece(grow_state, Qm);
    b.piece(a_idx, 8); b.piece(a_dist, 8); b.piece(a_from, 8); b.piece(b_idx, 8); b.piece(b_dist, 8); b.piece(b_from, 8);
    b.piece(targets, T * 8); b.piece(seeds, T * 14); b.piece(trig, 4); b.piece(summary, 4); b.piece(valid, 16); b.piece(vertex_ok, 16);
    b.piece(ikq, T * 14); b.piece(ik11_ok, 16); b.piece(ik11_which, T); b.piece(ik11_clear, T);
  }
};

/* ccmp_rrtc.cpp's handle */
struct ccmp_rrtc {
  ccmp_roadmap *rm = nullptr;
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  ccmp_problem p;
  const ccmp_scene *scene = nullptr;
  double margin = 0.0;
  ccmp_rrtc_opts o;
  uint64_t seed = 0;
  ccmp_rrtc_state host; // the state block as last read
  void *block = nullptr;
  // the pieces of `block`
  ccmp_rrtc_state *state;
  double *samples, *clear, *dist, *from, *to, *states, *carry, *rowA, *rowB, *gapB, *rows;
  uint8_t *s_ok, *jv, *free_, *use, *ok, *blocked, *madeA;
  int32_t *idxA, *idxB, *n_states, *iters, *outA, *outB, *rixA, *rixB, *parA, *parB, *uv, *counts;

  /* the one block, in this order: the state, then the cycle's arrays for W rows.  B is ccmp_stage.h's ResultBlock: piece(pointer, elements). */
  template <class B> void pieces(B &b)
  {
    const size_t W = (size_t)o.width, ms = (size_t)o.max_states;
    b.piece(state, 1);
    b.piece(samples, W * 14); b.piece(clear, W); b.piece(dist, W); b.piece(from, W * 14); b.piece(to, W * 14); b.piece(states, W * ms * 14);
    b.piece(carry, W * 2); b.piece(rowA, W * 14); b.piece(rowB, W * 14); b.piece(gapB, W); b.piece(rows, 2 * W * 14);
    b.piece(s_ok, W); b.piece(jv, W); b.piece(free_, W); b.piece(use, W); b.piece(ok, W); b.piece(blocked, W); b.piece(madeA, W);
    b.piece(idxA, W); b.piece(idxB, W); b.piece(n_states, W); b.piece(iters, W); b.piece(outA, W); b.piece(outB, W); b.piece(rixA, W);
    b.piece(rixB, W); b.piece(parA, W); b.piece(parB, W); b.piece(uv, 2 * W * 2); b.piece(counts, 4);
  }
};

namespace ccmp_host {
#pragma GCC visibility push(hidden)

template <class H> int read_state(H *pl) { return read_back(&pl->host, pl->state, sizeof pl->host, pl->ctx->stream); }

template <class H> int write_state(H *pl)
{
  HIP_TRY(hipMemcpyAsync(pl->state, &pl->host, sizeof pl->host, hipMemcpyHostToDevice, pl->ctx->stream));
  HIP_TRY(hipStreamSynchronize(pl->ctx->stream));
  return CCMP_OK;
}

/* the lists of the device's state block */
template <class S> int32_t *dev_starts(S *state) { return (int32_t *)((char *)state + offsetof(S, starts)); }
template <class S> int32_t *dev_goals(S *state) { return (int32_t *)((char *)state + offsetof(S, goals)); }

/* the whole of a *_state_read entry */
template <class H, class S> int planner_state_read(H *pl, S *out)
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

/* open's upload: the service kernel stopped, the device idle (appends on any stream before the call are seen), then `host` into the
 * state block and the planner's fixed rows (one without a source is skipped), one wait */
struct PlannerRow { void *dev; const void *src; size_t bytes; };
template <class H> int planner_upload(H *pl, std::initializer_list<PlannerRow> rows, const char *what)
{
  hipStream_t st = pl->ctx->stream;
  quiesce(pl->ctx);
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpyAsync(pl->state, &pl->host, sizeof pl->host, hipMemcpyHostToDevice, st);
  for (const PlannerRow &r : rows)
    if (e == hipSuccess && r.src) e = hipMemcpyAsync(r.dev, r.src, r.bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return e == hipSuccess ? CCMP_OK : hip_fail(e, what);
}

/* cycle += bump_cycle and the solution test on the store's arrays AS THEY STAND (a commit or an append may have moved them), then the
 * state block's read */
template <class H> int solution_test(H *pl, int bump_cycle)
{
  ccmp_launch::GraphStore gs;
  roadmap_arrays(pl->rm, &gs);
  HIP_TRY(ccmp_launch::plan_connected(gs, pl->state, bump_cycle, pl->ctx->stream));
  return read_state(pl);
}

/* the fields every report begins with; false: the caller wants no report */
template <class H, class R> bool report_head(const H *pl, int cycles_run, R *out)
{
  if (!out) return false;
  memset(out, 0, sizeof *out);
  out->status = pl->host.status;
  out->cycles_run = cycles_run;
  out->cycles_total = pl->host.cycle;
  out->size = ccmp_roadmap_size(pl->rm);
  out->edges = ccmp_roadmap_num_edges(pl->rm);
  out->solved_start = pl->host.solved_start;
  out->solved_goal = pl->host.solved_goal;
  return true;
}

/* the whole of a *_run entry: up to max_cycles cycles of FULL?, L::cycle, the solution test, SOLVED?; then the loop's own verdicts
 * (BUDGET, FULL) into the block too, and the report */
template <class L, class H, class R> int planner_run(H *pl, int max_cycles, R *out)
{
  if (!pl) return no_handle();
  if (max_cycles < 0) return CCMP_EINVAL;
  if (L::terminal(pl->host.status) || max_cycles == 0) { L::report(pl, 0, out); return CCMP_OK; } // no cycle: the report as it stands
  DeviceGuard guard(pl->device);
  if (!guard.ok) return CCMP_ENODEV;
  quiesce(pl->ctx);
  HIP_TRY(hipDeviceSynchronize());
  int ran = 0, status = CCMP_PLAN_BUDGET;
  for (; ran < max_cycles; ran++) {
    if (L::full(pl)) { status = CCMP_PLAN_FULL; break; }
    { const int rc = L::cycle(pl); if (rc != CCMP_OK) return rc; }
    { const int rc = solution_test(pl, 1); if (rc != CCMP_OK) return rc; }
    if (pl->host.status == CCMP_PLAN_SOLVED) { status = CCMP_PLAN_SOLVED; ran++; break; }
  }
  if (pl->host.status != status) {
    pl->host.status = status;
    const int rc = write_state(pl);
    if (rc != CCMP_OK) return rc;
  }
  L::report(pl, ran, out);
  return CCMP_OK;
}

#pragma GCC visibility pop
}  // namespace ccmp_host

#endif /* CCMP_PLANNER_H */
