// ccmp_ik.cpp — growTree's sampleCalibGoal step of the C ABI (include/ccmp.h: ccmp_pose_ik_*).  The solver and the rule are csrc/ccmp_ik.h,
// one text: ccmp_pose_ik_ref runs it here on the host (no device; the checker of the GPU tests and the CPU contender of tools/measure.py
// ik), ccmp_pose_ik_batch launches ik_solve_kernel and ik_select_kernel (ccmp_kernels_ik.hip) on it.  Every check runs and the
// context's workspace has its size before the first launch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_host.h"
#include "ccmp_ik.h"
#include "ccmp_ik_vet.h"
#include "ccmp_launch.h"
#include "ccmp_scene_math.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

namespace {

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

// the candidates' records of a checked call on the host: ccmp_ik.h's solver from every start configuration (ik_solve_kernel's bits)
struct RefRecords {
  std::vector<double> q, d2;
  std::vector<int32_t> rounds;
};
int ref_records(const ccmp_problem *p, const ccmp_consts &K, const ccmp::ik_params &P, const double *target_poses, const double *seeds, size_t T, int S,
                uint64_t rng_seed, uint64_t first_index, RefRecords &rec)
{
  const size_t C = ik_candidates(T, S, P), per = (size_t)(1 + P.restarts);
  try { rec.q.resize(C * 7); rec.d2.resize(C); rec.rounds.resize(C); } catch (...) { return CCMP_ENOMEM; }
  for (size_t ts = 0; ts < T * (size_t)S; ts++) {
    const double *row = seeds + ts * 14;
    bool finite = true;
    for (int i = 0; i < 14; i++) finite = finite && ccmp::ik_finite(row[i]);
    for (int arm = 0; arm < 2; arm++) {
      const double *pose = target_poses + (ts / (size_t)S) * 8;
      for (int r = 0; r <= P.restarts; r++) {
        const size_t c = (ts * 2 + (size_t)arm) * per + (size_t)r;
        double q[7];
        int rounds = finite ? ccmp::kIkNotConverged : ccmp::kIkSkipped;
        if (finite) {
          ccmp::ik_start(K, P, rng_seed, first_index * (uint64_t)S + ts, arm, r, row + 7 * arm, q);
          for (int it = 0; it <= P.max_rounds; it++)
            if (ccmp::ik_round<false>(K, arm, P, pose, p->t_o7_R[arm], p->t_o7_p[arm], q, it < P.max_rounds)) { rounds = it; break; }
        }
        for (int i = 0; i < 7; i++) rec.q[c * 7 + i] = finite ? q[i] : __builtin_nan("");
        rec.rounds[c] = rounds;
        rec.d2[c] = finite ? ccmp::ik_seed_d2(q, row + 7 * arm) : __builtin_nan("");
      }
    }
  }
  return CCMP_OK;
}

// a scene given as the caller's arrays (the *_ref forms, no device): the tables ccmp_scene_create derives, on the heap for the call
struct RefScene {
  ccmp::scene_dev *H = new (std::nothrow) ccmp::scene_dev;
  ccmp::scene_arm_dev *A = new (std::nothrow) ccmp::scene_arm_dev;
  RefScene() = default;
  RefScene(const RefScene &) = delete;
  RefScene &operator=(const RefScene &) = delete;
  int tables(const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes, const uint32_t allowed[32])
  {
    return H && A ? scene_tables(spheres, n_spheres, boxes, n_boxes, allowed, *H, *A) : CCMP_ENOMEM;
  }
  ~RefScene() { delete H; delete A; }
};

// The seven staged pieces of a pose-IK call on host buffers, in the order they take their room: the vetted form adds its own behind them.
struct IkStaged {
  size_t T, C, pb, sb, off_p, off_s, off_q, off_w, off_ok, off_cq, off_cr;
  IkStaged(StagedCall &sg, size_t T_, int S, size_t C_, const double *cand_q, const int32_t *cand_rounds)
      : T(T_), C(C_), pb(T_ * 8 * sizeof(double)), sb(T_ * (size_t)S * 14 * sizeof(double))
  {
    off_p = sg.add(pb);
    off_s = sg.add(sb);
    off_q = sg.add(T * 14 * sizeof(double));
    off_w = sg.add(T * sizeof(int32_t));
    off_ok = sg.add(T);
    off_cq = sg.add(cand_q ? C * 7 * sizeof(double) : 0);
    off_cr = sg.add(cand_rounds ? C * sizeof(int32_t) : 0);
  }
  void up(StagedCall &sg, const double *poses, const double *seeds) const
  {
    sg.up(off_p, poses, pb);
    sg.up(off_s, seeds, sb);
  }
  void down(StagedCall &sg, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds) const
  {
    sg.down(q_out, off_q, T * 14 * sizeof(double));
    sg.down(which, off_w, T * sizeof(int32_t));
    sg.down(ok, off_ok, T);
    sg.down(cand_q, off_cq, C * 7 * sizeof(double));
    sg.down(cand_rounds, off_cr, C * sizeof(int32_t));
  }
};

// What the four device entry points check before the device guard, in this order: the handle, ik_checks, a vetted form's scene and
// margin, then — T == 0 answers CCMP_OK here and the caller returns it — the five required pointers.
int ik_prologue(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, size_t T, int S, bool vet, const ccmp_scene *scene, double margin,
                const double *target_poses, const double *seeds, const double *q_out, const uint8_t *ok, const int32_t *which, ccmp::ik_params *P)
{
  if (!ctx) return no_handle();
  { const int rc = ik_checks(p, opts, T, S, P); if (rc != CCMP_OK) return rc; }
  if (vet) { const int rc = ik_vet_checks(ctx, scene, margin); if (rc != CCMP_OK) return rc; }
  if (T == 0) return CCMP_OK;
  if (!target_poses || !seeds || !q_out || !ok || !which) return CCMP_EINVAL;
  return CCMP_OK;
}

}  // namespace

namespace ccmp_host {

int ik_checks(const ccmp_problem *p, const ccmp_ik_opts *opts, size_t T, int S, ccmp::ik_params *P)
{
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  ccmp_ik_opts o;
  if (opts) o = *opts; else ccmp_ik_opts_default(&o);
  if (o.restarts < 0 || o.restarts > CCMP_IK_MAX_RESTARTS || o.max_rounds < 1 || o.max_rounds > CCMP_IK_MAX_ROUNDS) return CCMP_EINVAL;
  if (!positive(o.eps) || !positive(o.lambda) || !positive(o.err_clamp) || !std::isfinite(o.sigma) || o.sigma < 0.0) return CCMP_EINVAL;
  if (S < 1 || S > CCMP_IK_MAX_SEEDS) return CCMP_EINVAL;
  if (T >= ((size_t)1 << 31) / ((size_t)S * 2 * (size_t)(1 + o.restarts))) return CCMP_EINVAL; // candidate indices are below 2^31
  P->eps = o.eps;
  P->lambda2 = o.lambda * o.lambda;
  P->err_clamp = o.err_clamp;
  P->sigma = o.sigma;
  P->restarts = o.restarts;
  P->max_rounds = o.max_rounds;
  return CCMP_OK;
}

size_t ik_candidates(size_t T, int S, const ccmp::ik_params &P) { return T * (size_t)S * 2 * (size_t)(1 + P.restarts); }

int ik_reserve(ccmp_ctx *ctx, size_t candidates)
{
  return grow_buffer(ctx, &ctx->ik_ws, &ctx->ik_ws_cap, candidates, candidates * (8 * sizeof(double) + sizeof(int32_t)));
}

// what the launches of a checked call start from (T > 0, the device current, the workspace at its size): the kernels' constants, t_o7, and
// the records' places in the context's workspace
struct IkRecords {
  ccmp_consts K;
  ccmp::ik_arms arms;
  size_t C;
  double *q, *d2;
  int32_t *rounds;
  IkRecords(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp::ik_params &P, size_t T, int S) : C(ik_candidates(T, S, P))
  {
    make_consts(*p, K);
    if (!ctx->stock_kernels) K.stock = K.twin_arms = K.rot_x0 = 0;
    memcpy(arms.R, p->t_o7_R, sizeof arms.R);
    memcpy(arms.p, p->t_o7_p, sizeof arms.p);
    q = (double *)ctx->ik_ws;
    d2 = q + C * 7;
    rounds = (int32_t *)(d2 + C);
  }
  // the nullable record outputs of a call
  int copy_out(double *cand_q, int32_t *cand_rounds, hipStream_t st) const
  {
    if (cand_q) HIP_TRY(hipMemcpyAsync(cand_q, q, C * 7 * sizeof(double), hipMemcpyDeviceToDevice, st));
    if (cand_rounds) HIP_TRY(hipMemcpyAsync(cand_rounds, rounds, C * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
    return CCMP_OK;
  }
};

int ik_launches(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp::ik_params &P, const double *poses, const double *seeds, size_t T, int S, uint64_t rng_seed,
                uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds, hipStream_t st)
{
  const IkRecords rec(ctx, p, P, T, S);
  const ccmp_launch::IkCall c{&rec.K, &rec.arms, &P, poses, seeds, T, S, rng_seed, first_index, rec.q, rec.rounds, rec.d2};
  HIP_TRY(ccmp_launch::ik_solve(c, st));
  HIP_TRY(ccmp_launch::ik_select(c, q_out, ok, which, st));
  return rec.copy_out(cand_q, cand_rounds, st);
}

int ik_vet_checks(const ccmp_ctx *ctx, const ccmp_scene *scene, double margin)
{
  if (!scene || scene->device != ctx->device || std::isnan(margin)) return CCMP_EINVAL;
  return CCMP_OK;
}

int ik_vetted_reserve(ccmp_ctx *ctx, size_t T, int S, const ccmp::ik_params &P)
{
  const size_t C = ik_candidates(T, S, P), TS = T * (size_t)S;
  { const int rc = ik_reserve(ctx, C); if (rc != CCMP_OK) return rc; }
  const size_t bytes = (C + TS * 16) * sizeof(double) + TS; // counted in bytes: the slots per candidate vary with the restarts
  return grow_buffer(ctx, &ctx->ik_vet_ws, &ctx->ik_vet_ws_cap, bytes, bytes);
}

// the vetted call: the same records, then their arm clearances, the per-arm rule per slot, the slots' full clearances, the pick
int ik_vetted_launches(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp::ik_params &P, const double *poses, const double *seeds, size_t T, int S,
                       uint64_t rng_seed, uint64_t first_index, const ccmp_scene *scene, double margin, double *q_out, uint8_t *ok, int32_t *which,
                       double *cand_q, int32_t *cand_rounds, double *cand_clear, double *slot_clear, double *clearance, hipStream_t st)
{
  const IkRecords rec(ctx, p, P, T, S);
  const size_t TS = T * (size_t)S;
  const int per = 1 + P.restarts;
  double *ws_clear = (double *)ctx->ik_vet_ws, *ws_slot_clear = ws_clear + rec.C, *ws_slot_q = ws_slot_clear + TS;
  uint8_t *ws_has = (uint8_t *)(ws_slot_q + TS * 14);
  const ccmp_launch::IkCall c{&rec.K, &rec.arms, &P, poses, seeds, T, S, rng_seed, first_index, rec.q, rec.rounds, rec.d2};
  HIP_TRY(ccmp_launch::ik_solve(c, st));
  HIP_TRY(ccmp_launch::ik_vet(&rec.K, scene->dev, scene->arm_dev, rec.q, rec.rounds, TS * (size_t)per, per, 0, 2, margin, ws_clear, nullptr, st));
  HIP_TRY(ccmp_launch::ik_assemble(rec.q, rec.rounds, rec.d2, ws_clear, TS, P.restarts, margin, ws_slot_q, ws_has, st));
  // si_->isValid(result) on the assembled rows: the existing clearance machinery (a slot without a state is a row of zeros, never reported)
  { const int rc = ccmp_clearance_batch(ctx, p, scene, ws_slot_q, nullptr, TS, margin, ws_slot_clear, nullptr, nullptr, st); if (rc != CCMP_OK) return rc; }
  HIP_TRY(ccmp_launch::ik_pick(ws_slot_q, ws_has, ws_slot_clear, T, S, margin, q_out, ok, which, clearance, slot_clear, st));
  if (cand_clear) HIP_TRY(hipMemcpyAsync(cand_clear, ws_clear, rec.C * sizeof(double), hipMemcpyDeviceToDevice, st));
  return rec.copy_out(cand_q, cand_rounds, st);
}

}  // namespace ccmp_host

extern "C" {

void ccmp_ik_opts_default(ccmp_ik_opts *o)
{
  if (!o) return;
  o->restarts = 14;
  o->max_rounds = 64;
  o->eps = 1e-5;
  o->lambda = 0.05;
  o->err_clamp = 0.5;
  o->sigma = 0.3;
}

int ccmp_pose_ik_ref(const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S, uint64_t rng_seed,
                     uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds)
{
  ccmp::ik_params P;
  { const int rc = ik_checks(p, opts, T, S, &P); if (rc != CCMP_OK) return rc; }
  if (T == 0) return CCMP_OK;
  if (!target_poses || !seeds || !q_out || !ok || !which) return CCMP_EINVAL;
  ccmp_consts K;
  make_consts(*p, K);
  const size_t C = ik_candidates(T, S, P);
  RefRecords rec;
  { const int rc = ref_records(p, K, P, target_poses, seeds, T, S, rng_seed, first_index, rec); if (rc != CCMP_OK) return rc; }
  for (size_t t = 0; t < T; t++) ccmp::ik_select(rec.q.data(), rec.rounds.data(), rec.d2.data(), t, S, P.restarts, q_out + t * 14, ok + t, which + t);
  if (cand_q) memcpy(cand_q, rec.q.data(), C * 7 * sizeof(double));
  if (cand_rounds) memcpy(cand_rounds, rec.rounds.data(), C * sizeof(int32_t));
  return CCMP_OK;
}

int ccmp_pose_ik_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                       uint64_t rng_seed, uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds,
                       void *hip_stream)
{
  ccmp::ik_params P;
  { const int rc = ik_prologue(ctx, p, opts, T, S, false, nullptr, 0.0, target_poses, seeds, q_out, ok, which, &P); if (rc != CCMP_OK || T == 0) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  { const int rc = ik_reserve(ctx, ik_candidates(T, S, P)); if (rc != CCMP_OK) return rc; }
  return ik_launches(ctx, p, P, target_poses, seeds, T, S, rng_seed, first_index, q_out, ok, which, cand_q, cand_rounds, (hipStream_t)hip_stream);
}

// the same on host buffers: synchronous on the context's stream
int ccmp_pose_ik_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                      uint64_t rng_seed, uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds)
{
  ccmp::ik_params P;
  { const int rc = ik_prologue(ctx, p, opts, T, S, false, nullptr, 0.0, target_poses, seeds, q_out, ok, which, &P); if (rc != CCMP_OK || T == 0) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t C = ik_candidates(T, S, P);
  StagedCall sg(ctx, __func__);
  const IkStaged o(sg, T, S, C, cand_q, cand_rounds);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; } // the staging block has its size before the candidates' workspace
  { const int rc = ik_reserve(ctx, C); if (rc != CCMP_OK) return rc; }
  o.up(sg, target_poses, seeds);
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ik_launches(ctx, p, P, sg.at<const double>(o.off_p), sg.at<const double>(o.off_s), T, S, rng_seed, first_index, sg.at<double>(o.off_q),
                     sg.at<uint8_t>(o.off_ok), sg.at<int32_t>(o.off_w), sg.at<double>(o.off_cq, cand_q), sg.at<int32_t>(o.off_cr, cand_rounds), ctx->stream);
  if (rc == CCMP_OK) o.down(sg, q_out, ok, which, cand_q, cand_rounds);
  return sg.finish(rc); // waits on the error path too: the staging block must be quiet
}

// ---- the vetted forms (csrc/ccmp_ik_vet.h): the proxy scene where the reference puts IKValid and si_->isValid --------------------------------

// IKValid(arm_index, sol) as a call of its own, on the host: the scene as the caller's arrays, no device
int ccmp_arm_clearance_ref(const ccmp_problem *p, const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes, const uint32_t allowed[32],
                           int arm, const double *q7, size_t B, double margin, double *clearance, uint8_t *free_out)
{
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (arm < 0 || arm > 1 || std::isnan(margin)) return CCMP_EINVAL;
  RefScene sc;
  { const int rc = sc.tables(spheres, n_spheres, boxes, n_boxes, allowed); if (rc != CCMP_OK) return rc; }
  if (B > 0 && (!q7 || !clearance)) return CCMP_EINVAL;
  ccmp_consts K;
  make_consts(*p, K);
  for (size_t i = 0; i < B; i++) {
    clearance[i] = ccmp::scene_arm_clearance(K, *sc.H, *sc.A, arm, q7 + i * 7);
    if (free_out) free_out[i] = (uint8_t)(clearance[i] > margin);
  }
  return CCMP_OK;
}

static int arm_clearance_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, int arm, size_t B, double margin)
{
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  { const int rc = ik_vet_checks(ctx, scene, margin); if (rc != CCMP_OK) return rc; }
  if (arm < 0 || arm > 1 || B >= ((size_t)1 << 32)) return CCMP_EINVAL; // four rows per block, block indices below 2^31
  return CCMP_OK;
}

int ccmp_arm_clearance_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, int arm, const double *q7, size_t B, double margin,
                             double *clearance, uint8_t *free_out, void *hip_stream)
{
  if (!ctx) return no_handle();
  { const int rc = arm_clearance_checks(ctx, p, scene, arm, B, margin); if (rc != CCMP_OK) return rc; }
  if (B == 0) return CCMP_OK;
  if (!q7 || !clearance) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_consts K;
  make_consts(*p, K);
  HIP_TRY(ccmp_launch::ik_vet(&K, scene->dev, scene->arm_dev, q7, nullptr, B, 0, arm, 1, margin, clearance, free_out, (hipStream_t)hip_stream));
  return CCMP_OK;
}

int ccmp_arm_clearance_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, int arm, const double *q7, size_t B, double margin,
                            double *clearance, uint8_t *free_out)
{
  if (!ctx) return no_handle();
  { const int rc = arm_clearance_checks(ctx, p, scene, arm, B, margin); if (rc != CCMP_OK) return rc; }
  if (B == 0) return CCMP_OK;
  if (!q7 || !clearance) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(ctx, __func__);
  const size_t off_q = sg.add(B * 7 * sizeof(double)), off_c = sg.add(B * sizeof(double)), off_f = sg.add(free_out ? B : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_q, q7, B * 7 * sizeof(double));
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ccmp_arm_clearance_batch(ctx, p, scene, arm, sg.at<const double>(off_q), B, margin, sg.at<double>(off_c), sg.at<uint8_t>(off_f, free_out), ctx->stream);
  if (rc == CCMP_OK) {
    sg.down(clearance, off_c, B * sizeof(double));
    sg.down(free_out, off_f, B);
  }
  return sg.finish(rc);
}

int ccmp_pose_ik_vetted_ref(const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                            uint64_t rng_seed, uint64_t first_index, const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes,
                            const uint32_t allowed[32], double margin, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds,
                            double *cand_clear, double *slot_clear, double *clearance)
{
  ccmp::ik_params P;
  { const int rc = ik_checks(p, opts, T, S, &P); if (rc != CCMP_OK) return rc; }
  if (std::isnan(margin)) return CCMP_EINVAL;
  RefScene scn;
  { const int rc = scn.tables(spheres, n_spheres, boxes, n_boxes, allowed); if (rc != CCMP_OK) return rc; }
  if (T == 0) return CCMP_OK;
  if (!target_poses || !seeds || !q_out || !ok || !which) return CCMP_EINVAL;
  ccmp_consts K;
  make_consts(*p, K);
  const size_t C = ik_candidates(T, S, P), TS = T * (size_t)S, per = (size_t)(1 + P.restarts);
  RefRecords rec;
  std::vector<double> cc, sq, sc;
  std::vector<uint8_t> has;
  { const int rc = ref_records(p, K, P, target_poses, seeds, T, S, rng_seed, first_index, rec); if (rc != CCMP_OK) return rc; }
  try { cc.resize(C); sq.resize(TS * 14); sc.resize(TS); has.resize(TS); } catch (...) { return CCMP_ENOMEM; }
  for (size_t c = 0; c < C; c++)
    cc[c] = rec.rounds[c] >= 0 ? ccmp::scene_arm_clearance(K, *scn.H, *scn.A, (int)((c / per) % 2), rec.q.data() + c * 7) : -__builtin_inf();
  for (size_t ts = 0; ts < TS; ts++) {
    has[ts] = ccmp::ik_vet_assemble(rec.q.data(), rec.rounds.data(), rec.d2.data(), cc.data(), ts, P.restarts, margin, sq.data() + ts * 14) ? 1 : 0;
    sc[ts] = ccmp::scene_state_clearance(K, *scn.H, sq.data() + ts * 14);
  }
  for (size_t t = 0; t < T; t++)
    ccmp::ik_vet_pick(sq.data(), has.data(), sc.data(), t, S, margin, q_out + t * 14, ok + t, which + t, clearance ? clearance + t : nullptr, slot_clear);
  if (cand_q) memcpy(cand_q, rec.q.data(), C * 7 * sizeof(double));
  if (cand_rounds) memcpy(cand_rounds, rec.rounds.data(), C * sizeof(int32_t));
  if (cand_clear) memcpy(cand_clear, cc.data(), C * sizeof(double));
  return CCMP_OK;
}

int ccmp_pose_ik_vetted_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                              uint64_t rng_seed, uint64_t first_index, const ccmp_scene *scene, double margin, double *q_out, uint8_t *ok, int32_t *which,
                              double *cand_q, int32_t *cand_rounds, double *cand_clear, double *slot_clear, double *clearance, void *hip_stream)
{
  ccmp::ik_params P;
  { const int rc = ik_prologue(ctx, p, opts, T, S, true, scene, margin, target_poses, seeds, q_out, ok, which, &P); if (rc != CCMP_OK || T == 0) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  { const int rc = ik_vetted_reserve(ctx, T, S, P); if (rc != CCMP_OK) return rc; }
  return ik_vetted_launches(ctx, p, P, target_poses, seeds, T, S, rng_seed, first_index, scene, margin, q_out, ok, which, cand_q, cand_rounds, cand_clear,
                            slot_clear, clearance, (hipStream_t)hip_stream);
}

// the same on host buffers: synchronous on the context's stream
int ccmp_pose_ik_vetted_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                             uint64_t rng_seed, uint64_t first_index, const ccmp_scene *scene, double margin, double *q_out, uint8_t *ok, int32_t *which,
                             double *cand_q, int32_t *cand_rounds, double *cand_clear, double *slot_clear, double *clearance)
{
  ccmp::ik_params P;
  { const int rc = ik_prologue(ctx, p, opts, T, S, true, scene, margin, target_poses, seeds, q_out, ok, which, &P); if (rc != CCMP_OK || T == 0) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t C = ik_candidates(T, S, P), TS = T * (size_t)S;
  StagedCall sg(ctx, __func__);
  const IkStaged o(sg, T, S, C, cand_q, cand_rounds);
  const size_t off_cc = sg.add(cand_clear ? C * sizeof(double) : 0), off_sc = sg.add(slot_clear ? TS * sizeof(double) : 0),
               off_cl = sg.add(clearance ? T * sizeof(double) : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; } // the staging block has its size before the workspaces
  { const int rc = ik_vetted_reserve(ctx, T, S, P); if (rc != CCMP_OK) return rc; }
  o.up(sg, target_poses, seeds);
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ik_vetted_launches(ctx, p, P, sg.at<const double>(o.off_p), sg.at<const double>(o.off_s), T, S, rng_seed, first_index, scene, margin,
                            sg.at<double>(o.off_q), sg.at<uint8_t>(o.off_ok), sg.at<int32_t>(o.off_w), sg.at<double>(o.off_cq, cand_q),
                            sg.at<int32_t>(o.off_cr, cand_rounds), sg.at<double>(off_cc, cand_clear), sg.at<double>(off_sc, slot_clear),
                            sg.at<double>(off_cl, clearance), ctx->stream);
  if (rc == CCMP_OK) {
    o.down(sg, q_out, ok, which, cand_q, cand_rounds);
    sg.down(cand_clear, off_cc, C * sizeof(double));
    sg.down(slot_clear, off_sc, TS * sizeof(double));
    sg.down(clearance, off_cl, T * sizeof(double));
  }
  return sg.finish(rc);
}

}  // extern "C"
