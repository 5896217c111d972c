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
#include "ccmp_launch.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

namespace {

bool positive(double v) { return std::isfinite(v) && v > 0.0; }

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

// the launches of a checked call whose workspace has its size (T > 0, the device current)
int ik_launches(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp::ik_params &P, const double *poses, const double *seeds, size_t T, int S, uint64_t rng_seed,
                uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds, hipStream_t st)
{
  ccmp_consts K;
  make_consts(*p, K);
  if (!ctx->stock_kernels) K.stock = K.twin_arms = K.rot_x0 = 0;
  ccmp::ik_arms arms;
  memcpy(arms.R, p->t_o7_R, sizeof arms.R);
  memcpy(arms.p, p->t_o7_p, sizeof arms.p);
  const size_t C = ik_candidates(T, S, P);
  double *rec_q = (double *)ctx->ik_ws, *rec_d2 = rec_q + C * 7;
  int32_t *rec_rounds = (int32_t *)(rec_d2 + C);
  const ccmp_launch::IkCall c{&K, &arms, &P, poses, seeds, T, S, rng_seed, first_index, rec_q, rec_rounds, rec_d2};
  HIP_TRY(ccmp_launch::ik_solve(c, st));
  HIP_TRY(ccmp_launch::ik_select(c, q_out, ok, which, st));
  if (cand_q) HIP_TRY(hipMemcpyAsync(cand_q, rec_q, C * 7 * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (cand_rounds) HIP_TRY(hipMemcpyAsync(cand_rounds, rec_rounds, C * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  return CCMP_OK;
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
  const size_t C = ik_candidates(T, S, P), per = (size_t)(1 + P.restarts);
  std::vector<double> rec_q, rec_d2;
  std::vector<int32_t> rec_rounds;
  try { rec_q.resize(C * 7); rec_d2.resize(C); rec_rounds.resize(C); } catch (...) { return CCMP_ENOMEM; }
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
        for (int i = 0; i < 7; i++) rec_q[c * 7 + i] = finite ? q[i] : __builtin_nan("");
        rec_rounds[c] = rounds;
        rec_d2[c] = finite ? ccmp::ik_seed_d2(q, row + 7 * arm) : __builtin_nan("");
      }
    }
  }
  for (size_t t = 0; t < T; t++) ccmp::ik_select(rec_q.data(), rec_rounds.data(), rec_d2.data(), t, S, P.restarts, q_out + t * 14, ok + t, which + t);
  if (cand_q) memcpy(cand_q, rec_q.data(), C * 7 * sizeof(double));
  if (cand_rounds) memcpy(cand_rounds, rec_rounds.data(), C * sizeof(int32_t));
  return CCMP_OK;
}

int ccmp_pose_ik_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                       uint64_t rng_seed, uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds,
                       void *hip_stream)
{
  if (!ctx) return no_handle();
  ccmp::ik_params P;
  { const int rc = ik_checks(p, opts, T, S, &P); if (rc != CCMP_OK) return rc; }
  if (T == 0) return CCMP_OK;
  if (!target_poses || !seeds || !q_out || !ok || !which) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  { const int rc = ik_reserve(ctx, ik_candidates(T, S, P)); if (rc != CCMP_OK) return rc; }
  return ik_launches(ctx, p, P, target_poses, seeds, T, S, rng_seed, first_index, q_out, ok, which, cand_q, cand_rounds, (hipStream_t)hip_stream);
}

// the same on host buffers: synchronous on the context's stream
int ccmp_pose_ik_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                      uint64_t rng_seed, uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds)
{
  if (!ctx) return no_handle();
  ccmp::ik_params P;
  { const int rc = ik_checks(p, opts, T, S, &P); if (rc != CCMP_OK) return rc; }
  if (T == 0) return CCMP_OK;
  if (!target_poses || !seeds || !q_out || !ok || !which) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t C = ik_candidates(T, S, P), pb = T * 8 * sizeof(double), sb = T * (size_t)S * 14 * sizeof(double);
  StagedCall sg(ctx, __func__);
  const size_t off_p = sg.add(pb), off_s = sg.add(sb), off_q = sg.add(T * 14 * sizeof(double)), off_w = sg.add(T * sizeof(int32_t)), off_ok = sg.add(T),
               off_cq = sg.add(cand_q ? C * 7 * sizeof(double) : 0), off_cr = sg.add(cand_rounds ? C * sizeof(int32_t) : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; } // the staging block has its size before the candidates' workspace
  { const int rc = ik_reserve(ctx, C); if (rc != CCMP_OK) return rc; }
  sg.up(off_p, target_poses, pb);
  sg.up(off_s, seeds, sb);
  int rc = CCMP_OK;
  if (sg.copy_ok())
    rc = ik_launches(ctx, p, P, sg.at<const double>(off_p), sg.at<const double>(off_s), T, S, rng_seed, first_index, sg.at<double>(off_q), sg.at<uint8_t>(off_ok),
                     sg.at<int32_t>(off_w), sg.at<double>(off_cq, cand_q), sg.at<int32_t>(off_cr, cand_rounds), ctx->stream);
  if (rc == CCMP_OK) {
    sg.down(q_out, off_q, T * 14 * sizeof(double));
    sg.down(which, off_w, T * sizeof(int32_t));
    sg.down(ok, off_ok, T);
    sg.down(cand_q, off_cq, C * 7 * sizeof(double));
    sg.down(cand_rounds, off_cr, C * sizeof(int32_t));
  }
  return sg.finish(rc); // waits on the error path too: the staging block must be quiet
}

}  // extern "C"
