// ccmp_setpoints.cpp — controller-rate setpoints and the execution audit of the C ABI (include/ccmp.h: ccmp_path_setpoints*, ccmp_setpoints_*,
// ccmp_setpoints_ref, ccmp_setpoint_tangents_ref).  The rule is csrc/ccmp_setpoints.h.  A call is one status launch, one read of F status
// words and F tick counts (they size the result), then the tangent and sample launches, the function, is-satisfied and — with a scene —
// clearance entry points ONCE each over all ticks of all paths, and the peak launch.  The _ref forms run the same rule text in plain loops.
// What this unit has in common with the fit and jerk units' host code is csrc/ccmp_timed.h: the argument checks, the staging of the _host
// form, the tick ranges, the delivery tail (deliver: this unit hands it its tangent + sample and its peak launches) and the _ref loops.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_launch.h"
#include "ccmp_resident.h"
#include "ccmp_setpoints.h"
#include "ccmp_stage.h"
#include "ccmp_timed.h"

using namespace ccmp_host;
using ccmp::setpoint_limits;

/* the result of ccmp_path_setpoints: one allocation, the arrays point into it */
struct ccmp_setpoints {
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  size_t F = 0, ticks = 0;
  void *block = nullptr;
  double *q = nullptr, *qd = nullptr, *tau = nullptr, *f = nullptr, *clearance = nullptr, *peak = nullptr, *stretch = nullptr;
  int32_t *tick_first = nullptr, *status = nullptr, *peak_tick = nullptr, *counts = nullptr;
  uint8_t *satisfied = nullptr;
};

namespace {

constexpr const char *kArenaWhat = "ccmp_path_setpoints: hipMalloc";

int opts_ok(const ccmp_setpoint_opts &o) { return finite_positive(o.period) && o.max_ticks >= 2 ? CCMP_OK : CCMP_EINVAL; }

// what every form checks of its arguments (the host and _ref forms check path_first too)
int input_checks(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                 const ccmp_setpoint_opts &o, setpoint_limits *lim)
{
  { const int rc = opts_ok(o); if (rc != CCMP_OK) return rc; }
  { const int rc = limits_ok(vmax, amax, lim->vmax, lim->amax); if (rc != CCMP_OK) return rc; }
  if (total_rows > kMaxRows || F > kMaxRows) return CCMP_EINVAL;
  if (F && (!path_first || (total_rows && (!rows || !time)))) return CCMP_EINVAL;
  return CCMP_OK;
}

int make_handle(ccmp_ctx *ctx, size_t F, size_t ticks, ccmp_setpoints **out)
{
  ccmp_setpoints *h = new (std::nothrow) ccmp_setpoints();
  if (!h) return CCMP_ENOMEM;
  h->F = F;
  h->ticks = ticks;
  const size_t M = ticks ? ticks : 1, P = F + 1;
  ResultBlock b;
  const size_t o_q = b.take(M * 14 * sizeof(double)), o_qd = b.take(M * 14 * sizeof(double)), o_tau = b.take(M * sizeof(double)),
               o_f = b.take(M * 2 * sizeof(double)), o_cl = b.take(M * sizeof(double)), o_peak = b.take(P * ccmp::kPeaks * sizeof(double)),
               o_str = b.take(P * sizeof(double)), o_tf = b.take(P * sizeof(int32_t)), o_st = b.take(P * sizeof(int32_t)),
               o_pt = b.take(P * ccmp::kPeaks * sizeof(int32_t)), o_cnt = b.take(P * 2 * sizeof(int32_t)), o_sat = b.take(M);
  { const int rc = b.alloc(h, ctx, kArenaWhat); if (rc != CCMP_OK) { delete h; return rc; } }
  h->q = b.at<double>(o_q);
  h->qd = b.at<double>(o_qd);
  h->tau = b.at<double>(o_tau);
  h->f = b.at<double>(o_f);
  h->clearance = b.at<double>(o_cl);
  h->peak = b.at<double>(o_peak);
  h->stretch = b.at<double>(o_str);
  h->tick_first = b.at<int32_t>(o_tf);
  h->status = b.at<int32_t>(o_st);
  h->peak_tick = b.at<int32_t>(o_pt);
  h->counts = b.at<int32_t>(o_cnt);
  h->satisfied = b.at<uint8_t>(o_sat);
  *out = h;
  return CCMP_OK;
}

// the body of ccmp_path_setpoints behind its checks, on device pointers.  On any failure *out stays NULL.
int setpoints(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first, const double *time,
              size_t F, size_t total_rows, const setpoint_limits &lim, const ccmp_setpoint_opts &o, ccmp_setpoints **out, hipStream_t st)
{
  std::vector<int32_t> status(F ? F : 1), ticks(F ? F : 1), tick_first(F + 1, 0);
  CallArena mem(ctx, kArenaWhat);
  int32_t *d_status = nullptr;
  if (F) {
    d_status = mem.array<int32_t>(F);
    int32_t *d_ticks = mem.array<int32_t>(F);
    if (!mem.ok()) return CCMP_EHIP;
    hipError_t e = ccmp_launch::setpoints_status(rows, path_first, time, F, total_rows, o.period, o.max_ticks, d_status, d_ticks, st);
    if (e == hipSuccess) e = hipMemcpyAsync(status.data(), d_status, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ticks.data(), d_ticks, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    HIP_TRY(e);
    HIP_TRY(es);
  }
  int64_t M = 0;
  { const int rc = tick_ranges(F, o.max_ticks, 0, [&](size_t f) { return (int64_t)ticks[f]; }, &tick_first, &M); if (rc != CCMP_OK) return rc; }
  double *tangent = M ? mem.array<double>((total_rows ? total_rows : 1) * 14) : nullptr;
  if (!mem.ok()) return CCMP_EHIP;

  ccmp_setpoints *h = nullptr;
  { const int rc = make_handle(ctx, F, (size_t)M, &h); if (rc != CCMP_OK) return rc; }
  return deliver(
      ctx, p, scene, margin, h, tick_first, d_status, "ccmp_path_setpoints", st,
      [&] {
        const hipError_t e = ccmp_launch::setpoints_tangent(rows, path_first, time, F, total_rows, d_status, tangent, st);
        return e != hipSuccess ? e
                               : ccmp_launch::setpoints_sample(rows, path_first, time, tangent, d_status, h->tick_first, F, h->ticks, total_rows, o.period, h->q, h->qd,
                                                               h->tau, h->clearance, st);
      },
      [&] {
        return ccmp_launch::setpoints_peak(h->qd, h->tau, h->f, h->satisfied, h->clearance, h->tick_first, F, h->ticks, lim, margin, h->peak, h->peak_tick, h->counts,
                                           h->stretch, st);
      },
      out);
}

int result_copy(ccmp_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied, double *clearance, int32_t *status,
                double *peak, int32_t *peak_tick, int32_t *counts, double *stretch, hipMemcpyKind how, hipStream_t st)
{
  const size_t M = h->ticks, F = h->F;
  if (q && M) HIP_TRY(hipMemcpyAsync(q, h->q, M * 14 * sizeof(double), how, st));
  if (qd && M) HIP_TRY(hipMemcpyAsync(qd, h->qd, M * 14 * sizeof(double), how, st));
  if (tau && M) HIP_TRY(hipMemcpyAsync(tau, h->tau, M * sizeof(double), how, st));
  if (tick_first) HIP_TRY(hipMemcpyAsync(tick_first, h->tick_first, (F + 1) * sizeof(int32_t), how, st));
  if (f && M) HIP_TRY(hipMemcpyAsync(f, h->f, M * 2 * sizeof(double), how, st));
  if (satisfied && M) HIP_TRY(hipMemcpyAsync(satisfied, h->satisfied, M, how, st));
  if (clearance && M) HIP_TRY(hipMemcpyAsync(clearance, h->clearance, M * sizeof(double), how, st));
  if (status && F) HIP_TRY(hipMemcpyAsync(status, h->status, F * sizeof(int32_t), how, st));
  if (peak && F) HIP_TRY(hipMemcpyAsync(peak, h->peak, F * ccmp::kPeaks * sizeof(double), how, st));
  if (peak_tick && F) HIP_TRY(hipMemcpyAsync(peak_tick, h->peak_tick, F * ccmp::kPeaks * sizeof(int32_t), how, st));
  if (counts && F) HIP_TRY(hipMemcpyAsync(counts, h->counts, F * 2 * sizeof(int32_t), how, st));
  if (stretch && F) HIP_TRY(hipMemcpyAsync(stretch, h->stretch, F * sizeof(double), how, st));
  return CCMP_OK;
}

// the tangents of one path with ordered, finite stamps: w [R][14]
void tangents(const double *q, const double *t, size_t R, double *w)
{
  for (size_t i = 0; i < R; i++)
    for (int c = 0; c < 14; c++) {
      double v = 0.0;
      if (i > 0 && i + 1 < R) {
        const double hp = t[i] - t[i - 1], h = t[i + 1] - t[i];
        v = ccmp::setpoint_tangent(hp, h, ccmp::setpoint_slope(q[(i - 1) * 14 + c], q[i * 14 + c], hp), ccmp::setpoint_slope(q[i * 14 + c], q[(i + 1) * 14 + c], h));
      }
      w[i * 14 + c] = v;
    }
}

}  // namespace

extern "C" {

void ccmp_setpoint_opts_default(ccmp_setpoint_opts *opts)
{
  if (!opts) return;
  opts->period = 0.001;
  opts->max_ticks = 65536;
}

int ccmp_path_setpoints(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first,
                        const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax, const ccmp_setpoint_opts *opts,
                        ccmp_setpoints **out, void *hip_stream)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out) return CCMP_EINVAL;
  { const int rc = device_checks(ctx, p, scene, margin); if (rc != CCMP_OK) return rc; }
  const ccmp_setpoint_opts o = opts_or(opts, ccmp_setpoint_opts_default);
  setpoint_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, o, &lim); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  return setpoints(ctx, p, scene, margin, rows, path_first, time, F, total_rows, lim, o, out, (hipStream_t)hip_stream);
}

int ccmp_path_setpoints_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first,
                             const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax, const ccmp_setpoint_opts *opts,
                             ccmp_setpoints **out)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out) return CCMP_EINVAL;
  { const int rc = device_checks(ctx, p, scene, margin); if (rc != CCMP_OK) return rc; }
  const ccmp_setpoint_opts o = opts_or(opts, ccmp_setpoint_opts_default);
  setpoint_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, o, &lim); if (rc != CCMP_OK) return rc; }
  if (F) { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  CallArena mem(ctx, "ccmp_path_setpoints_host: hipMalloc"); // the staging is memory of this call
  const PathStage d(mem, F, total_rows);
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  d.up(sg, rows, time, path_first, F, total_rows);
  { const int rc = sg.finish(CCMP_OK); if (rc != CCMP_OK) return rc; }
  return setpoints(ctx, p, scene, margin, d.rows, d.path_first, d.time, F, total_rows, lim, o, out, ctx->stream);
}

int ccmp_setpoints_info(const ccmp_setpoints *h, size_t *F, size_t *ticks)
{
  if (!h) return CCMP_EINVAL;
  if (F) *F = h->F;
  if (ticks) *ticks = h->ticks;
  return CCMP_OK;
}

int ccmp_setpoints_copy(ccmp_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied, double *clearance,
                        int32_t *status, double *peak, int32_t *peak_tick, int32_t *counts, double *stretch, void *hip_stream)
{
  if (!h) return no_handle();
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  return result_copy(h, q, qd, tau, tick_first, f, satisfied, clearance, status, peak, peak_tick, counts, stretch, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream);
}

int ccmp_setpoints_copy_host(ccmp_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied, double *clearance,
                             int32_t *status, double *peak, int32_t *peak_tick, int32_t *counts, double *stretch)
{
  if (!h) return no_handle();
  if (!ccmp_host::context_alive(h->ctx)) return CCMP_EINVAL;
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(h->ctx, __func__); // nothing staged: the copies come straight from the result
  const int rc = result_copy(h, q, qd, tau, tick_first, f, satisfied, clearance, status, peak, peak_tick, counts, stretch, hipMemcpyDeviceToHost, h->ctx->stream);
  return sg.finish(rc);
}

void ccmp_setpoints_destroy(ccmp_setpoints *h) { result_destroy(h); }

int ccmp_setpoints_ref(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                       const ccmp_setpoint_opts *opts, int32_t *tick_first, int32_t *status, double *q, double *qd, double *tau, double *peak,
                       int32_t *peak_tick, double *stretch)
{
  const ccmp_setpoint_opts o = opts_or(opts, ccmp_setpoint_opts_default);
  setpoint_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, o, &lim); if (rc != CCMP_OK) return rc; }
  if (!tick_first || (F && !status)) return CCMP_EINVAL;
  if (F) { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  // first pass: the statuses and the tick counts (all a sizing call asks for); nothing is written before the total is known to fit
  std::vector<int32_t> st(F ? F : 1), first(F + 1, 0);
  int64_t M = 0;
  for (size_t f = 0; f < F; f++) {
    const size_t a = (size_t)path_first[f], R = (size_t)(path_first[f + 1] - path_first[f]);
    const double *r = rows + a * 14, *t = time + a;
    first[f] = (int32_t)M;
    int32_t n = 0;
    if (R == 0) {
      st[f] = ccmp::kSetpointsEmpty;
    } else {
      bool nonfinite = false, unordered = false;
      for (size_t w = 0; w < R * 14; w++) nonfinite = nonfinite || !ccmp::setpoint_finite(r[w]);
      for (size_t i = 0; i < R; i++) nonfinite = nonfinite || !ccmp::setpoint_finite(t[i]);
      if (!nonfinite) {
        unordered = t[0] != 0.0;
        for (size_t i = 0; i + 1 < R; i++) {
          bool moved = false;
          for (int c = 0; c < 14; c++) moved = moved || r[i * 14 + c] != r[(i + 1) * 14 + c];
          unordered = unordered || ccmp::setpoint_unordered(t[i], t[i + 1], moved);
        }
      }
      st[f] = ccmp::setpoint_status(nonfinite, unordered, (int64_t)R, nonfinite ? 0.0 : t[R - 1], o.period, o.max_ticks, &n);
    }
    M += n;
    if ((uint64_t)M > kMaxRows) return CCMP_EOVERFLOW;
  }
  first[F] = (int32_t)M;
  memcpy(tick_first, first.data(), (F + 1) * sizeof(int32_t));
  if (F) memcpy(status, st.data(), F * sizeof(int32_t));
  if (!q && !qd && !tau && !peak && !peak_tick && !stretch) return CCMP_OK;

  std::vector<double> w, x, xd, at;
  for (size_t f = 0; f < F; f++) {
    const size_t a = (size_t)path_first[f], R = (size_t)(path_first[f + 1] - path_first[f]), g0 = (size_t)first[f], N = (size_t)(first[f + 1] - first[f]);
    const double *r = rows + a * 14, *t = time + a;
    x.assign(N * 14, 0.0); xd.assign(N * 14, 0.0); at.assign(N, 0.0);
    if (st[f] == ccmp::kSetpointsPoint) {
      memcpy(x.data(), r, 14 * sizeof(double));
    } else if (st[f] == ccmp::kSetpointsOk) {
      const double D = t[R - 1];
      w.resize(R * 14);
      tangents(r, t, R, w.data());
      memcpy(x.data(), r, 14 * sizeof(double));
      memcpy(x.data() + (N - 1) * 14, r + (R - 1) * 14, 14 * sizeof(double));
      at[N - 1] = D;
      for (size_t j = 1; j + 1 < N; j++) (void)ref_tick(r, w.data(), t, R, (int64_t)j, (int64_t)N, o.period, D, &at[j], &x[j * 14], &xd[j * 14]);
    }
    double pv[2] = {0.0, 0.0};
    int32_t pj[2] = {-1, -1};
    speed_acc_peaks(xd.data(), (int64_t)N, [&](int64_t j) { return at[j + 1] - at[j]; }, lim.vmax, lim.amax, pv, pj);
    if (q && N) memcpy(q + g0 * 14, x.data(), N * 14 * sizeof(double));
    if (qd && N) memcpy(qd + g0 * 14, xd.data(), N * 14 * sizeof(double));
    if (tau && N) memcpy(tau + g0, at.data(), N * sizeof(double));
    if (peak) { peak[f * 2] = pv[0]; peak[f * 2 + 1] = pv[1]; }
    if (peak_tick) { peak_tick[f * 2] = pj[0]; peak_tick[f * 2 + 1] = pj[1]; }
    if (stretch) stretch[f] = ccmp::setpoint_stretch(pv[0], pv[1]);
  }
  return CCMP_OK;
}

int ccmp_setpoint_tangents_ref(const double *rows, const double *time, size_t R, double *w_out)
{
  if (R > kMaxRows || (R && (!rows || !time || !w_out))) return CCMP_EINVAL;
  tangents(rows, time, R, w_out);
  return CCMP_OK;
}

}  // extern "C"
