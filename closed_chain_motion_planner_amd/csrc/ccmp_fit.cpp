// ccmp_fit.cpp — time stamps fitted to the limits at the controller's rate, of the C ABI (include/ccmp.h: ccmp_path_fit_timestamps*,
// ccmp_fit_opts_default).  The rule is csrc/ccmp_fit.h.  A call is one begin launch, then per pass: the setpoints unit's status launch on the
// current stamps, ONE read of F status words and F tick counts (they size the measure launch and tell when no path is open), the setpoints
// unit's tangent launch, the measure and the dilate launches; it stops at the first pass with no open path.  Nothing else is read on the
// host and no allocation is sized by the ticks.  The _ref form runs the same rule text in plain loops, path by path.  The argument checks,
// the staging of the _host form, the tick ranges and the _ref form's tick and per-tick figures are csrc/ccmp_timed.h's, shared with the
// setpoints and jerk units; the pass loop is this unit's own.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_fit.h"
#include "ccmp_launch.h"
#include "ccmp_stage.h"
#include "ccmp_timed.h"

using namespace ccmp_host;
using ccmp::setpoint_limits;

namespace {

constexpr const char *kArenaWhat = "ccmp_path_fit_timestamps: hipMalloc";

int opts_ok(const ccmp_fit_opts &o)
{
  return finite_positive(o.period) && o.max_ticks >= 2 && o.aim > 0.0 && o.aim <= 1.0 && o.max_passes >= 0 ? CCMP_OK : CCMP_EINVAL;
}

// what every form checks of its arguments (the host and _ref forms check path_first too)
int input_checks(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                 const ccmp_fit_opts &o, const double *time_out, const int32_t *status, const int32_t *passes, const double *peak, const double *duration,
                 setpoint_limits *lim)
{
  { const int rc = opts_ok(o); if (rc != CCMP_OK) return rc; }
  { const int rc = limits_ok(vmax, amax, lim->vmax, lim->amax); if (rc != CCMP_OK) return rc; }
  if (total_rows > kMaxRows || F > kMaxRows) return CCMP_EINVAL;
  if (F && (!path_first || !status || !passes || !peak || !duration || (total_rows && (!rows || !time || !time_out)))) return CCMP_EINVAL;
  if (overlaps(time, total_rows * sizeof(double), time_out, total_rows * sizeof(double))) return CCMP_EINVAL;
  return CCMP_OK;
}

// the body of ccmp_path_fit_timestamps behind its checks, on device pointers; F > 0
int fit(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const setpoint_limits &lim,
        const ccmp_fit_opts &o, double *time_out, int32_t *status, int32_t *passes, double *peak, double *duration, double *factor, hipStream_t st)
{
  const size_t R = total_rows ? total_rows : 1;
  CallArena mem(ctx, kArenaWhat);
  int32_t *d_sp = mem.array<int32_t>(F), *d_ticks = mem.array<int32_t>(F), *d_first = mem.array<int32_t>(F + 1);
  double *tangent = mem.array<double>(R * 14);
  unsigned long long *S = mem.array<unsigned long long>(R), *A = mem.array<unsigned long long>(R);
  if (!mem.ok()) return CCMP_EHIP;
  std::vector<int32_t> state(F), ticks(F), first(F + 1, 0);
  int rc = CCMP_OK;
  hipError_t e = hipMemsetAsync(S, 0, R * sizeof(unsigned long long), st);
  if (e == hipSuccess) e = hipMemsetAsync(A, 0, R * sizeof(unsigned long long), st);
  if (e == hipSuccess) e = ccmp_launch::fit_begin(path_first, time, F, total_rows, time_out, status, passes, peak, duration, st);
  // pass p measures the paths that p dilations have left open; the pass behind the last dilation closes them all
  for (long long pass = 0; rc == CCMP_OK && e == hipSuccess && pass <= (long long)o.max_passes + 1; pass++) {
    e = ccmp_launch::setpoints_status(rows, path_first, time_out, F, total_rows, o.period, o.max_ticks, d_sp, d_ticks, st);
    if (e == hipSuccess) e = hipMemcpyAsync(state.data(), status, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(ticks.data(), d_ticks, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) break;
    bool open = false;
    for (size_t f = 0; f < F; f++) open = open || state[f] == ccmp::kFitOpen;
    int64_t M = 0; // the tick intervals of the open paths: N - 1 of an OK path, none of a path this pass's status ends
    rc = tick_ranges(F, o.max_ticks, 1, [&](size_t f) { return (int64_t)(state[f] == ccmp::kFitOpen ? ticks[f] : 0); }, &first, &M);
    if (rc != CCMP_OK || !open) break;
    if (M) {
      e = hipMemcpyAsync(d_first, first.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
      if (e == hipSuccess) e = ccmp_launch::setpoints_tangent(rows, path_first, time_out, F, total_rows, d_sp, tangent, st);
      if (e == hipSuccess) e = ccmp_launch::fit_measure(rows, path_first, time_out, tangent, d_first, F, (size_t)M, total_rows, o.period, lim, S, A, st);
    }
    if (e == hipSuccess) e = ccmp_launch::fit_dilate(path_first, d_sp, F, o.aim, o.max_passes, time_out, S, A, status, passes, peak, duration, st);
  }
  if (rc == CCMP_OK && e == hipSuccess && factor && total_rows) e = ccmp_launch::fit_factor(path_first, F, total_rows, time, time_out, factor, st);
  const hipError_t es = hipStreamSynchronize(st); // the call is synchronous: the host arrays above and the arena go when it returns
  if (rc == CCMP_OK && e != hipSuccess) rc = hip_fail(e, "ccmp_path_fit_timestamps");
  if (rc == CCMP_OK && es != hipSuccess) rc = hip_fail(es, "ccmp_path_fit_timestamps: hipStreamSynchronize");
  return rc;
}

// one path of the _ref form: t [R] is dilated in place; S, A, w are the caller's scratch
void fit_path_ref(const double *r, double *t, size_t R, const setpoint_limits &lim, const ccmp_fit_opts &o, std::vector<double> &S, std::vector<double> &A,
                  std::vector<double> &w, int32_t *status, int32_t *passes, double *peak, double *duration)
{
  *passes = 0;
  peak[0] = peak[1] = 0.0;
  for (;;) {
    // status and N of (rows, t): the setpoints rule's own host form, as a sizing call
    const int32_t pf[2] = {0, (int32_t)R};
    const ccmp_setpoint_opts so = {o.period, o.max_ticks};
    int32_t tf[2] = {0, 0}, st = ccmp::kSetpointsEmpty;
    (void)ccmp_setpoints_ref(r, pf, t, 1, R, lim.vmax, lim.amax, &so, tf, &st, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    const int32_t n = tf[1];
    if (st != ccmp::kSetpointsOk) {
      *status = st;
      *duration = ccmp::fit_closed_duration(st, R ? t[R - 1] : 0.0);
      return;
    }
    const int64_t N = n;
    const double D = t[R - 1];
    w.resize(R * 14);
    (void)ccmp_setpoint_tangents_ref(r, t, R, w.data());
    S.assign(R, 0.0);
    A.assign(R, 0.0);
    double v0[14], v1[14], x[14], tau0 = 0.0; // (x: the position half, never used)
    int k0 = 0;
    for (int c = 0; c < 14; c++) v0[c] = 0.0;
    for (int64_t j = 0; j + 1 < N; j++) { // the tick interval (j, j + 1)
      double tau1;
      const int k1 = ref_tick(r, w.data(), t, R, j + 1, N, o.period, D, &tau1, x, v1);
      if (j + 1 == N - 1)
        for (int c = 0; c < 14; c++) v1[c] = 0.0; // the last tick is at rest: only its bracket counts
      if (j == 0) k0 = k1;
      const double width = tau1 - tau0;
      const TickFigures g = tick_figures(v0, v1, width, lim.vmax, lim.amax);
      if (!g.speed_nan && g.speed > S[k0]) S[k0] = g.speed;
      if (width > 0.0 && !g.acc_nan)
        for (int k = k0; k <= k1; k++)
          if (g.acc > A[k]) A[k] = g.acc;
      for (int c = 0; c < 14; c++) v0[c] = v1[c];
      tau0 = tau1;
      k0 = k1;
    }
    double Ps = 0.0, Pa = 0.0;
    for (size_t k = 1; k < R; k++) {
      if (S[k] > Ps) Ps = S[k];
      if (A[k] > Pa) Pa = A[k];
    }
    peak[0] = Ps;
    peak[1] = Pa;
    const bool done = ccmp::fit_done(Ps, Pa);
    if (done || *passes >= o.max_passes) {
      *status = done ? ccmp::kFitFitted : ccmp::kFitPasses;
      *duration = D;
      return;
    }
    double acc = 0.0, prev = t[0];
    t[0] = 0.0;
    for (size_t k = 1; k < R; k++) {
      const double tk = t[k];
      acc = acc + ccmp::fit_width(prev, tk, ccmp::fit_factor(S[k], A[k], o.aim));
      t[k] = acc;
      prev = tk;
    }
    *passes += 1;
  }
}

}  // namespace

extern "C" {

void ccmp_fit_opts_default(ccmp_fit_opts *opts)
{
  if (!opts) return;
  opts->period = 0.001;
  opts->max_ticks = 65536;
  opts->aim = 0.95;
  opts->max_passes = 8;
}

int ccmp_path_fit_timestamps(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows,
                             const double *vmax, const double *amax, const ccmp_fit_opts *opts, double *time_out, int32_t *status, int32_t *passes,
                             double *peak, double *duration, double *factor, void *hip_stream)
{
  if (!ctx) return no_handle();
  const ccmp_fit_opts o = opts_or(opts, ccmp_fit_opts_default);
  setpoint_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, o, time_out, status, passes, peak, duration, &lim); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  return fit(ctx, rows, path_first, time, F, total_rows, lim, o, time_out, status, passes, peak, duration, factor, (hipStream_t)hip_stream);
}

int ccmp_path_fit_timestamps_host(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows,
                                  const double *vmax, const double *amax, const ccmp_fit_opts *opts, double *time_out, int32_t *status, int32_t *passes,
                                  double *peak, double *duration, double *factor)
{
  if (!ctx) return no_handle();
  const ccmp_fit_opts o = opts_or(opts, ccmp_fit_opts_default);
  setpoint_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, o, time_out, status, passes, peak, duration, &lim); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t R = total_rows ? total_rows : 1;
  CallArena mem(ctx, "ccmp_path_fit_timestamps_host: hipMalloc"); // the staging is memory of this call
  const PathStage d(mem, F, total_rows);
  double *d_out = mem.array<double>(R), *d_factor = mem.array<double>(R), *d_peak = mem.array<double>(F * 2), *d_dur = mem.array<double>(F);
  int32_t *d_status = mem.array<int32_t>(F), *d_passes = mem.array<int32_t>(F);
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  d.up(sg, rows, time, path_first, F, total_rows);
  sg.up(d_out, time_out, total_rows * sizeof(double)); // the caller's values go up first: rows outside every path stay the caller's
  sg.up(d_factor, factor, total_rows * sizeof(double));
  { const int rc = sg.finish(CCMP_OK); if (rc != CCMP_OK) return rc; }
  { const int rc = fit(ctx, d.rows, d.path_first, d.time, F, total_rows, lim, o, d_out, d_status, d_passes, d_peak, d_dur, factor ? d_factor : nullptr, ctx->stream);
    if (rc != CCMP_OK) return sg.finish(rc); }
  sg.down(time_out, d_out, total_rows * sizeof(double));
  sg.down(factor, d_factor, total_rows * sizeof(double));
  sg.down(status, d_status, F * sizeof(int32_t));
  sg.down(passes, d_passes, F * sizeof(int32_t));
  sg.down(peak, d_peak, F * 2 * sizeof(double));
  sg.down(duration, d_dur, F * sizeof(double));
  return sg.finish(CCMP_OK);
}

int ccmp_path_fit_timestamps_ref(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax,
                                 const double *amax, const ccmp_fit_opts *opts, double *time_out, int32_t *status, int32_t *passes, double *peak,
                                 double *duration, double *factor)
{
  const ccmp_fit_opts o = opts_or(opts, ccmp_fit_opts_default);
  setpoint_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, o, time_out, status, passes, peak, duration, &lim); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  std::vector<double> S, A, w;
  for (size_t f = 0; f < F; f++) {
    const size_t a = (size_t)path_first[f], R = (size_t)(path_first[f + 1] - path_first[f]);
    if (R) memcpy(time_out + a, time + a, R * sizeof(double));
    fit_path_ref(rows + a * 14, time_out + a, R, lim, o, S, A, w, status + f, passes + f, peak + f * 2, duration + f);
    if (factor)
      for (size_t i = 0; i < R; i++) factor[a + i] = i == 0 ? 1.0 : ccmp::fit_ratio(time[a + i - 1], time[a + i], time_out[a + i - 1], time_out[a + i]);
  }
  return CCMP_OK;
}

}  // extern "C"
