// ccmp_retime.cpp — resample and time stamps of the C ABI (include/ccmp.h: ccmp_path_resample, ccmp_sampled_paths_*, ccmp_path_timestamps*,
// ccmp_arc_bracket_ref, ccmp_resample_targets_ref).  The rule is csrc/ccmp_retime.h.  Resampling reads a dense result where the library
// keeps it: one status launch, one read of what decides the statuses and the row counts (path_first, the lengths, seg_first / seg_ok and
// F status words), then a bracket launch, the projector's batch entry on ALL blends of all paths in one call, a pick launch and the dense
// unit's arc kernel on the new rows.  Time stamps are four launches on the caller's stream and read nothing on the host.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_launch.h"
#include "ccmp_pair_tests.h"
#include "ccmp_resident.h"
#include "ccmp_retime.h"
#include "ccmp_stage.h"
#include "ccmp_timed.h"

using namespace ccmp_host;
using ccmp::retime_limits;

/* the result of ccmp_path_resample: one allocation, the arrays point into it */
struct ccmp_sampled_paths {
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  size_t F = 0, rows = 0;
  void *block = nullptr;
  double *d_rows = nullptr, *arc = nullptr, *length = nullptr;
  int32_t *path_first = nullptr, *status = nullptr, *counts = nullptr;
  uint8_t *kind = nullptr;
};

namespace {

constexpr const char *kArenaWhat = "ccmp_path_resample: hipMalloc";

int resample_opts_ok(const ccmp_resample_opts &o)
{
  if (o.count == 1 || o.count < 0) return CCMP_EINVAL;
  if (o.count == 0 && !(o.spacing > 0.0)) return CCMP_EINVAL; // a NaN spacing fails the comparison
  if (o.max_rows < 2) return CCMP_EINVAL;
  return CCMP_OK;
}

// rows out of a path with T > 0, or -1: FULL
int64_t rows_out(double T, const ccmp_resample_opts &o)
{
  const int64_t n = ccmp::retime_count(T, o.count, o.spacing);
  return (n < 0 || n > (int64_t)o.max_rows) ? -1 : n;
}

int make_handle(ccmp_ctx *ctx, size_t F, size_t rows, ccmp_sampled_paths **out)
{
  ccmp_sampled_paths *h = new (std::nothrow) ccmp_sampled_paths();
  if (!h) return CCMP_ENOMEM;
  h->F = F;
  h->rows = rows;
  const size_t R = rows ? rows : 1, P = F + 1;
  ResultBlock b;
  const size_t o_rows = b.take(R * 14 * sizeof(double)), o_arc = b.take(R * sizeof(double)), o_len = b.take(P * sizeof(double)),
               o_pf = b.take(P * sizeof(int32_t)), o_st = b.take(P * sizeof(int32_t)), o_cnt = b.take(P * ccmp::kRetimeKinds * sizeof(int32_t)), o_kind = b.take(R);
  { const int rc = b.alloc(h, ctx, kArenaWhat); if (rc != CCMP_OK) { delete h; return rc; } }
  h->d_rows = b.at<double>(o_rows);
  h->arc = b.at<double>(o_arc);
  h->length = b.at<double>(o_len);
  h->path_first = b.at<int32_t>(o_pf);
  h->status = b.at<int32_t>(o_st);
  h->counts = b.at<int32_t>(o_cnt);
  h->kind = b.at<uint8_t>(o_kind);
  *out = h;
  return CCMP_OK;
}

// the body of ccmp_path_resample behind its checks.  On any failure *out stays NULL.
int resample(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_dense_paths *d, const ccmp_resample_opts &o, ccmp_sampled_paths **out, hipStream_t st)
{
  const size_t F = d->F, S = d->slots, W = F ? S / F : 0;
  std::vector<int32_t> path_first(F + 1, 0), seg_first(S ? S : 1), status(F ? F : 1), out_first(F + 1, 0);
  std::vector<uint8_t> seg_ok(S ? S : 1);
  std::vector<double> length(F ? F : 1);
  CallArena mem(ctx, kArenaWhat);
  if (F) {
    int32_t *d_status = mem.array<int32_t>(F);
    if (!mem.ok()) return CCMP_EHIP;
    hipError_t e = ccmp_launch::retime_status(d->d_rows, d->path_first, F, d->rows, d_status, nullptr, st);
    if (e == hipSuccess) e = hipMemcpyAsync(status.data(), d_status, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(path_first.data(), d->path_first, (F + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(length.data(), d->length, F * sizeof(double), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && S) e = hipMemcpyAsync(seg_first.data(), d->seg_first, S * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && S) e = hipMemcpyAsync(seg_ok.data(), d->seg_ok, S, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    HIP_TRY(e);
    HIP_TRY(es);
  }
  int64_t M = 0;
  for (size_t f = 0; f < F; f++) { // the statuses, in the rule's order
    out_first[f] = (int32_t)M;
    int64_t n = 0;
    bool broken = false;
    for (size_t i = 0; i < W; i++) broken = broken || (seg_first[f * W + i] >= 0 && seg_ok[f * W + i] == 0);
    if (status[f] == ccmp::kRetimeEmpty) n = 0;
    else if (broken) status[f] = ccmp::kRetimeBroken;
    else if (status[f] == ccmp::kRetimeNonFinite) n = 0;
    else if (!(length[f] > 0.0)) { status[f] = ccmp::kRetimePoint; n = 1; }
    else if ((n = rows_out(length[f], o)) < 0) { status[f] = ccmp::kRetimeFull; n = 0; }
    M += n;
    if ((uint64_t)M > kMaxRows) return CCMP_EOVERFLOW;
  }
  out_first[F] = (int32_t)M;

  ccmp_sampled_paths *h = nullptr;
  { const int rc = make_handle(ctx, F, (size_t)M, &h); if (rc != CCMP_OK) return rc; }
  int rc = CCMP_OK;
  hipError_t e = hipMemcpyAsync(h->path_first, out_first.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && F) e = hipMemcpyAsync(h->status, status.data(), F * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && F) e = hipMemsetAsync(h->counts, 0, F * ccmp::kRetimeKinds * sizeof(int32_t), st);
  if (e == hipSuccess && M) {
    const size_t m = (size_t)M;
    double *x = mem.array<double>(m * 14), *y = mem.array<double>(m * 14);
    int32_t *choice = mem.array<int32_t>(m);
    uint8_t *kind0 = mem.array<uint8_t>(m), *ok = mem.array<uint8_t>(m);
    if (!mem.ok()) rc = CCMP_EHIP;
    if (rc == CCMP_OK) e = hipMemsetAsync(choice, 0xff, m * sizeof(int32_t), st); // a row the bracket refuses to trust is left alone by the pick too
    if (rc == CCMP_OK && e == hipSuccess) e = hipMemsetAsync(x, 0, m * 14 * sizeof(double), st);
    if (rc == CCMP_OK && e == hipSuccess)
      e = ccmp_launch::resample_bracket(d->d_rows, d->arc, d->path_first, h->status, h->path_first, F, m, d->rows, x, choice, kind0, st);
    if (rc == CCMP_OK && e == hipSuccess) rc = ccmp_project_batch(ctx, p, x, y, ok, nullptr, m, st); // ONE call for all paths
    if (rc == CCMP_OK && e == hipSuccess)
      e = ccmp_launch::resample_pick(d->d_rows, h->path_first, F, m, d->rows, choice, kind0, y, ok, h->d_rows, h->kind, h->counts, st);
  }
  if (rc == CCMP_OK && e == hipSuccess && F) e = ccmp_launch::dense_arc(h->d_rows, h->path_first, F, h->arc, h->length, st);
  const hipError_t es = hipStreamSynchronize(st); // the call is synchronous: the host arrays above and the arena go when it returns
  if (rc == CCMP_OK && e != hipSuccess) rc = hip_fail(e, "ccmp_path_resample");
  if (rc == CCMP_OK && es != hipSuccess) rc = hip_fail(es, "ccmp_path_resample: hipStreamSynchronize");
  if (rc != CCMP_OK) { ccmp_sampled_paths_destroy(h); return rc; }
  *out = h;
  return CCMP_OK;
}

int sampled_copy(ccmp_sampled_paths *h, double *rows_out, int32_t *path_first, double *arc, double *length, uint8_t *kind, int32_t *status, int32_t *counts,
                 hipMemcpyKind how, hipStream_t st)
{
  const size_t R = h->rows, F = h->F;
  if (rows_out && R) HIP_TRY(hipMemcpyAsync(rows_out, h->d_rows, R * 14 * sizeof(double), how, st));
  if (path_first) HIP_TRY(hipMemcpyAsync(path_first, h->path_first, (F + 1) * sizeof(int32_t), how, st));
  if (arc && R) HIP_TRY(hipMemcpyAsync(arc, h->arc, R * sizeof(double), how, st));
  if (length && F) HIP_TRY(hipMemcpyAsync(length, h->length, F * sizeof(double), how, st));
  if (kind && R) HIP_TRY(hipMemcpyAsync(kind, h->kind, R, how, st));
  if (status && F) HIP_TRY(hipMemcpyAsync(status, h->status, F * sizeof(int32_t), how, st));
  if (counts && F) HIP_TRY(hipMemcpyAsync(counts, h->counts, F * ccmp::kRetimeKinds * sizeof(int32_t), how, st));
  return CCMP_OK;
}

// what every time-stamp form checks of its arguments (the host form checks path_first too)
int stamps_checks(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax, const double *amax, double beta,
                  const double *time, const double *duration, const int32_t *status, retime_limits *lim)
{
  if (!(beta > 0.0 && beta < 1.0)) return CCMP_EINVAL;
  { const int rc = limits_ok(vmax, amax, lim->vmax, lim->amax); if (rc != CCMP_OK) return rc; }
  lim->beta = beta;
  if (total_rows > kMaxRows || F > kMaxRows) return CCMP_EINVAL;
  if (F == 0) return CCMP_OK;
  if (!path_first || !duration || !status || (total_rows && (!rows || !time))) return CCMP_EINVAL;
  return CCMP_OK;
}

// the launches of a checked call; a_bits [F], ceiling and envelope [total_rows] on the device
int stamps_launches(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const retime_limits &lim, unsigned long long *a_bits,
                    double *time, double *duration, double *ceiling, double *envelope, int32_t *status, hipStream_t st)
{
  HIP_TRY(ccmp_launch::retime_status(rows, path_first, F, total_rows, status, a_bits, st));
  if (total_rows) {
    HIP_TRY(ccmp_launch::retime_ceiling(rows, path_first, F, total_rows, status, lim, ceiling, a_bits, st));
    HIP_TRY(ccmp_launch::retime_envelope(ceiling, path_first, F, total_rows, status, a_bits, envelope, st));
  }
  HIP_TRY(ccmp_launch::retime_stamp(rows, envelope, path_first, status, a_bits, lim, F, time, duration, st));
  return CCMP_OK;
}

}  // namespace

extern "C" {

void ccmp_resample_opts_default(const ccmp_problem *p, ccmp_resample_opts *opts)
{
  if (!opts) return;
  opts->count = 0;
  opts->spacing = p ? p->delta : 0.0;
  opts->max_rows = 65536;
}

int ccmp_path_resample(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_dense_paths *dense, const ccmp_resample_opts *opts, ccmp_sampled_paths **out,
                       void *hip_stream)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out || !dense) return CCMP_EINVAL;
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  ccmp_resample_opts o;
  ccmp_resample_opts_default(p, &o);
  if (opts) o = *opts;
  { const int rc = resample_opts_ok(o); if (rc != CCMP_OK) return rc; }
  if (dense->device != ctx->device) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  return resample(ctx, p, dense, o, out, (hipStream_t)hip_stream);
}

int ccmp_sampled_paths_info(const ccmp_sampled_paths *h, size_t *F, size_t *rows)
{
  if (!h) return CCMP_EINVAL;
  if (F) *F = h->F;
  if (rows) *rows = h->rows;
  return CCMP_OK;
}

int ccmp_sampled_paths_copy(ccmp_sampled_paths *h, double *rows_out, int32_t *path_first, double *arc, double *length, uint8_t *kind, int32_t *status,
                            int32_t *counts, void *hip_stream)
{
  if (!h) return no_handle();
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  return sampled_copy(h, rows_out, path_first, arc, length, kind, status, counts, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream);
}

int ccmp_sampled_paths_copy_host(ccmp_sampled_paths *h, double *rows_out, int32_t *path_first, double *arc, double *length, uint8_t *kind, int32_t *status,
                                 int32_t *counts)
{
  if (!h) return no_handle();
  if (!ccmp_host::context_alive(h->ctx)) return CCMP_EINVAL;
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(h->ctx, __func__); // nothing staged: the copies come straight from the result
  const int rc = sampled_copy(h, rows_out, path_first, arc, length, kind, status, counts, hipMemcpyDeviceToHost, h->ctx->stream);
  return sg.finish(rc);
}

void ccmp_sampled_paths_destroy(ccmp_sampled_paths *h) { result_destroy(h); }

int ccmp_path_timestamps(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax, const double *amax,
                         double beta, double *time, double *duration, double *ceiling, double *envelope, int32_t *status, void *hip_stream)
{
  if (!ctx) return no_handle();
  retime_limits lim;
  { const int rc = stamps_checks(rows, path_first, F, total_rows, vmax, amax, beta, time, duration, status, &lim); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  // the context's workspace: the bits of A [F], then a ceiling and an envelope array where the caller gave none (the first call at a size grows it)
  const size_t per = align256((total_rows ? total_rows : 1) * sizeof(double)), head = align256(F * sizeof(unsigned long long));
  const size_t bytes = head + (ceiling ? 0 : per) + (envelope ? 0 : per);
  { const int rc = grow_buffer(ctx, &ctx->retime_ws, &ctx->retime_ws_cap, bytes, bytes); if (rc != CCMP_OK) return rc; }
  char *ws = (char *)ctx->retime_ws;
  double *x = ceiling ? ceiling : (double *)(ws + head), *y = envelope ? envelope : (double *)(ws + head + (ceiling ? 0 : per));
  return stamps_launches(rows, path_first, F, total_rows, lim, (unsigned long long *)ws, time, duration, x, y, status, (hipStream_t)hip_stream);
}

int ccmp_path_timestamps_host(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax,
                              const double *amax, double beta, double *time, double *duration, double *ceiling, double *envelope, int32_t *status)
{
  if (!ctx) return no_handle();
  retime_limits lim;
  { const int rc = stamps_checks(rows, path_first, F, total_rows, vmax, amax, beta, time, duration, status, &lim); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t R = total_rows ? total_rows : 1;
  CallArena mem(ctx, "ccmp_path_timestamps_host: hipMalloc"); // the staging is memory of this call
  double *d_rows = mem.array<double>(R * 14), *d_time = mem.array<double>(R), *d_x = mem.array<double>(R), *d_y = mem.array<double>(R), *d_dur = mem.array<double>(F);
  int32_t *d_pf = mem.array<int32_t>(F + 1), *d_status = mem.array<int32_t>(F);
  unsigned long long *d_a = mem.array<unsigned long long>(F);
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  sg.up(d_rows, rows, total_rows * 14 * sizeof(double));
  sg.up(d_pf, path_first, (F + 1) * sizeof(int32_t));
  sg.up(d_time, time, total_rows * sizeof(double)); // the caller's values go up first: rows of a path that is not OK stay the caller's
  sg.up(d_x, ceiling, total_rows * sizeof(double));
  sg.up(d_y, envelope, total_rows * sizeof(double));
  { const int rc = sg.finish(CCMP_OK); if (rc != CCMP_OK) return rc; }
  { const int rc = stamps_launches(d_rows, d_pf, F, total_rows, lim, d_a, d_time, d_dur, d_x, d_y, d_status, ctx->stream); if (rc != CCMP_OK) return sg.finish(rc); }
  sg.down(time, d_time, total_rows * sizeof(double));
  sg.down(ceiling, d_x, total_rows * sizeof(double));
  sg.down(envelope, d_y, total_rows * sizeof(double));
  sg.down(duration, d_dur, F * sizeof(double));
  sg.down(status, d_status, F * sizeof(int32_t));
  return sg.finish(CCMP_OK);
}

int ccmp_path_timestamps_ref(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax, const double *amax, double beta,
                             double *time, double *duration, double *ceiling, double *envelope, int32_t *status)
{
  retime_limits lim;
  { const int rc = stamps_checks(rows, path_first, F, total_rows, vmax, amax, beta, time, duration, status, &lim); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  const double inf = __builtin_inf();
  std::vector<double> V, x, y;
  for (size_t f = 0; f < F; f++) {
    const size_t first = (size_t)path_first[f], R = (size_t)(path_first[f + 1] - path_first[f]);
    const double *q = rows + first * 14;
    if (R == 0) { status[f] = ccmp::kRetimeEmpty; duration[f] = 0.0; continue; }
    bool finite = true;
    for (size_t w = 0; w < R * 14; w++) finite = finite && ccmp::retime_finite(q[w]);
    if (!finite) { status[f] = ccmp::kRetimeNonFinite; duration[f] = __builtin_nan(""); continue; }
    status[f] = ccmp::kRetimeOk;
    V.assign(R, inf); x.assign(R, 0.0); y.assign(R, 0.0);
    double A = inf;
    for (size_t i = 0; i + 1 < R; i++)
      for (int c = 0; c < 14; c++) {
        const double d = q[(i + 1) * 14 + c] - q[i * 14 + c];
        V[i] = ccmp::retime_min(V[i], ccmp::retime_joint_v(lim.vmax[c], d));
        A = ccmp::retime_min(A, ccmp::retime_joint_acc(lim.beta, lim.amax[c], d));
      }
    for (size_t i = 1; i + 1 < R; i++) {
      double curv = inf;
      for (int c = 0; c < 14; c++) {
        const double d = q[(i + 1) * 14 + c] - q[i * 14 + c], dp = q[i * 14 + c] - q[(i - 1) * 14 + c];
        curv = ccmp::retime_min(curv, ccmp::retime_joint_curv(lim.beta, lim.amax[c], d, dp));
      }
      x[i] = ccmp::retime_ceiling(V[i - 1], V[i], curv);
    }
    const double g = 2.0 * A;
    for (size_t i = 0; i < R; i++) {
      double m = x[i];
      for (size_t k = 0; k < R; k++)
        if (k != i) m = ccmp::retime_min(m, ccmp::retime_env_term(x[k], g, (int64_t)(k > i ? k - i : i - k)));
      y[i] = m;
    }
    double t = 0.0;
    time[first] = t;
    if (R == 2) {
      t = t + ccmp::retime_dt_pair(V[0], g);
      time[first + 1] = t;
    } else {
      for (size_t i = 0; i + 1 < R; i++) {
        t = t + ccmp::retime_dt(y[i], y[i + 1]);
        time[first + i + 1] = t;
      }
    }
    duration[f] = t;
    if (ceiling) memcpy(ceiling + first, x.data(), R * sizeof(double));
    if (envelope) memcpy(envelope + first, y.data(), R * sizeof(double));
  }
  return CCMP_OK;
}

int ccmp_arc_bracket_ref(const double *arcs, int n, double h, int *k, double *t, int *lower)
{
  if (!arcs || n < 2 || !k || !t || !lower || !(h > 0.0) || !(h <= arcs[n - 1])) return CCMP_EINVAL;
  bool lo;
  ccmp::arc_bracket(arcs, n, h, k, t, &lo);
  *lower = lo ? 1 : 0;
  return CCMP_OK;
}

int ccmp_resample_targets_ref(double T, int count, double spacing, int max_rows, int *N, double *h_out)
{
  const ccmp_resample_opts o{count, spacing, max_rows};
  if (!N || resample_opts_ok(o) != CCMP_OK) return CCMP_EINVAL;
  if (!(T > 0.0)) { // POINT: one row, at arc +0.0
    *N = 1;
    if (h_out) h_out[0] = 0.0;
    return CCMP_OK;
  }
  const int64_t n = rows_out(T, o);
  *N = n < 0 ? 0 : (int)n; // FULL: no row
  if (n < 0 || !h_out) return CCMP_OK;
  h_out[0] = 0.0;
  for (int64_t j = 1; j + 1 < n; j++) h_out[j] = ccmp::retime_target(j, n, T);
  h_out[n - 1] = T;
  return CCMP_OK;
}

}  // extern "C"
