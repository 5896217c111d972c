// ccmp_jerk.cpp — jerk-bounded setpoints of the C ABI (include/ccmp.h: ccmp_path_jerk_setpoints*, ccmp_jerk_setpoints_*, ccmp_jerk_opts_default,
// ccmp_jerk_next_window_ref).
// The rule is csrc/ccmp_jerk.h.  A call is the setpoints unit's status and tangent launches, one decide launch that opens the paths, then per
// pass of the window search: ONE read of F words (they size the measure launch and tell when no path is open), one measure launch over the
// open paths' tiles and one decide launch; then the sample launch, the function, is-satisfied and — with a scene — clearance entry points
// ONCE each over all ticks of all paths, and the peak launch.  No allocation inside the search is sized by the ticks.  The _ref form runs
// the same rule text in plain loops, path by path.  The argument checks, the staging of the _host form, the tick ranges, the delivery tail
// (deliver: this unit hands it its sample launch and, with the window and passes copies, its peak launch) and the _ref form's tick and
// speed and acceleration peaks are csrc/ccmp_timed.h's, shared with the setpoints and fit units; the window search is this unit's own.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_jerk.h"
#include "ccmp_launch.h"
#include "ccmp_resident.h"
#include "ccmp_stage.h"
#include "ccmp_timed.h"

using namespace ccmp_host;
using ccmp::jerk_limits;

/* the result of ccmp_path_jerk_setpoints: one allocation, the arrays point into it */
struct ccmp_jerk_setpoints {
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  size_t F = 0, ticks = 0;
  void *block = nullptr;
  double *q = nullptr, *qd = nullptr, *tau = nullptr, *f = nullptr, *clearance = nullptr, *peak = nullptr;
  int32_t *tick_first = nullptr, *status = nullptr, *window = nullptr, *passes = nullptr, *peak_tick = nullptr, *counts = nullptr;
  uint8_t *satisfied = nullptr;
};

namespace {

constexpr const char *kArenaWhat = "ccmp_path_jerk_setpoints: hipMalloc";

int opts_ok(const ccmp_jerk_opts &o)
{
  return finite_positive(o.period) && o.max_ticks >= 2 && o.max_window >= 1 && o.max_window <= ccmp::kJerkMaxWindow && o.window >= 0 && o.window <= o.max_window &&
                 o.aim > 0.0 && o.aim <= 1.0 && o.tile_ticks >= 0
             ? CCMP_OK
             : CCMP_EINVAL;
}

// what every form checks of its arguments (the host and _ref forms check path_first too)
int input_checks(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                 const double *jmax, const ccmp_jerk_opts &o, jerk_limits *lim)
{
  { const int rc = opts_ok(o); if (rc != CCMP_OK) return rc; }
  { const int rc = limits_ok(vmax, amax, lim->vmax, lim->amax, jmax, lim->jmax); if (rc != CCMP_OK) return rc; }
  if (total_rows > kMaxRows || F > kMaxRows) return CCMP_EINVAL;
  if (F && (!path_first || (total_rows && (!rows || !time)))) return CCMP_EINVAL;
  return CCMP_OK;
}

int make_handle(ccmp_ctx *ctx, size_t F, size_t ticks, ccmp_jerk_setpoints **out)
{
  ccmp_jerk_setpoints *h = new (std::nothrow) ccmp_jerk_setpoints();
  if (!h) return CCMP_ENOMEM;
  h->F = F;
  h->ticks = ticks;
  const size_t M = ticks ? ticks : 1, P = F + 1;
  ResultBlock b;
  const size_t o_q = b.take(M * 14 * sizeof(double)), o_qd = b.take(M * 14 * sizeof(double)), o_tau = b.take(M * sizeof(double)),
               o_f = b.take(M * 2 * sizeof(double)), o_cl = b.take(M * sizeof(double)), o_peak = b.take(P * ccmp::kJerkPeaks * sizeof(double)),
               o_tf = b.take(P * sizeof(int32_t)), o_st = b.take(P * sizeof(int32_t)), o_w = b.take(P * sizeof(int32_t)), o_ps = b.take(P * sizeof(int32_t)),
               o_pt = b.take(P * ccmp::kJerkPeaks * sizeof(int32_t)), o_cnt = b.take(P * 2 * sizeof(int32_t)), o_sat = b.take(M);
  { const int rc = b.alloc(h, ctx, kArenaWhat); if (rc != CCMP_OK) { delete h; return rc; } }
  h->q = b.at<double>(o_q);
  h->qd = b.at<double>(o_qd);
  h->tau = b.at<double>(o_tau);
  h->f = b.at<double>(o_f);
  h->clearance = b.at<double>(o_cl);
  h->peak = b.at<double>(o_peak);
  h->tick_first = b.at<int32_t>(o_tf);
  h->status = b.at<int32_t>(o_st);
  h->window = b.at<int32_t>(o_w);
  h->passes = b.at<int32_t>(o_ps);
  h->peak_tick = b.at<int32_t>(o_pt);
  h->counts = b.at<int32_t>(o_cnt);
  h->satisfied = b.at<uint8_t>(o_sat);
  *out = h;
  return CCMP_OK;
}

int tile_of(const ccmp_jerk_opts &o) { return o.tile_ticks >= 1 && o.tile_ticks <= ccmp_launch::kJerkTile ? o.tile_ticks : ccmp_launch::kJerkTile; }

// the body of ccmp_path_jerk_setpoints behind its checks, on device pointers.  On any failure *out stays NULL.
int jerk(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first, const double *time,
         size_t F, size_t total_rows, const jerk_limits &lim, const ccmp_jerk_opts &o, ccmp_jerk_setpoints **out, hipStream_t st)
{
  const size_t Fn = F ? F : 1;
  const int T = tile_of(o), Ts = T < ccmp_launch::kJerkSampleTile ? T : ccmp_launch::kJerkSampleTile;
  std::vector<int32_t> word(Fn, -1), tile_first(F + 1, 0), tick_first(F + 1, 0);
  CallArena mem(ctx, kArenaWhat);
  int32_t *d_sp = mem.array<int32_t>(Fn), *d_ticks = mem.array<int32_t>(Fn), *d_word = mem.array<int32_t>(Fn), *d_tiles = mem.array<int32_t>(F + 1),
          *d_status = mem.array<int32_t>(Fn), *d_window = mem.array<int32_t>(Fn), *d_passes = mem.array<int32_t>(Fn);
  unsigned long long *P = mem.array<unsigned long long>(Fn);
  double *tangent = mem.array<double>((total_rows ? total_rows : 1) * 14);
  if (!mem.ok()) return CCMP_EHIP;
  int rc = CCMP_OK;
  hipError_t e = hipSuccess;
  if (F) {
    e = ccmp_launch::setpoints_status(rows, path_first, time, F, total_rows, o.period, o.max_ticks, d_sp, d_ticks, st);
    if (e == hipSuccess && total_rows) e = ccmp_launch::setpoints_tangent(rows, path_first, time, F, total_rows, d_sp, tangent, st);
    if (e == hipSuccess) e = ccmp_launch::jerk_decide(d_sp, d_ticks, F, true, o.window, o.max_window, o.aim, o.max_ticks, P, d_status, d_window, d_passes, d_word, st);
    // pass k measures the paths that k growths of the window have left open; W strictly increases, so max_window passes close them all
    for (int pass = 0; e == hipSuccess && pass <= o.max_window + 1; pass++) {
      e = hipMemcpyAsync(word.data(), d_word, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
      const hipError_t es = hipStreamSynchronize(st);
      if (e == hipSuccess) e = es;
      if (e != hipSuccess) break;
      bool open = false;
      int64_t tiles = 0;
      for (size_t f = 0; f < F; f++) {
        tile_first[f] = (int32_t)tiles;
        const int32_t M = word[f];
        if (M < 0) continue;
        open = true;
        if (M > o.max_ticks) { rc = CCMP_EHIP; break; } // (never: the kernel's count obeys the rule)
        if (M >= 3) tiles += (M - 2 + T - 1) / T;       // the tiles that hold a left tick j <= M - 3
        if ((uint64_t)tiles > kMaxRows) { rc = CCMP_EOVERFLOW; break; }
      }
      tile_first[F] = (int32_t)tiles;
      if (rc != CCMP_OK || !open) break;
      if (pass > o.max_window) { rc = CCMP_EHIP; break; } // (never: every decide launch closes a path or grows its window)
      if (tiles) {
        e = hipMemcpyAsync(d_tiles, tile_first.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
          e = ccmp_launch::jerk_measure(rows, path_first, time, tangent, d_tiles, (size_t)tiles, d_word, d_window, d_ticks, F, total_rows, o.period, T, lim, P, st);
      }
      if (e == hipSuccess) e = ccmp_launch::jerk_decide(d_sp, d_ticks, F, false, o.window, o.max_window, o.aim, o.max_ticks, P, d_status, d_window, d_passes, d_word, st);
    }
  }
  if (rc == CCMP_OK && e != hipSuccess) rc = hip_fail(e, "ccmp_path_jerk_setpoints");
  if (rc != CCMP_OK) { (void)hipStreamSynchronize(st); return rc; }

  int64_t M = 0, tiles = 0; // every path is closed: word [f] = -1 - its ticks
  { const int r = tick_ranges(F, o.max_ticks, 0, [&](size_t f) { return -1 - (int64_t)word[f]; }, &tick_first, &M); if (r != CCMP_OK) return r; }
  for (size_t f = 0; f < F; f++) {
    tile_first[f] = (int32_t)tiles;
    tiles += (tick_first[f + 1] - tick_first[f] + Ts - 1) / Ts;
  }
  tile_first[F] = (int32_t)tiles;

  ccmp_jerk_setpoints *h = nullptr;
  { const int r = make_handle(ctx, F, (size_t)M, &h); if (r != CCMP_OK) return r; }
  return deliver(
      ctx, p, scene, margin, h, tick_first, d_status, "ccmp_path_jerk_setpoints", st,
      [&] {
        const hipError_t eu = hipMemcpyAsync(d_tiles, tile_first.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
        return eu != hipSuccess ? eu
                                : ccmp_launch::jerk_sample(rows, path_first, time, tangent, d_tiles, (size_t)tiles, h->tick_first, d_status, d_window, d_ticks, F, h->ticks,
                                                           total_rows, o.period, Ts, h->q, h->qd, h->tau, h->clearance, st);
      },
      [&] { // the window and the passes of every path, then the audit
        hipError_t ef = hipMemcpyAsync(h->window, d_window, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        if (ef == hipSuccess) ef = hipMemcpyAsync(h->passes, d_passes, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
        return ef != hipSuccess ? ef
                                : ccmp_launch::jerk_peak(h->qd, h->f, h->satisfied, h->clearance, h->tick_first, F, h->ticks, o.period, lim, margin, h->peak, h->peak_tick,
                                                         h->counts, st);
      },
      out);
}

int result_copy(ccmp_jerk_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied, double *clearance, int32_t *status,
                int32_t *window, int32_t *passes, double *peak, int32_t *peak_tick, int32_t *counts, hipMemcpyKind how, hipStream_t st)
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
  if (window && F) HIP_TRY(hipMemcpyAsync(window, h->window, F * sizeof(int32_t), how, st));
  if (passes && F) HIP_TRY(hipMemcpyAsync(passes, h->passes, F * sizeof(int32_t), how, st));
  if (peak && F) HIP_TRY(hipMemcpyAsync(peak, h->peak, F * ccmp::kJerkPeaks * sizeof(double), how, st));
  if (peak_tick && F) HIP_TRY(hipMemcpyAsync(peak_tick, h->peak_tick, F * ccmp::kJerkPeaks * sizeof(int32_t), how, st));
  if (counts && F) HIP_TRY(hipMemcpyAsync(counts, h->counts, F * 2 * sizeof(int32_t), how, st));
  return CCMP_OK;
}

// The _ref form's view of one OK path: the inputs x_0 .. x_n (position and velocity parts), computed once
struct RefPath {
  std::vector<double> xq, xd; // [(n + 1)][14]
  int64_t n = 0;
  const double *input(const std::vector<double> &x, int64_t i) const { return x.data() + (size_t)(i <= 0 ? 0 : i >= n ? n : i) * 14; }
};

// the filtered velocity of tick j of M = n + W ticks, joint c
double filtered(const RefPath &p, const std::vector<double> &x, int64_t j, int W, int c)
{
  double sum = p.input(x, j - W + 1)[c];
  for (int k = 1; k < W; k++) sum = sum + p.input(x, j - W + 1 + k)[c];
  return ccmp::jerk_mean(sum, W);
}

// qd [M][14] of the window W: the copies at both ends are +0.0 (as every term of their windows is)
void filtered_qd(const RefPath &p, int W, int64_t M, std::vector<double> *v)
{
  v->assign((size_t)M * 14, 0.0);
  for (int64_t j = 1; j + 1 < M; j++)
    for (int c = 0; c < 14; c++) (*v)[(size_t)j * 14 + c] = filtered(p, p.xd, j, W, c);
}

// the jerk peak of qd [M][14]: ticks in order, so the first tick of a tie stays
void jerk_peak_ref(const std::vector<double> &v, int64_t M, double period, const jerk_limits &lim, double *pv, int32_t *pj)
{
  *pv = 0.0;
  *pj = -1;
  for (int64_t j = 0; j + 2 < M; j++) {
    double jerk = 0.0;
    bool nan = false;
    for (int c = 0; c < 14; c++) {
      const double s = ccmp::jerk_share(v[(size_t)j * 14 + c], v[(size_t)(j + 1) * 14 + c], v[(size_t)(j + 2) * 14 + c], j, period, lim.jmax[c]);
      nan = nan || s != s;
      if (s > jerk) jerk = s;
    }
    if (!nan && ccmp::setpoint_higher(jerk, (int32_t)(j + 1), *pv, *pj)) { *pv = jerk; *pj = (int32_t)(j + 1); }
  }
}

}  // namespace

extern "C" {

void ccmp_jerk_opts_default(ccmp_jerk_opts *opts)
{
  if (!opts) return;
  opts->period = 0.001;
  opts->max_ticks = 65536;
  opts->window = 0;
  opts->max_window = 64;
  opts->aim = 0.95;
  opts->tile_ticks = 0;
}

int ccmp_path_jerk_setpoints(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first,
                             const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax, const double *jmax,
                             const ccmp_jerk_opts *opts, ccmp_jerk_setpoints **out, void *hip_stream)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out) return CCMP_EINVAL;
  { const int rc = device_checks(ctx, p, scene, margin); if (rc != CCMP_OK) return rc; }
  const ccmp_jerk_opts o = opts_or(opts, ccmp_jerk_opts_default);
  jerk_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, jmax, o, &lim); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  return jerk(ctx, p, scene, margin, rows, path_first, time, F, total_rows, lim, o, out, (hipStream_t)hip_stream);
}

int ccmp_path_jerk_setpoints_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows,
                                  const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                                  const double *jmax, const ccmp_jerk_opts *opts, ccmp_jerk_setpoints **out)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out) return CCMP_EINVAL;
  { const int rc = device_checks(ctx, p, scene, margin); if (rc != CCMP_OK) return rc; }
  const ccmp_jerk_opts o = opts_or(opts, ccmp_jerk_opts_default);
  jerk_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, jmax, o, &lim); if (rc != CCMP_OK) return rc; }
  if (F) { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  CallArena mem(ctx, "ccmp_path_jerk_setpoints_host: hipMalloc"); // the staging is memory of this call
  const PathStage d(mem, F, total_rows);
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  d.up(sg, rows, time, path_first, F, total_rows);
  { const int rc = sg.finish(CCMP_OK); if (rc != CCMP_OK) return rc; }
  return jerk(ctx, p, scene, margin, d.rows, d.path_first, d.time, F, total_rows, lim, o, out, ctx->stream);
}

int ccmp_jerk_setpoints_info(const ccmp_jerk_setpoints *h, size_t *F, size_t *ticks)
{
  if (!h) return CCMP_EINVAL;
  if (F) *F = h->F;
  if (ticks) *ticks = h->ticks;
  return CCMP_OK;
}

int ccmp_jerk_setpoints_copy(ccmp_jerk_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied,
                             double *clearance, int32_t *status, int32_t *window, int32_t *passes, double *peak, int32_t *peak_tick, int32_t *counts,
                             void *hip_stream)
{
  if (!h) return no_handle();
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  return result_copy(h, q, qd, tau, tick_first, f, satisfied, clearance, status, window, passes, peak, peak_tick, counts, hipMemcpyDeviceToDevice,
                     (hipStream_t)hip_stream);
}

int ccmp_jerk_setpoints_copy_host(ccmp_jerk_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied,
                                  double *clearance, int32_t *status, int32_t *window, int32_t *passes, double *peak, int32_t *peak_tick,
                                  int32_t *counts)
{
  if (!h) return no_handle();
  if (!ccmp_host::context_alive(h->ctx)) return CCMP_EINVAL;
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(h->ctx, __func__); // nothing staged: the copies come straight from the result
  const int rc = result_copy(h, q, qd, tau, tick_first, f, satisfied, clearance, status, window, passes, peak, peak_tick, counts, hipMemcpyDeviceToHost, h->ctx->stream);
  return sg.finish(rc);
}

void ccmp_jerk_setpoints_destroy(ccmp_jerk_setpoints *h) { result_destroy(h); }

int ccmp_jerk_setpoints_ref(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax,
                            const double *amax, const double *jmax, const ccmp_jerk_opts *opts, int32_t *tick_first, int32_t *status, int32_t *window,
                            int32_t *passes, double *q, double *qd, double *tau, double *peak, int32_t *peak_tick)
{
  const ccmp_jerk_opts o = opts_or(opts, ccmp_jerk_opts_default);
  jerk_limits lim;
  { const int rc = input_checks(rows, path_first, time, F, total_rows, vmax, amax, jmax, o, &lim); if (rc != CCMP_OK) return rc; }
  if (!tick_first || (F && (!status || !window || !passes))) return CCMP_EINVAL;
  if (F) { const int rc = path_first_ok(path_first, F, total_rows); if (rc != CCMP_OK) return rc; }
  // first pass: status, window, passes and the tick counts (all a sizing call asks for); nothing is written before the total is known to fit
  std::vector<int32_t> st(F ? F : 1), win(F ? F : 1, 0), pas(F ? F : 1, 0), first(F + 1, 0);
  std::vector<RefPath> paths(F);
  std::vector<double> w, v;
  int64_t total = 0;
  for (size_t f = 0; f < F; f++) {
    const size_t a = (size_t)path_first[f], R = (size_t)(path_first[f + 1] - path_first[f]);
    const double *r = rows + a * 14, *t = time + a;
    first[f] = (int32_t)total;
    // status and N of (rows, stamps): the setpoints rule's own host form, as a sizing call
    const int32_t pf[2] = {0, (int32_t)R};
    const ccmp_setpoint_opts so = {o.period, o.max_ticks};
    int32_t tf[2] = {0, 0}, sp = ccmp::kSetpointsEmpty;
    { const int rc = ccmp_setpoints_ref(r, pf, t, 1, R, lim.vmax, lim.amax, &so, tf, &sp, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); if (rc != CCMP_OK) return rc; }
    int32_t M = 0;
    if (sp != ccmp::kSetpointsOk) {
      st[f] = sp;
      M = sp == ccmp::kSetpointsPoint ? 1 : 0;
      if (sp == ccmp::kSetpointsFull) win[f] = o.window ? o.window : 1; // FULL names the window that did not fit
    } else {
      RefPath &p = paths[f];
      const int64_t n = p.n = (int64_t)tf[1] - 1;
      const double D = t[R - 1];
      int W = o.window ? o.window : 1;
      M = ccmp::jerk_ticks(n, W, o.max_ticks);
      st[f] = M ? ccmp::kJerkOpen : ccmp::kJerkFull;
      if (M) { // the inputs x_0 .. x_n, once
        w.resize(R * 14);
        (void)ccmp_setpoint_tangents_ref(r, t, R, w.data());
        p.xq.assign((size_t)(n + 1) * 14, 0.0);
        p.xd.assign((size_t)(n + 1) * 14, 0.0);
        memcpy(p.xq.data(), r, 14 * sizeof(double));
        memcpy(p.xq.data() + (size_t)n * 14, r + (R - 1) * 14, 14 * sizeof(double));
        double at; // (the input's own tau: the output's grid is jerk_tau)
        for (int64_t i = 1; i < n; i++) (void)ref_tick(r, w.data(), t, R, i, n + 1, o.period, D, &at, &p.xq[(size_t)i * 14], &p.xd[(size_t)i * 14]);
      }
      while (st[f] == ccmp::kJerkOpen) {
        double pv;
        int32_t pj;
        filtered_qd(p, W, M, &v);
        jerk_peak_ref(v, M, o.period, lim, &pv, &pj);
        if (pv <= 1.0 || o.window || W >= o.max_window) {
          st[f] = pv <= 1.0 ? ccmp::kJerkOk : ccmp::kJerkWindow;
        } else {
          W = ccmp::jerk_next_window(W, pv, o.aim, o.max_window);
          pas[f] += 1;
          M = ccmp::jerk_ticks(n, W, o.max_ticks);
          if (!M) st[f] = ccmp::kJerkFull;
        }
      }
      win[f] = W;
    }
    total += M;
    if ((uint64_t)total > kMaxRows) return CCMP_EOVERFLOW;
  }
  first[F] = (int32_t)total;
  memcpy(tick_first, first.data(), (F + 1) * sizeof(int32_t));
  if (F) {
    memcpy(status, st.data(), F * sizeof(int32_t));
    memcpy(window, win.data(), F * sizeof(int32_t));
    memcpy(passes, pas.data(), F * sizeof(int32_t));
  }
  if (!q && !qd && !tau && !peak && !peak_tick) return CCMP_OK;

  for (size_t f = 0; f < F; f++) {
    const size_t a = (size_t)path_first[f], g0 = (size_t)first[f];
    const int64_t M = first[f + 1] - first[f];
    const RefPath &p = paths[f];
    const int W = win[f];
    double pv[3] = {0.0, 0.0, 0.0};
    int32_t pj[3] = {-1, -1, -1};
    if (st[f] == ccmp::kSetpointsPoint) {
      if (q) memcpy(q + g0 * 14, rows + a * 14, 14 * sizeof(double));
      if (qd) for (int c = 0; c < 14; c++) qd[g0 * 14 + c] = 0.0;
      if (tau) tau[g0] = 0.0;
      pj[0] = 0; // one tick at rest: the speed ratio +0.0 at tick 0
    } else if (M) {
      filtered_qd(p, W, M, &v);
      for (int64_t j = 0; j < M; j++) {
        if (q)
          for (int c = 0; c < 14; c++)
            q[(g0 + (size_t)j) * 14 + c] = j == 0 ? p.xq[c] : j == M - 1 ? p.xq[(size_t)p.n * 14 + c] : filtered(p, p.xq, j, W, c);
        if (tau) tau[g0 + (size_t)j] = ccmp::jerk_tau(j, o.period);
      }
      if (qd) memcpy(qd + g0 * 14, v.data(), (size_t)M * 14 * sizeof(double));
      speed_acc_peaks(v.data(), M, [&](int64_t j) { return ccmp::jerk_tau(j + 1, o.period) - ccmp::jerk_tau(j, o.period); }, lim.vmax, lim.amax, pv, pj);
      jerk_peak_ref(v, M, o.period, lim, &pv[2], &pj[2]);
    }
    if (peak) for (int k = 0; k < 3; k++) peak[f * 3 + k] = pv[k];
    if (peak_tick) for (int k = 0; k < 3; k++) peak_tick[f * 3 + k] = pj[k];
  }
  return CCMP_OK;
}

int ccmp_jerk_next_window_ref(int W, double P, double aim, int max_window, int *next)
{
  if (!next || max_window < 1 || max_window > ccmp::kJerkMaxWindow || W < 1 || W >= max_window || P != P || !(aim > 0.0 && aim <= 1.0)) return CCMP_EINVAL;
  *next = ccmp::jerk_next_window(W, P, aim, max_window);
  return CCMP_OK;
}

}  // extern "C"
