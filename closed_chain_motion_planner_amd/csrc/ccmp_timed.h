/* ccmp_timed.h — what the host code of the timed-path units shares (ccmp_setpoints.cpp, ccmp_fit.cpp, ccmp_jerk.cpp; the argument checks
 * also ccmp_retime.cpp): the checks of limits, path_first, problem and scene, the staging of a *_host call's path arrays, the checked
 * prefix sum of per-path counts, the delivery tail of the two units that hand out ticks, and the host loops of the _ref forms over the
 * rule text of ccmp_setpoints.h.  Host only, C++ linkage, hidden as the path units' share of ccmp_stage.h is: nothing here adds to the
 * library's dynamic symbols.  Every entry point keeps its own order of checks; this header only holds their texts. */
#ifndef CCMP_TIMED_H
#define CCMP_TIMED_H
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_scene.h"
#include "ccmp_setpoints.h"
#include "ccmp_stage.h"

namespace ccmp_host {

#pragma GCC visibility push(hidden)

inline bool finite_positive(double v) { return v > 0.0 && v - v == 0.0; }

/* path_first [F + 1] of a host or _ref form: starts at or above zero, never decreases, ends within the rows; F >= 1 */
inline int path_first_ok(const int32_t *path_first, size_t F, size_t total_rows)
{
  if (path_first[0] < 0) return CCMP_EINVAL;
  for (size_t f = 0; f < F; f++)
    if (path_first[f + 1] < path_first[f]) return CCMP_EINVAL;
  return (size_t)path_first[F] <= total_rows ? CCMP_OK : CCMP_EINVAL;
}

/* what a call that evaluates the constraint and, with a scene, the clearance checks of them */
inline int device_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin)
{
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
  return CCMP_OK;
}

/* the limits of a call, each of its 14 values finite and > 0, copied to v and a — and jmax to j where the unit has one (j != nullptr) */
inline int limits_ok(const double *vmax, const double *amax, double *v, double *a, const double *jmax = nullptr, double *j = nullptr)
{
  if (!vmax || !amax || (j && !jmax)) return CCMP_EINVAL;
  for (int c = 0; c < 14; c++) {
    if (!finite_positive(vmax[c]) || !finite_positive(amax[c]) || (j && !finite_positive(jmax[c]))) return CCMP_EINVAL;
    v[c] = vmax[c];
    a[c] = amax[c];
    if (j) j[c] = jmax[c];
  }
  return CCMP_OK;
}

/* rows [total_rows][14], time [total_rows] and path_first [F + 1] of a *_host call in memory of the call: taken from its arena (the caller
 * asks mem.ok() once, after all its arrays), then sent up on the staged call */
struct PathStage {
  double *rows, *time;
  int32_t *path_first;
  PathStage(CallArena &mem, size_t F, size_t total_rows)
      : rows(mem.array<double>((total_rows ? total_rows : 1) * 14)), time(mem.array<double>(total_rows ? total_rows : 1)), path_first(mem.array<int32_t>(F + 1)) {}
  void up(StagedCall &sg, const double *r, const double *t, const int32_t *pf, size_t F, size_t total_rows) const
  {
    sg.up(rows, r, total_rows * 14 * sizeof(double));
    sg.up(time, t, total_rows * sizeof(double));
    if (F) sg.up(path_first, pf, (F + 1) * sizeof(int32_t));
  }
};

/* The checked prefix sum of per-path counts into first [F + 1]: path f adds ticks(f) less `less`, and nothing where that is negative.  A
 * count outside 0 .. max_ticks is CCMP_EHIP (never: the kernels' counts obey the rule), a total beyond kMaxRows CCMP_EOVERFLOW. */
template <class Ticks> int tick_ranges(size_t F, int max_ticks, int less, Ticks ticks, std::vector<int32_t> *first, int64_t *total)
{
  int64_t M = 0;
  for (size_t f = 0; f < F; f++) {
    (*first)[f] = (int32_t)M;
    const int64_t n = ticks(f);
    if (n < 0 || n > max_ticks) return CCMP_EHIP;
    if (n > less) M += n - less;
    if ((uint64_t)M > kMaxRows) return CCMP_EOVERFLOW;
  }
  (*first)[F] = (int32_t)M;
  *total = M;
  return CCMP_OK;
}

/* The delivery tail of ccmp_path_setpoints and ccmp_path_jerk_setpoints on the fresh handle h (fields F, ticks, q, qd, tau, f, satisfied,
 * clearance, tick_first, status): the tick ranges and the statuses into h, the ticks cleared, the unit's sample step — its launches up to
 * and with the one that writes q, qd, tau and the clearance's NaN —, the function, is-satisfied and, with a scene, clearance entry points
 * ONCE each over all ticks of all paths, the unit's finish step — what is left up to and with its peak launch —, then the wait and the
 * errors under the entry point's name.  sample runs when there is a tick, finish when there is a path.  On any failure h is destroyed
 * and *out stays as it is. */
template <class H, class Sample, class Finish>
int deliver(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, H *h, const std::vector<int32_t> &tick_first, const int32_t *d_status,
            const char *what, hipStream_t st, Sample sample, Finish finish, H **out)
{
  const size_t F = h->F, m = h->ticks;
  int rc = CCMP_OK;
  hipError_t e = hipMemcpyAsync(h->tick_first, tick_first.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && F) e = hipMemcpyAsync(h->status, d_status, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && m) {
    e = hipMemsetAsync(h->q, 0, m * 14 * sizeof(double), st); // a tick the sample kernel refuses to trust stays zero
    if (e == hipSuccess) e = hipMemsetAsync(h->qd, 0, m * 14 * sizeof(double), st);
    if (e == hipSuccess) e = hipMemsetAsync(h->tau, 0, m * sizeof(double), st);
    if (e == hipSuccess) e = sample();
    if (e == hipSuccess) rc = ccmp_function_batch(ctx, p, h->q, h->f, m, st); // ONE call each for all ticks of all paths
    if (rc == CCMP_OK && e == hipSuccess) rc = ccmp_is_satisfied_batch(ctx, p, h->q, h->satisfied, m, st);
    if (rc == CCMP_OK && e == hipSuccess && scene) rc = ccmp_clearance_batch(ctx, p, scene, h->q, nullptr, m, margin, h->clearance, nullptr, nullptr, st);
  }
  if (rc == CCMP_OK && e == hipSuccess && F) e = finish();
  const hipError_t es = hipStreamSynchronize(st); // the call is synchronous: the caller's host arrays and its arena go when it returns
  if (rc == CCMP_OK && e != hipSuccess) rc = hip_fail(e, what);
  if (rc == CCMP_OK && es != hipSuccess) rc = hip_fail(es, (std::string(what) + ": hipStreamSynchronize").c_str());
  if (rc != CCMP_OK) { result_destroy(h); return rc; }
  *out = h;
  return CCMP_OK;
}

/* The _ref forms' tick j >= 1 of N of one OK path (rows r, tangents w, stamps t [R], D = t[R-1]): *tau, q and qd [14] on its bracket;
 * the bracket's k, 0 where the rule's precondition fails (never on an OK path) and q, qd stay as they are */
inline int ref_tick(const double *r, const double *w, const double *t, size_t R, int64_t j, int64_t N, double period, double D, double *tau, double *q, double *qd)
{
  int k;
  double u;
  if (!ccmp::setpoint_bracket(t, (int)R, j, N, period, D, tau, &k, &u)) return 0;
  for (int c = 0; c < 14 && k > 0; c++) ccmp::setpoint_joint(r + c, w + c, t, k, u, q + c, qd + c);
  return k;
}

/* one tick's speed and acceleration figures over the joints, from qd_a [14] at the tick and qd_b [14] at the next (read when width > 0):
 * the maxima of the shares, and whether a share was a NaN — such a figure never contributes */
struct TickFigures {
  double speed = 0.0, acc = 0.0;
  bool speed_nan = false, acc_nan = false;
};
inline TickFigures tick_figures(const double *qd_a, const double *qd_b, double width, const double *vmax, const double *amax)
{
  TickFigures g;
  for (int c = 0; c < 14; c++) {
    const double s = ccmp::setpoint_speed(qd_a[c], vmax[c]);
    g.speed_nan = g.speed_nan || s != s;
    if (s > g.speed) g.speed = s;
    if (width > 0.0) {
      const double a = ccmp::setpoint_acc(qd_a[c], qd_b[c], width, amax[c]);
      g.acc_nan = g.acc_nan || a != a;
      if (a > g.acc) g.acc = a;
    }
  }
  return g;
}

/* the speed and acceleration peaks pv, pj [2] of a qd sequence [N][14], width(j) = tau_{j+1} - tau_j: ticks in order, so the first tick of a
 * tie stays; the caller hands in "no contributor" (+0.0 at tick -1) */
template <class Width> void speed_acc_peaks(const double *qd, int64_t N, Width width, const double *vmax, const double *amax, double *pv, int32_t *pj)
{
  for (int64_t j = 0; j < N; j++) {
    const double wd = j + 1 < N ? width(j) : 0.0;
    const TickFigures g = tick_figures(qd + (size_t)j * 14, qd + (size_t)(j + 1) * 14, wd, vmax, amax);
    if (!g.speed_nan && ccmp::setpoint_higher(g.speed, (int32_t)j, pv[0], pj[0])) { pv[0] = g.speed; pj[0] = (int32_t)j; }
    if (wd > 0.0 && !g.acc_nan && ccmp::setpoint_higher(g.acc, (int32_t)j, pv[1], pj[1])) { pv[1] = g.acc; pj[1] = (int32_t)j; }
  }
}

#pragma GCC visibility pop

}  // namespace ccmp_host

#endif /* CCMP_TIMED_H */
