// ccmp_smooth.cpp — smooth solution paths of the C ABI (include/ccmp.h: ccmp_path_smooth, ccmp_smooth_*): B-spline passes on the
// manifold.  The rule is csrc/ccmp_smooth.h.  This unit owns the pass loop.  A pass is three midpoint steps and one test step over the
// paths that are still active: a midpoint step is the dense unit's densify on E two-waypoint paths in the distinct layout (it continues
// open segments, keeps the lists on the device and writes the arcs), a bracket launch, the projector's batch entry on the E blends and a
// pick launch; the test step is the shortcut unit's tile and continuation loop over explicit (from, to) rows (ccmp_pair_tests.h).  The
// host reads what those loops read, the F finiteness flags once and the F counts of accepted vertices per pass.  The paths alternate
// between two buffers of the call; only when every path has stopped does anything reach the caller's outputs, so a call that spends
// max_calls leaves them untouched.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_launch.h"
#include "ccmp_pair_tests.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"
#include "ccmp_smooth.h"
#include "ccmp_stage.h"

using namespace ccmp_host;
using ccmp::smooth_path;

namespace {

constexpr const char *kArenaWhat = "ccmp_path_smooth: hipMalloc";

int opts_ok(const ccmp_smooth_opts &o)
{
  if (o.max_steps < 0 || !(o.min_change >= 0.0)) return CCMP_EINVAL; // a NaN min_change fails the comparison; +inf passes
  if (o.chunk_states < 2 || o.round_budget < 0 || o.max_calls < 1 || o.tile_edges < 1) return CCMP_EINVAL;
  return CCMP_OK;
}

// what the calling thread's last ccmp_path_smooth / _host did (ccmp_smooth_last_counts): extend calls, projector calls, bytes read on the host
thread_local PairLoopCounts t_counts;
thread_local long long t_projects = 0;

struct Outputs {
  double *joints;
  int32_t *len, *passes, *moved, *stop;
  double *length_in, *length_out;
  int32_t *stats;
};

// everything both forms check before anything touches the device
int smooth_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                  size_t F, int max_len, int out_max_len, const ccmp_smooth_opts &o, const Outputs &out)
{
  { const int rc = traversal_checks(ctx, p, scene, margin, opts_ok(o)); if (rc != CCMP_OK) return rc; }
  if (max_len < 1 || out_max_len < max_len) return CCMP_EINVAL;
  if (F == 0) return CCMP_OK;
  if (F > kMaxRows / (size_t)out_max_len) return CCMP_EINVAL;
  if (!path_joints || !path_len || !out.joints || !out.len || !out.passes || !out.moved || !out.stop || !out.length_in || !out.length_out) return CCMP_EINVAL;
  const void *in[2] = {path_joints, path_len};
  const size_t in_n[2] = {F * (size_t)max_len * 14 * sizeof(double), F * sizeof(int32_t)};
  const void *outs[8] = {out.joints, out.len, out.passes, out.moved, out.stop, out.length_in, out.length_out, out.stats};
  const size_t out_n[8] = {F * (size_t)out_max_len * 14 * sizeof(double), F * sizeof(int32_t), F * sizeof(int32_t), F * sizeof(int32_t), F * sizeof(int32_t),
                           F * sizeof(double), F * sizeof(double), F * ccmp::kSmoothStats * sizeof(int32_t)};
  for (int a = 0; a < 8; a++)
    for (int b = 0; b < 2; b++)
      if (overlaps(outs[a], out_n[a], in[b], in_n[b])) return CCMP_EINVAL;
  return CCMP_OK;
}

// One midpoint step: E pairs [E][2][14] -> mid [E][14]; the kinds are counted into stats [F][5] at pair_path[e].
int midpoints(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_smooth_opts &o, const double *pairs, const int32_t *pair_path, size_t E, size_t F, double *mid,
              int32_t *stats, CallArena &mem, hipStream_t st)
{
  if (E == 0) return CCMP_OK;
  ccmp_dense_opts d;
  d.flags = CCMP_DENSE_DISTINCT;
  d.chunk_states = o.chunk_states;
  d.round_budget = o.round_budget;
  d.max_calls = o.max_calls;
  ccmp_dense_paths *h = nullptr;
  { const int rc = densify_rows(ctx, p, nullptr, 0.0, pairs, std::vector<int32_t>(E, 2), E, 2, d, &h, st); if (rc != CCMP_OK) return rc; }
  t_counts.calls += h->calls;
  t_counts.read_bytes += (long long)h->read_bytes;
  t_projects++;
  double *x = mem.array<double>(E * 14), *y = mem.array<double>(E * 14);
  int32_t *choice = mem.array<int32_t>(E);
  uint8_t *ok = mem.array<uint8_t>(E);
  int rc = mem.ok() ? CCMP_OK : CCMP_EHIP;
  hipError_t e = hipSuccess;
  if (rc == CCMP_OK) e = ccmp_launch::smooth_bracket(h->d_rows, h->arc, h->path_first, E, h->rows, x, choice, st);
  if (rc == CCMP_OK && e == hipSuccess) rc = ccmp_project_batch(ctx, p, x, y, ok, nullptr, E, st);
  if (rc == CCMP_OK && e == hipSuccess) e = ccmp_launch::smooth_pick(h->d_rows, h->path_first, choice, y, ok, pair_path, E, h->rows, F, mid, stats, st);
  const hipError_t es = hipStreamSynchronize(st); // the dense result goes before the step returns
  ccmp_dense_paths_destroy(h);
  if (rc != CCMP_OK) return rc;
  HIP_TRY(e);
  HIP_TRY(es);
  return CCMP_OK;
}

// The body of the device form behind its checks; `len0` = path_len as read once from the device.
int smooth(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
           const std::vector<int32_t> &len0, size_t F, int max_len, int cap, const ccmp_smooth_opts &o, const Outputs &out, hipStream_t st)
{
  t_counts = PairLoopCounts();
  t_projects = 0;
  t_counts.read_bytes = (long long)(F * (sizeof(int32_t) + 1)); // path_len and the finiteness flags, once
  CallArena mem(ctx, kArenaWhat); // what lives as long as the call: the two path buffers and the per-path arrays
  const size_t rows = F * (size_t)cap;
  double *buf[2] = {mem.array<double>(rows * 14), mem.array<double>(rows * 14)};
  double *w_len_in = mem.array<double>(F), *w_len_out = mem.array<double>(F);
  int32_t *w_stats = mem.array<int32_t>(F * ccmp::kSmoothStats), *w_moved = mem.array<int32_t>(F), *w_len = mem.array<int32_t>(F);
  int32_t *w_int = mem.array<int32_t>(F * 3); // passes, moved, stop as uploaded at the end
  uint8_t *w_bad = mem.array<uint8_t>(F), *w_where = mem.array<uint8_t>(F);
  if (!mem.ok()) return CCMP_EHIP;
  std::vector<uint8_t> bad(F, 0), where(F, 0);
  HIP_TRY(hipMemsetAsync(w_bad, 0, F, st));
  HIP_TRY(hipMemsetAsync(w_stats, 0, F * ccmp::kSmoothStats * sizeof(int32_t), st));
  HIP_TRY(hipMemsetAsync(w_moved, 0, F * sizeof(int32_t), st));
  HIP_TRY(ccmp_launch::smooth_load(path_joints, path_len, F, max_len, cap, buf[0], w_bad, st));
  HIP_TRY(ccmp_launch::smooth_length(buf[0], buf[0], nullptr, path_len, F, cap, w_len_in, st));
  { const int rc = read_back(bad.data(), w_bad, F, st); if (rc != CCMP_OK) return rc; }

  std::vector<int32_t> len(len0), passes(F, 0), moved(F, 0), stop(F, -1), moved_h(F, 0);
  for (size_t f = 0; f < F; f++) {
    if (bad[f]) stop[f] = ccmp::kSmoothStopNonFinite;
    else if (len[f] < 3) stop[f] = ccmp::kSmoothStopShort;
  }
  std::vector<smooth_path> act;
  for (;;) {
    act.clear();
    int32_t S = 0, V = 0;
    for (size_t f = 0; f < F; f++) {
      if (stop[f] >= 0) continue;
      if (passes[f] >= o.max_steps) { stop[f] = ccmp::kSmoothStopSteps; continue; }
      if (2 * (int64_t)len[f] - 1 > (int64_t)cap) { stop[f] = ccmp::kSmoothStopFull; continue; }
      act.push_back(smooth_path{(int32_t)f, len[f], S, V});
      S += len[f] - 1;
      V += len[f] - 2;
    }
    if (act.empty()) break;
    const size_t nA = act.size(), nS = (size_t)S, nV = (size_t)V;
    CallArena pm(ctx, kArenaWhat); // one pass's memory
    smooth_path *d_act = pm.array<smooth_path>(nA);
    double *pairs = pm.array<double>(2 * nV > nS ? 2 * nV * 28 : nS * 28), *m = pm.array<double>(nS * 14), *t12 = pm.array<double>(2 * nV * 14);
    double *cand = pm.array<double>(nV * 14), *from = pm.array<double>(2 * nV * 14), *to = pm.array<double>(2 * nV * 14);
    int32_t *pair_path = pm.array<int32_t>(2 * nV > nS ? 2 * nV : nS);
    uint8_t *test_ok = pm.array<uint8_t>(2 * nV);
    double *clear_m = scene ? pm.array<double>(nS) : nullptr, *clear_c = scene ? pm.array<double>(nV) : nullptr;
    if (!pm.ok()) return CCMP_EHIP;
    const double *cur = buf[0]; // the gather reads each active path from the buffer it is in: all active paths share one (they ran the same passes)
    const int side = where[act[0].f];
    cur = buf[side];
    HIP_TRY(hipMemcpyAsync(d_act, act.data(), nA * sizeof(smooth_path), hipMemcpyHostToDevice, st));
    // m_i for every segment
    HIP_TRY(ccmp_launch::smooth_gather(0, d_act, nA, nS, cur, cap, nullptr, nullptr, nullptr, pairs, nullptr, nullptr, pair_path, st));
    { const int rc = midpoints(ctx, p, o, pairs, pair_path, nS, F, m, w_stats, pm, st); if (rc != CCMP_OK) return rc; }
    // t1, t2 for every interior vertex
    HIP_TRY(ccmp_launch::smooth_gather(1, d_act, nA, 2 * nV, cur, cap, m, nullptr, nullptr, pairs, nullptr, nullptr, pair_path, st));
    { const int rc = midpoints(ctx, p, o, pairs, pair_path, 2 * nV, F, t12, w_stats, pm, st); if (rc != CCMP_OK) return rc; }
    // c_i
    HIP_TRY(ccmp_launch::smooth_gather(2, d_act, nA, nV, cur, cap, m, t12, nullptr, pairs, nullptr, nullptr, pair_path, st));
    { const int rc = midpoints(ctx, p, o, pairs, pair_path, nV, F, cand, w_stats, pm, st); if (rc != CCMP_OK) return rc; }
    // the two tests of every candidate
    HIP_TRY(ccmp_launch::smooth_gather(3, d_act, nA, 2 * nV, cur, cap, m, nullptr, cand, nullptr, from, to, nullptr, st));
    HIP_TRY(hipMemsetAsync(test_ok, 0, 2 * nV, st));
    {
      PairSource src;
      src.from = from; src.to = to;
      const int rc = pair_tests(ctx, p, scene, margin, PairLoopOpts{o.chunk_states, o.round_budget, o.max_calls, o.tile_edges}, 2 * (long long)nV, src, 2 * nV,
                                test_ok, nullptr, nullptr, pm, st, "ccmp_path_smooth", &t_counts);
      if (rc != CCMP_OK) return rc;
    }
    if (scene) {
      { const int rc = ccmp_clearance_batch(ctx, p, scene, m, nullptr, nS, margin, clear_m, nullptr, nullptr, st); if (rc != CCMP_OK) return rc; }
      { const int rc = ccmp_clearance_batch(ctx, p, scene, cand, nullptr, nV, margin, clear_c, nullptr, nullptr, st); if (rc != CCMP_OK) return rc; }
    }
    hipError_t e = hipMemsetAsync(w_moved, 0, F * sizeof(int32_t), st);
    if (e == hipSuccess)
      e = ccmp_launch::smooth_accept(d_act, nA, 2 * nS + nA, cur, cap, m, cand, test_ok, clear_m, clear_c, margin, o.min_change, buf[side ^ 1], w_moved, w_stats, st);
    if (e == hipSuccess) e = hipMemcpyAsync(moved_h.data(), w_moved, F * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    HIP_TRY(e);
    HIP_TRY(es);
    t_counts.read_bytes += (long long)(F * sizeof(int32_t));
    for (const smooth_path &a : act) {
      const size_t f = (size_t)a.f;
      passes[f]++;
      moved[f] += moved_h[f];
      len[f] = 2 * len[f] - 1;
      where[f] = (uint8_t)(side ^ 1);
      if (moved_h[f] == 0) stop[f] = ccmp::kSmoothStopStill;
    }
  }

  // every path has stopped: the lengths, then the caller's outputs
  std::vector<int32_t> ints(F * 3);
  for (size_t f = 0; f < F; f++) { ints[f] = passes[f]; ints[F + f] = moved[f]; ints[2 * F + f] = stop[f]; }
  HIP_TRY(hipMemcpyAsync(w_where, where.data(), F, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w_len, len.data(), F * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(w_int, ints.data(), F * 3 * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(ccmp_launch::smooth_length(buf[0], buf[1], w_where, w_len, F, cap, w_len_out, st));
  HIP_TRY(ccmp_launch::smooth_store(buf[0], buf[1], w_where, w_len, F, cap, out.joints, st));
  HIP_TRY(hipMemcpyAsync(out.len, w_len, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(out.passes, w_int, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(out.moved, w_int + F, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(out.stop, w_int + 2 * F, F * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(out.length_in, w_len_in, F * sizeof(double), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(out.length_out, w_len_out, F * sizeof(double), hipMemcpyDeviceToDevice, st));
  if (out.stats) HIP_TRY(hipMemcpyAsync(out.stats, w_stats, F * ccmp::kSmoothStats * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st)); // the call is synchronous: its workspace goes when it returns
  return CCMP_OK;
}

}  // namespace

extern "C" {

void ccmp_smooth_opts_default(ccmp_smooth_opts *opts)
{
  if (!opts) return;
  opts->max_steps = 5;
  opts->min_change = 0.005;
  opts->chunk_states = 16;
  opts->round_budget = 128;
  opts->max_calls = 4096;
  opts->tile_edges = 65536;
}

int ccmp_smooth_len_after(int L, int passes) { return ccmp::smooth_len_after(L, passes); }

void ccmp_smooth_last_counts(long long *extend_calls, long long *project_calls, long long *bytes_read)
{
  if (extend_calls) *extend_calls = t_counts.calls;
  if (project_calls) *project_calls = t_projects;
  if (bytes_read) *bytes_read = t_counts.read_bytes;
}

int ccmp_path_smooth(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                     size_t F, int max_len, const ccmp_smooth_opts *opts, int out_max_len, double *out_joints, int32_t *out_len, int32_t *passes,
                     int32_t *moved, int32_t *stop, double *length_in, double *length_out, int32_t *stats, void *hip_stream)
{
  if (!ctx) return no_handle();
  const ccmp_smooth_opts o = opts_or(opts, ccmp_smooth_opts_default);
  const Outputs out{out_joints, out_len, passes, moved, stop, length_in, length_out, stats};
  { const int rc = smooth_checks(ctx, p, scene, margin, path_joints, path_len, F, max_len, out_max_len, o, out); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<int32_t> len;
  { const int rc = read_lens(path_len, F, max_len, st, &len); if (rc != CCMP_OK) return rc; }
  return smooth(ctx, p, scene, margin, path_joints, path_len, len, F, max_len, out_max_len, o, out, st);
}

int ccmp_path_smooth_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                          size_t F, int max_len, const ccmp_smooth_opts *opts, int out_max_len, double *out_joints, int32_t *out_len, int32_t *passes,
                          int32_t *moved, int32_t *stop, double *length_in, double *length_out, int32_t *stats)
{
  if (!ctx) return no_handle();
  const ccmp_smooth_opts o = opts_or(opts, ccmp_smooth_opts_default);
  const Outputs out{out_joints, out_len, passes, moved, stop, length_in, length_out, stats};
  { const int rc = smooth_checks(ctx, p, scene, margin, path_joints, path_len, F, max_len, out_max_len, o, out); if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  { const int rc = lens_ok(path_len, F, max_len); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t in_rows = F * (size_t)max_len, out_rows = F * (size_t)out_max_len;
  CallArena mem(ctx, kArenaWhat); // the staging is memory of this call
  double *d_in = mem.array<double>(in_rows * 14), *d_out = mem.array<double>(out_rows * 14), *d_li = mem.array<double>(F), *d_lo = mem.array<double>(F);
  int32_t *d_len = mem.array<int32_t>(F), *d_ints = mem.array<int32_t>(F * 4), *d_stats = stats ? mem.array<int32_t>(F * ccmp::kSmoothStats) : nullptr;
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  sg.up(d_in, path_joints, in_rows * 14 * sizeof(double));
  sg.up(d_len, path_len, F * sizeof(int32_t));
  sg.up(d_out, out_joints, out_rows * 14 * sizeof(double)); // the caller's out_joints go up first: rows behind out_len stay the caller's
  { const int rc = sg.finish(CCMP_OK); if (rc != CCMP_OK) return rc; }
  const Outputs dev{d_out, d_ints, d_ints + F, d_ints + 2 * F, d_ints + 3 * F, d_li, d_lo, d_stats};
  const int rc = smooth(ctx, p, scene, margin, d_in, d_len, std::vector<int32_t>(path_len, path_len + F), F, max_len, out_max_len, o, dev, ctx->stream);
  if (rc != CCMP_OK) return rc; // (CCMP_EOVERFLOW at max_calls among them: no output is written)
  sg.down(out_joints, d_out, out_rows * 14 * sizeof(double));
  sg.down(out_len, d_ints, F * sizeof(int32_t));
  sg.down(passes, d_ints + F, F * sizeof(int32_t));
  sg.down(moved, d_ints + 2 * F, F * sizeof(int32_t));
  sg.down(stop, d_ints + 3 * F, F * sizeof(int32_t));
  sg.down(length_in, d_li, F * sizeof(double));
  sg.down(length_out, d_lo, F * sizeof(double));
  sg.down(stats, d_stats, F * ccmp::kSmoothStats * sizeof(int32_t));
  return sg.finish(CCMP_OK);
}

int ccmp_smooth_mid_ref(const double *rows, const double *arcs, int n, int *k, double *t, double *blend, int *fallback)
{
  if (!rows || !arcs || n < 2 || !k || !t || !blend || !fallback) return CCMP_EINVAL;
  bool lower;
  const bool live = ccmp::smooth_bracket(arcs, n, k, t, &lower);
  if (!live) { // degenerate: the midpoint is row 0
    *k = 0;
    *t = 0.0;
    *fallback = 0;
    memcpy(blend, rows, 14 * sizeof(double));
    return CCMP_OK;
  }
  *fallback = lower ? *k - 1 : *k;
  for (int c = 0; c < 14; c++) blend[c] = ccmp::smooth_interpolate(rows[(size_t)(*k - 1) * 14 + c], rows[(size_t)*k * 14 + c], *t);
  return CCMP_OK;
}

}  // extern "C"
