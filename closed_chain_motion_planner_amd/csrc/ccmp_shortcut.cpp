// ccmp_shortcut.cpp — shortcut solution paths of the C ABI (include/ccmp.h: ccmp_path_shortcut, ccmp_shortcut_*): every pair of a path's
// waypoints is put to one checkMotion, then the cheapest path over the pairs that passed is taken.  The rule is csrc/ccmp_shortcut.h.  The
// traversals are ccmp_geodesic_batch_ex's (ccmp_geodesic_scene_batch's with a proxy scene), unchanged: this unit owns the loop over tiles of
// the enumeration and, per tile, the continuation loop — one extend launch over the open pairs, one scatter launch that adds what the call
// contributed to the pair's matrix entries, one read of n_states / ok (5 bytes per open pair, 6 with a scene), the compaction of the open
// subset on those bytes, one gather launch for the next call.  Nothing but an open pair's last stored state and carry survives a call: the
// two list buffers of a tile alternate.  The matrices are filled in a workspace of the call; only when every tile has closed does the
// selection run and anything reach the caller's outputs, so a call that spends max_calls leaves them untouched.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_launch.h"
#include "ccmp_pair_tests.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"
#include "ccmp_shortcut.h"
#include "ccmp_stage.h"

using namespace ccmp_host;
using ccmp::shortcut_best;
using ccmp::shortcut_open;

namespace {

constexpr size_t kMaxCells = (size_t)1 << 40; // F max_len^2 beyond this is an argument error, not an allocation to try

constexpr const char *kArenaWhat = "ccmp_path_shortcut: hipMalloc";

int opts_ok(const ccmp_shortcut_opts &o)
{
  if (o.max_span < 0 || o.chunk_states < 2 || o.round_budget < 0 || o.max_calls < 1 || o.tile_edges < 1) return CCMP_EINVAL;
  return CCMP_OK;
}

// the shapes, the required pointers and the overlap of outputs with inputs: shared by every form that has them
int select_checks(const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok_in, double *out_joints, int32_t *out_len,
                  int32_t *kept, double *cost_in, double *cost_out, uint8_t *pair_ok, int32_t *pair_states, int32_t *pair_newton)
{
  if (max_len < 1 || max_len > CCMP_SHORTCUT_MAX_LEN) return CCMP_EINVAL;
  if (F == 0) return CCMP_OK;
  if (F > kMaxCells / ((size_t)max_len * (size_t)max_len)) return CCMP_EINVAL;
  if (!path_joints || !path_len || !out_joints || !out_len || !kept || !cost_in || !cost_out) return CCMP_EINVAL;
  const size_t rows = F * (size_t)max_len, cells = rows * (size_t)max_len;
  const void *in[3] = {path_joints, path_len, pair_ok_in};
  const size_t in_n[3] = {rows * 14 * sizeof(double), F * sizeof(int32_t), pair_ok_in ? cells : 0};
  const void *out[8] = {out_joints, out_len, kept, cost_in, cost_out, pair_ok, pair_states, pair_newton};
  const size_t out_n[8] = {rows * 14 * sizeof(double), F * sizeof(int32_t), rows * sizeof(int32_t), F * sizeof(double), F * sizeof(double),
                           cells,                      cells * sizeof(int32_t), cells * sizeof(int32_t)};
  for (int a = 0; a < 8; a++)
    for (int b = 0; b < 3; b++)
      if (overlaps(out[a], out_n[a], in[b], in_n[b])) return CCMP_EINVAL;
  return CCMP_OK;
}

// one extend call's buffers; a tile has two and alternates
struct CallBufs {
  double *from = nullptr, *to = nullptr, *states = nullptr, *carry_out = nullptr, *carry_in = nullptr;
  int32_t *n = nullptr, *its = nullptr;
  uint8_t *ok = nullptr, *blocked = nullptr;
  shortcut_open *open = nullptr;
};

void make_bufs(CallArena &mem, size_t T, int cs, bool scene, CallBufs *b) // (the caller asks mem.ok() once)
{
  b->from = mem.array<double>(T * 14);
  b->to = mem.array<double>(T * 14);
  b->states = mem.array<double>(T * (size_t)cs * 14);
  b->carry_out = mem.array<double>(T * 2);
  b->carry_in = mem.array<double>(T * 2);
  b->n = mem.array<int32_t>(T);
  b->its = mem.array<int32_t>(T);
  b->ok = mem.array<uint8_t>(T);
  b->blocked = scene ? mem.array<uint8_t>(T) : nullptr;
  b->open = mem.array<shortcut_open>(T);
}

}  // namespace

// The tile and continuation loop (ccmp_pair_tests.h), shared with the smoothing's test step: only where a tile's endpoints come from differs.
int ccmp_host::pair_tests(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const PairLoopOpts &o, long long total,
                          const PairSource &src, size_t cells, uint8_t *w_ok, int32_t *w_states, int32_t *w_newton, CallArena &mem, hipStream_t st,
                          const char *what, PairLoopCounts *counts)
{
  if (total <= 0) return CCMP_OK;
  const int cs = o.chunk_states;
  const bool enumerated = src.from == nullptr;
  const size_t T_max = (size_t)((long long)o.tile_edges < total ? (long long)o.tile_edges : total);
  long long *d_cell = enumerated ? mem.array<long long>(T_max) : nullptr;
  CallBufs bufs[2];
  make_bufs(mem, T_max, cs, scene != nullptr, &bufs[0]);
  make_bufs(mem, T_max, cs, scene != nullptr, &bufs[1]);
  if (!mem.ok()) return CCMP_EHIP;
  std::vector<int32_t> n_h(T_max);
  std::vector<uint8_t> ok_h(T_max), bl_h(T_max, 0);
  std::vector<shortcut_open> open_h, next_h;
  std::vector<int32_t> slot_of(T_max); // per pair of the current call: its slot in the tile
  for (long long first = 0; first < total; first += (long long)T_max) {
    const size_t T = (size_t)(total - first < (long long)T_max ? total - first : (long long)T_max);
    size_t E = T;
    int cur = 0, calls = 0;
    bool cont = false; // the tile's first call reads its endpoints from the source
    for (size_t k = 0; k < T; k++) slot_of[k] = (int32_t)k;
    if (enumerated) {
      HIP_TRY(ccmp_launch::shortcut_enumerate(src.path_joints, src.path_len, src.d_prefix, src.F, src.max_len, src.max_span, first, T, d_cell, bufs[0].from,
                                              bufs[0].to, st));
    } else {
      HIP_TRY(hipMemcpyAsync(bufs[0].from, src.from + (size_t)first * 14, T * 14 * sizeof(double), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipMemcpyAsync(bufs[0].to, src.to + (size_t)first * 14, T * 14 * sizeof(double), hipMemcpyDeviceToDevice, st));
    }
    while (E > 0) {
      if (calls == o.max_calls) { // a cut traversal must never look complete: nothing reaches the outputs
        (void)hipStreamSynchronize(st);
        return CCMP_EOVERFLOW;
      }
      CallBufs &b = bufs[cur];
      int rc;
      if (scene)
        rc = ccmp_geodesic_scene_batch(ctx, p, scene, margin, b.from, b.to, E, cs, b.states, b.n, b.ok, b.its, b.blocked, nullptr, cont ? b.carry_in : nullptr,
                                       b.carry_out, o.round_budget, cont ? 0 : 1, st);
      else
        rc = ccmp_geodesic_batch_ex(ctx, p, b.from, b.to, E, cs, b.states, b.n, b.ok, b.its, cont ? b.carry_in : nullptr, b.carry_out, o.round_budget,
                                    cont ? 0 : 1, st);
      hipError_t e = hipSuccess;
      if (rc == CCMP_OK)
        e = ccmp_launch::shortcut_scatter(cont ? b.open : nullptr, E, d_cell, first, b.n, b.ok, b.its, b.blocked, cs, cells, w_ok, w_states, w_newton, st);
      if (e == hipSuccess && rc == CCMP_OK) e = hipMemcpyAsync(n_h.data(), b.n, E * sizeof(int32_t), hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && rc == CCMP_OK) e = hipMemcpyAsync(ok_h.data(), b.ok, E, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && rc == CCMP_OK && scene) e = hipMemcpyAsync(bl_h.data(), b.blocked, E, hipMemcpyDeviceToHost, st);
      const hipError_t es = hipStreamSynchronize(st);
      if (rc != CCMP_OK) return rc;
      HIP_TRY(e);
      HIP_TRY(es);
      calls++;
      if (counts) { counts->calls++; counts->read_bytes += (long long)E * (scene ? 6 : 5); }
      next_h.clear();
      for (size_t k = 0; k < E; k++) {
        if (bl_h[k] || !ccmp::dense_open(n_h[k], ok_h[k], cs)) continue;
        const int32_t stored = ccmp::dense_stored(n_h[k], cs);
        if (stored < 1) { snprintf(g_hip_err, sizeof g_hip_err, "%s: an extend call stored no state", what); return CCMP_EHIP; }
        next_h.push_back(shortcut_open{(int32_t)k, stored - 1, slot_of[k], 0});
      }
      E = next_h.size();
      if (E == 0) break;
      open_h.swap(next_h); // kept until the next synchronisation: it backs the upload below
      for (size_t k = 0; k < E; k++) slot_of[k] = open_h[k].slot;
      CallBufs &nb = bufs[cur ^ 1];
      HIP_TRY(hipMemcpyAsync(nb.open, open_h.data(), E * sizeof(shortcut_open), hipMemcpyHostToDevice, st));
      HIP_TRY(ccmp_launch::shortcut_regather(nb.open, E, b.states, cs, b.to, b.carry_out, nb.from, nb.to, nb.carry_in, st));
      cur ^= 1;
      cont = true;
    }
  }
  return CCMP_OK;
}

namespace {

// The body of the device form behind its checks; `len` = path_len as read once from the device.  The outputs are written only after every
// tile has closed.
int shortcut(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
             const std::vector<int32_t> &len, size_t F, int max_len, const ccmp_shortcut_opts &o, double *out_joints, int32_t *out_len, int32_t *kept,
             double *cost_in, double *cost_out, uint8_t *pair_ok, int32_t *pair_states, int32_t *pair_newton, hipStream_t st)
{
  const size_t cells = F * (size_t)max_len * (size_t)max_len;
  std::vector<long long> prefix(F + 1, 0);
  for (size_t f = 0; f < F; f++) prefix[f + 1] = prefix[f] + ccmp::shortcut_pair_count(len[f], o.max_span);
  const long long total = prefix[F];
  CallArena mem(ctx, kArenaWhat); // everything below lives until the call returns
  // the call's own matrices: the caller's stay untouched until the end
  uint8_t *w_ok = mem.array<uint8_t>(cells);
  int32_t *w_states = pair_states ? mem.array<int32_t>(cells) : nullptr;
  int32_t *w_newton = pair_newton ? mem.array<int32_t>(cells) : nullptr;
  if (!mem.ok()) return CCMP_EHIP;
  HIP_TRY(hipMemsetAsync(w_ok, 0, cells, st));
  if (w_states) HIP_TRY(hipMemsetAsync(w_states, 0, cells * sizeof(int32_t), st));
  if (w_newton) HIP_TRY(hipMemsetAsync(w_newton, 0, cells * sizeof(int32_t), st));

  if (total > 0) {
    long long *d_prefix = mem.array<long long>(F + 1);
    if (!mem.ok()) return CCMP_EHIP;
    HIP_TRY(hipMemcpyAsync(d_prefix, prefix.data(), (F + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    PairSource src;
    src.path_joints = path_joints; src.path_len = path_len; src.d_prefix = d_prefix; src.F = F; src.max_len = max_len; src.max_span = o.max_span;
    const int rc = pair_tests(ctx, p, scene, margin, PairLoopOpts{o.chunk_states, o.round_budget, o.max_calls, o.tile_edges}, total, src, cells, w_ok, w_states,
                              w_newton, mem, st, "ccmp_path_shortcut");
    if (rc != CCMP_OK) return rc;
  }

  // every pair is closed: the selection, then the caller's outputs
  HIP_TRY(ccmp_launch::shortcut_select(path_joints, path_len, F, max_len, w_ok, out_len, kept, cost_in, cost_out, st));
  HIP_TRY(ccmp_launch::shortcut_gather_kept(path_joints, out_len, kept, F, max_len, out_joints, st));
  if (pair_ok) HIP_TRY(hipMemcpyAsync(pair_ok, w_ok, cells, hipMemcpyDeviceToDevice, st));
  if (pair_states) HIP_TRY(hipMemcpyAsync(pair_states, w_states, cells * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  if (pair_newton) HIP_TRY(hipMemcpyAsync(pair_newton, w_newton, cells * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipStreamSynchronize(st)); // the call is synchronous: its workspace goes when it returns
  return CCMP_OK;
}

// the rule on host pointers, one thread (ccmp_shortcut_select_ref)
void select_one(const double *rows, int L, int max_len, const uint8_t *okm, double *out_rows, int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out)
{
  std::vector<double> d((size_t)(L > 0 ? L : 1));
  std::vector<int32_t> hops(d.size()), pred(d.size());
  for (int k = 0; k < max_len; k++) kept[k] = -1;
  double a = 0.0;
  for (int j = 1; j < L; j++) a = a + ccmp::graph_joint_dist(rows + (size_t)(j - 1) * 14, rows + (size_t)j * 14);
  *cost_in = a;
  if (L == 0) { *out_len = 0; *cost_out = 0.0; return; }
  d[0] = 0.0; hops[0] = 0; pred[0] = -1;
  for (int j = 1; j < L; j++) {
    shortcut_best b = ccmp::shortcut_none();
    for (int i = 0; i < j; i++) {
      if (!ccmp::shortcut_admitted(i, j, i + 1 == j ? 1 : okm[(size_t)i * (size_t)max_len + (size_t)j])) continue;
      ccmp::shortcut_relax(&b, i, d[i], hops[i], ccmp::graph_joint_dist(rows + (size_t)i * 14, rows + (size_t)j * 14));
    }
    const bool reached = b.pred != ccmp::kShortcutNoPred;
    d[j] = reached ? b.d : __builtin_inf();
    hops[j] = reached ? b.parent_hops + 1 : ccmp::kPathNoHops;
    pred[j] = reached ? b.pred : -1;
  }
  *cost_out = d[L - 1];
  if (hops[L - 1] == ccmp::kPathNoHops) { // unchanged
    for (int k = 0; k < L; k++) kept[k] = k;
    *out_len = L;
  } else {
    const int n = hops[L - 1] + 1;
    int v = L - 1;
    for (int k = n - 1; k >= 0 && v >= 0; k--) { kept[k] = v; v = pred[v]; }
    *out_len = n;
  }
  for (int k = 0; k < *out_len; k++) memcpy(out_rows + (size_t)k * 14, rows + (size_t)kept[k] * 14, 14 * sizeof(double));
}

}  // namespace

extern "C" {

void ccmp_shortcut_opts_default(ccmp_shortcut_opts *opts)
{
  if (!opts) return;
  opts->max_span = 0;
  opts->chunk_states = 16;
  opts->round_budget = 128;
  opts->max_calls = 4096;
  opts->tile_edges = 65536;
}

int ccmp_path_shortcut(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                       size_t F, int max_len, const ccmp_shortcut_opts *opts, double *out_joints, int32_t *out_len, int32_t *kept, double *cost_in,
                       double *cost_out, uint8_t *pair_ok, int32_t *pair_states, int32_t *pair_newton, void *hip_stream)
{
  if (!ctx) return no_handle();
  const ccmp_shortcut_opts o = opts_or(opts, ccmp_shortcut_opts_default);
  { const int rc = traversal_checks(ctx, p, scene, margin, opts_ok(o)); if (rc != CCMP_OK) return rc; }
  { const int rc = select_checks(path_joints, path_len, F, max_len, nullptr, out_joints, out_len, kept, cost_in, cost_out, pair_ok, pair_states, pair_newton);
    if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<int32_t> len;
  { const int rc = read_lens(path_len, F, max_len, st, &len); if (rc != CCMP_OK) return rc; }
  return shortcut(ctx, p, scene, margin, path_joints, path_len, len, F, max_len, o, out_joints, out_len, kept, cost_in, cost_out, pair_ok, pair_states,
                  pair_newton, st);
}

int ccmp_path_shortcut_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints,
                            const int32_t *path_len, size_t F, int max_len, const ccmp_shortcut_opts *opts, double *out_joints, int32_t *out_len,
                            int32_t *kept, double *cost_in, double *cost_out, uint8_t *pair_ok, int32_t *pair_states, int32_t *pair_newton)
{
  if (!ctx) return no_handle();
  const ccmp_shortcut_opts o = opts_or(opts, ccmp_shortcut_opts_default);
  { const int rc = traversal_checks(ctx, p, scene, margin, opts_ok(o)); if (rc != CCMP_OK) return rc; }
  { const int rc = select_checks(path_joints, path_len, F, max_len, nullptr, out_joints, out_len, kept, cost_in, cost_out, pair_ok, pair_states, pair_newton);
    if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  { const int rc = lens_ok(path_len, F, max_len); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t rows = F * (size_t)max_len, cells = rows * (size_t)max_len;
  CallArena mem(ctx, kArenaWhat); // the staging is memory of this call, not the context's block: it can be hundreds of megabytes
  double *d_in = mem.array<double>(rows * 14), *d_out = mem.array<double>(rows * 14), *d_ci = mem.array<double>(F), *d_co = mem.array<double>(F);
  int32_t *d_len = mem.array<int32_t>(F), *d_olen = mem.array<int32_t>(F), *d_kept = mem.array<int32_t>(rows);
  uint8_t *d_ok = pair_ok ? mem.array<uint8_t>(cells) : nullptr;
  int32_t *d_ps = pair_states ? mem.array<int32_t>(cells) : nullptr, *d_pn = pair_newton ? mem.array<int32_t>(cells) : nullptr;
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  sg.up(d_in, path_joints, rows * 14 * sizeof(double));
  sg.up(d_len, path_len, F * sizeof(int32_t));
  sg.up(d_out, out_joints, rows * 14 * sizeof(double)); // the caller's out_joints go up first: rows behind out_len stay the caller's
  { const int rc = sg.finish(CCMP_OK); if (rc != CCMP_OK) return rc; }
  const int rc = shortcut(ctx, p, scene, margin, d_in, d_len, std::vector<int32_t>(path_len, path_len + F), F, max_len, o, d_out, d_olen, d_kept, d_ci, d_co, d_ok,
                          d_ps, d_pn, ctx->stream);
  if (rc != CCMP_OK) return rc; // (CCMP_EOVERFLOW at max_calls among them: no output is written; the arena's hipFree waits for what is in flight)
  sg.down(out_joints, d_out, rows * 14 * sizeof(double));
  sg.down(out_len, d_olen, F * sizeof(int32_t));
  sg.down(kept, d_kept, rows * sizeof(int32_t));
  sg.down(cost_in, d_ci, F * sizeof(double));
  sg.down(cost_out, d_co, F * sizeof(double));
  sg.down(pair_ok, d_ok, cells);
  sg.down(pair_states, d_ps, cells * sizeof(int32_t));
  sg.down(pair_newton, d_pn, cells * sizeof(int32_t));
  return sg.finish(CCMP_OK);
}

int ccmp_shortcut_select(ccmp_ctx *ctx, const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok,
                         double *out_joints, int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out, void *hip_stream)
{
  if (!ctx) return no_handle();
  { const int rc = select_checks(path_joints, path_len, F, max_len, pair_ok, out_joints, out_len, kept, cost_in, cost_out, nullptr, nullptr, nullptr);
    if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  if (!pair_ok) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(ccmp_launch::shortcut_select(path_joints, path_len, F, max_len, pair_ok, out_len, kept, cost_in, cost_out, st));
  HIP_TRY(ccmp_launch::shortcut_gather_kept(path_joints, out_len, kept, F, max_len, out_joints, st));
  return CCMP_OK;
}

int ccmp_shortcut_select_host(ccmp_ctx *ctx, const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok,
                              double *out_joints, int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out)
{
  if (!ctx) return no_handle();
  { const int rc = select_checks(path_joints, path_len, F, max_len, pair_ok, out_joints, out_len, kept, cost_in, cost_out, nullptr, nullptr, nullptr);
    if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  if (!pair_ok) return CCMP_EINVAL;
  { const int rc = lens_ok(path_len, F, max_len); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t rows = F * (size_t)max_len, cells = rows * (size_t)max_len;
  CallArena mem(ctx, kArenaWhat); // memory of this call, as in ccmp_path_shortcut_host
  double *d_in = mem.array<double>(rows * 14), *d_out = mem.array<double>(rows * 14), *d_ci = mem.array<double>(F), *d_co = mem.array<double>(F);
  int32_t *d_len = mem.array<int32_t>(F), *d_olen = mem.array<int32_t>(F), *d_kept = mem.array<int32_t>(rows);
  uint8_t *d_ok = mem.array<uint8_t>(cells);
  if (!mem.ok()) return CCMP_EHIP;
  StagedCall sg(ctx, __func__);
  sg.up(d_in, path_joints, rows * 14 * sizeof(double));
  sg.up(d_len, path_len, F * sizeof(int32_t));
  sg.up(d_ok, pair_ok, cells);
  sg.up(d_out, out_joints, rows * 14 * sizeof(double)); // the caller's out_joints go up first: rows behind out_len stay the caller's
  if (sg.copy_ok()) sg.note(ccmp_launch::shortcut_select(d_in, d_len, F, max_len, d_ok, d_olen, d_kept, d_ci, d_co, ctx->stream));
  if (sg.copy_ok()) sg.note(ccmp_launch::shortcut_gather_kept(d_in, d_olen, d_kept, F, max_len, d_out, ctx->stream));
  sg.down(out_joints, d_out, rows * 14 * sizeof(double));
  sg.down(out_len, d_olen, F * sizeof(int32_t));
  sg.down(kept, d_kept, rows * sizeof(int32_t));
  sg.down(cost_in, d_ci, F * sizeof(double));
  sg.down(cost_out, d_co, F * sizeof(double));
  return sg.finish(CCMP_OK);
}

int ccmp_shortcut_select_ref(const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok, double *out_joints,
                             int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out)
{
  { const int rc = select_checks(path_joints, path_len, F, max_len, pair_ok, out_joints, out_len, kept, cost_in, cost_out, nullptr, nullptr, nullptr);
    if (rc != CCMP_OK) return rc; }
  if (F == 0) return CCMP_OK;
  if (!pair_ok) return CCMP_EINVAL;
  { const int rc = lens_ok(path_len, F, max_len); if (rc != CCMP_OK) return rc; }
  for (size_t f = 0; f < F; f++)
    select_one(path_joints + f * (size_t)max_len * 14, path_len[f], max_len, pair_ok + f * (size_t)max_len * (size_t)max_len,
               out_joints + f * (size_t)max_len * 14, out_len + f, kept + f * (size_t)max_len, cost_in + f, cost_out + f);
  return CCMP_OK;
}

int ccmp_shortcut_pairs_ref(const double *path_joints, const int32_t *path_len, size_t F, int max_len, int max_span, int32_t *triples, size_t capacity,
                            size_t *count)
{
  if (!count || max_len < 1 || max_len > CCMP_SHORTCUT_MAX_LEN || max_span < 0) return CCMP_EINVAL;
  *count = 0;
  if (F == 0) return CCMP_OK;
  if (!path_joints || !path_len || F > (size_t)0x7fffffff) return CCMP_EINVAL;
  { const int rc = lens_ok(path_len, F, max_len); if (rc != CCMP_OK) return rc; }
  size_t n = 0;
  for (size_t f = 0; f < F; f++) {
    const int L = path_len[f];
    const double *rows = path_joints + f * (size_t)max_len * 14;
    const long long slots = ccmp::shortcut_pair_count(L, max_span);
    for (long long r = 0; r < slots; r++) { // the enumeration the device walks, slot by slot
      int i, j;
      ccmp::shortcut_pair_of(L, max_span, r, &i, &j);
      if (!ccmp::shortcut_row_finite(rows + (size_t)i * 14) || !ccmp::shortcut_row_finite(rows + (size_t)j * 14)) continue;
      if (triples && n < capacity) { triples[n * 3] = (int32_t)f; triples[n * 3 + 1] = i; triples[n * 3 + 2] = j; }
      n++;
    }
  }
  *count = n;
  return (triples && n > capacity) ? CCMP_EOVERFLOW : CCMP_OK;
}

}  // extern "C"
