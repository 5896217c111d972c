// ccmp_dense.cpp — dense solution paths of the C ABI (include/ccmp.h: ccmp_path_densify, ccmp_dense_*): PathGeometric::interpolate over
// waypoint rows that are already on the device.  The rule is csrc/ccmp_dense.h.  The traversals are ccmp_geodesic_batch_ex's, unchanged:
// this unit owns the continuation loop — per round one endpoint gather and one extend launch over the open segments, one read of
// n_states / ok (5 bytes per open segment), the compaction of the open subset on those bytes — and keeps every call's list buffer on the
// device as chunks; the layout is computed on the host from the counts it has read anyway, then one pack launch moves the chunks and
// the waypoint rows to their final rows, one block per path sums the arc, and with a scene the clearance kernel runs once over all rows
// and one block per path reduces it.  The loop is bounded by max_calls; spent with a segment open, the call creates nothing.
#include <hip/hip_runtime.h>

#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_dense.h"
#include "ccmp_launch.h"
#include "ccmp_pair_tests.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"
#include "ccmp_stage.h"

using namespace ccmp_host;
using ccmp::dense_chunk;
using ccmp::dense_open_seg;

// (struct ccmp_dense_paths: ccmp_pair_tests.h — the smoothing's midpoint step reads a result's rows and arcs on the device)

namespace {

constexpr const char *kArenaWhat = "ccmp_path_densify: hipMalloc";

// The layout rule on the host (ccmp_dense.h): what ccmp_dense_layout_ref answers and what the device call lays its result out by.
int layout(const int32_t *path_len, size_t F, int max_len, const int32_t *seg_states, int distinct, int32_t *path_first, int32_t *seg_first, size_t *rows)
{
  const size_t W = (size_t)max_len - 1;
  int64_t row = 0;
  for (size_t f = 0; f < F; f++) {
    const int L = path_len[f];
    if (L < 0 || L > max_len) return CCMP_EINVAL;
    if (path_first) path_first[f] = (int32_t)row;
    int64_t states = 0;
    for (int i = 0; i + 1 < L; i++) {
      const int32_t n = seg_states ? seg_states[f * W + (size_t)i] : 0;
      if (n < 1) return CCMP_EINVAL;
      const int64_t first = row + ccmp::dense_seg_first(i, states, distinct);
      if ((uint64_t)first > kMaxRows) return CCMP_EOVERFLOW;
      if (seg_first) seg_first[f * W + (size_t)i] = (int32_t)first;
      states += n;
    }
    if (seg_first)
      for (size_t i = L > 1 ? (size_t)L - 1 : 0; i < W; i++) seg_first[f * W + i] = -1;
    row += ccmp::dense_path_rows(L, states, distinct);
    if ((uint64_t)row > kMaxRows) return CCMP_EOVERFLOW;
  }
  if (path_first) path_first[F] = (int32_t)row;
  *rows = (size_t)row;
  return CCMP_OK;
}

int opts_ok(const ccmp_dense_opts &o)
{
  if ((o.flags & ~CCMP_DENSE_DISTINCT) != 0 || o.chunk_states < 2 || o.round_budget < 0 || o.max_calls < 1) return CCMP_EINVAL;
  return CCMP_OK;
}

// what both forms check before anything touches the device
int densify_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                   size_t F, int max_len, const ccmp_dense_opts &o)
{
  { const int rc = traversal_checks(ctx, p, scene, margin, opts_ok(o)); if (rc != CCMP_OK) return rc; }
  if (F > 0 && (!path_joints || !path_len || max_len < 1)) return CCMP_EINVAL;
  if (F > 0 && F > kMaxRows / (size_t)max_len) return CCMP_EINVAL;
  return CCMP_OK;
}

// one extend call of the loop: its open segments (host copy kept until the call's upload has certainly been read) and its buffers
struct Round {
  std::vector<dense_open_seg> open;
  std::vector<int32_t> seg; // per open segment: its slot in [F][max_len - 1]
  double *states = nullptr, *carry = nullptr;
  int32_t *n = nullptr, *its = nullptr;
  uint8_t *ok = nullptr;
};

struct HostChunk {
  int32_t seg;
  const double *src;
  const int32_t *its;
  int32_t count;
};

// the result's one allocation
int make_handle(ccmp_ctx *ctx, size_t F, int max_len, size_t rows, bool has_scene, ccmp_dense_paths **out)
{
  ccmp_dense_paths *h = new (std::nothrow) ccmp_dense_paths();
  if (!h) return CCMP_ENOMEM;
  h->F = F;
  h->max_len = max_len;
  h->rows = rows;
  h->slots = F * (size_t)(max_len > 0 ? max_len - 1 : 0);
  h->has_scene = has_scene;
  const size_t R = rows ? rows : 1, S = h->slots ? h->slots : 1, P = F + 1;
  ResultBlock b;
  const size_t o_rows = b.take(R * 14 * sizeof(double)), o_arc = b.take(R * sizeof(double)), o_len = b.take(P * sizeof(double)),
               o_clr = b.take(has_scene ? R * sizeof(double) : 0), o_minc = b.take(has_scene ? P * sizeof(double) : 0), o_pf = b.take(P * sizeof(int32_t)),
               o_sf = b.take(S * sizeof(int32_t)), o_sn = b.take(S * sizeof(int32_t)), o_minr = b.take(has_scene ? P * sizeof(int32_t) : 0),
               o_fb = b.take(has_scene ? P * sizeof(int32_t) : 0), o_ok = b.take(S);
  { const int rc = b.alloc(h, ctx, kArenaWhat); if (rc != CCMP_OK) { delete h; return rc; } }
  h->d_rows = b.at<double>(o_rows);
  h->arc = b.at<double>(o_arc);
  h->length = b.at<double>(o_len);
  h->path_first = b.at<int32_t>(o_pf);
  h->seg_first = b.at<int32_t>(o_sf);
  h->seg_newton = b.at<int32_t>(o_sn);
  h->seg_ok = b.at<uint8_t>(o_ok);
  if (has_scene) {
    h->clearance = b.at<double>(o_clr);
    h->min_clear = b.at<double>(o_minc);
    h->min_row = b.at<int32_t>(o_minr);
    h->first_blocked = b.at<int32_t>(o_fb);
  }
  *out = h;
  return CCMP_OK;
}

// the body of the device form behind its checks; `len` = path_len as read once from the device.  On any failure *out stays NULL.
int densify(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const std::vector<int32_t> &len, size_t F,
            int max_len, const ccmp_dense_opts &o, ccmp_dense_paths **out, hipStream_t st)
{
  const int cs = o.chunk_states, distinct = (o.flags & CCMP_DENSE_DISTINCT) ? 1 : 0;
  const size_t W = F ? (size_t)max_len - 1 : 0, slots = F * W;
  std::vector<int32_t> seg_states(slots, 0);
  std::vector<uint8_t> seg_ok(slots, 0);
  std::vector<HostChunk> pieces;
  std::vector<Round> rounds; // kept whole until the end: their host arrays back uploads, their device arrays are the chunks
  CallArena arena(ctx, kArenaWhat); // every extend call's buffers live until the pack has run, then all of it goes at once
  int calls = 0;

  Round first;
  for (size_t f = 0; f < F; f++)
    for (int i = 0; i + 1 < len[f]; i++) {
      first.open.push_back(dense_open_seg{(int32_t)(f * (size_t)max_len + (size_t)i), -1, 0, 0});
      first.seg.push_back((int32_t)(f * W + (size_t)i));
    }
  rounds.reserve(16);
  rounds.push_back(std::move(first));
  std::vector<int32_t> n_h;
  std::vector<uint8_t> ok_h;
  while (!rounds.back().open.empty()) {
    if (calls == o.max_calls) { // a cut list must never look complete: nothing is created
      (void)hipStreamSynchronize(st);
      return CCMP_EOVERFLOW;
    }
    Round &r = rounds.back();
    const Round *prev = rounds.size() > 1 ? &rounds[rounds.size() - 2] : nullptr;
    const size_t E = r.open.size();
    dense_open_seg *d_open = arena.array<dense_open_seg>(E);
    double *from = arena.array<double>(E * 14), *to = arena.array<double>(E * 14);
    double *carry_in = prev ? arena.array<double>(E * 2) : nullptr;
    r.states = arena.array<double>(E * (size_t)cs * 14);
    r.carry = arena.array<double>(E * 2);
    r.n = arena.array<int32_t>(E);
    r.its = arena.array<int32_t>(E);
    r.ok = arena.array<uint8_t>(E);
    if (!arena.ok()) { (void)hipStreamSynchronize(st); return CCMP_EHIP; }
    hipError_t e = hipMemcpyAsync(d_open, r.open.data(), E * sizeof(dense_open_seg), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = ccmp_launch::dense_gather(d_open, E, path_joints, prev ? prev->states : nullptr, cs, prev ? prev->carry : nullptr, from, to, carry_in, st);
    int rc = CCMP_OK;
    if (e == hipSuccess)
      rc = ccmp_geodesic_batch_ex(ctx, p, from, to, E, cs, r.states, r.n, r.ok, r.its, carry_in, r.carry, o.round_budget, 0, st);
    n_h.resize(E);
    ok_h.resize(E);
    if (e == hipSuccess && rc == CCMP_OK) e = hipMemcpyAsync(n_h.data(), r.n, E * sizeof(int32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && rc == CCMP_OK) e = hipMemcpyAsync(ok_h.data(), r.ok, E, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (rc != CCMP_OK) return rc;
    HIP_TRY(e);
    HIP_TRY(es);
    calls++;
    Round next;
    const int take_from = prev ? 1 : 0; // a continuation's row 0 repeats the state it started from
    for (size_t k = 0; k < E; k++) {
      const int32_t stored = ccmp::dense_stored(n_h[k], cs);
      if (stored < 1) { snprintf(g_hip_err, sizeof g_hip_err, "ccmp_path_densify: an extend call stored no state"); return CCMP_EHIP; }
      const int32_t count = stored - take_from;
      pieces.push_back(HostChunk{r.seg[k], r.states + (k * (size_t)cs + (size_t)take_from) * 14, r.its + k, count});
      if ((size_t)seg_states[r.seg[k]] + (size_t)count > kMaxRows) return CCMP_EOVERFLOW;
      seg_states[r.seg[k]] += count;
      if (ccmp::dense_open(n_h[k], ok_h[k], cs)) {
        next.open.push_back(dense_open_seg{r.open[k].slot, (int32_t)k, stored - 1, 0});
        next.seg.push_back(r.seg[k]);
      } else {
        seg_ok[r.seg[k]] = ok_h[k];
      }
    }
    rounds.push_back(std::move(next));
  }

  // the layout, from the rule's text on the counts the loop has read
  std::vector<int32_t> path_first(F + 1, 0), seg_first(slots ? slots : 1, -1);
  size_t rows = 0;
  { const int rc = layout(len.data(), F, F ? max_len : 1, seg_states.data(), distinct, path_first.data(), seg_first.data(), &rows); if (rc != CCMP_OK) return rc; }
  std::vector<dense_chunk> chunks;
  chunks.reserve(pieces.size() + F * (size_t)(distinct ? 1 : (max_len > 0 ? max_len : 1)));
  for (size_t f = 0; f < F; f++) { // the waypoint rows: the leading copy of every segment's start (reference layout), the path's last waypoint
    const int L = len[f];
    if (!distinct)
      for (int i = 0; i + 1 < L; i++) chunks.push_back(dense_chunk{path_joints + (f * (size_t)max_len + (size_t)i) * 14, nullptr, 1, seg_first[f * W + (size_t)i] - 1, -1, 0});
    if (L > 0) chunks.push_back(dense_chunk{path_joints + (f * (size_t)max_len + (size_t)L - 1) * 14, nullptr, 1, path_first[f + 1] - 1, -1, 0});
  }
  {
    std::vector<int32_t> cursor(seg_first); // pieces are in call order per segment: each goes behind the one before
    for (const HostChunk &c : pieces) {
      chunks.push_back(dense_chunk{c.src, c.its, c.count, cursor[c.seg], c.seg, 0});
      cursor[c.seg] += c.count;
    }
  }
  ccmp_dense_paths *h = nullptr;
  { const int rc = make_handle(ctx, F, F ? max_len : 0, rows, scene != nullptr, &h); if (rc != CCMP_OK) return rc; }
  h->calls = calls;
  for (const Round &r : rounds) h->read_bytes += r.open.size() * 5;
  int rc = CCMP_OK;
  hipError_t e = hipMemcpyAsync(h->path_first, path_first.data(), (F + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && slots) e = hipMemcpyAsync(h->seg_first, seg_first.data(), slots * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && slots) e = hipMemcpyAsync(h->seg_ok, seg_ok.data(), slots, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && slots) e = hipMemsetAsync(h->seg_newton, 0, slots * sizeof(int32_t), st);
  if (e == hipSuccess && !chunks.empty()) {
    dense_chunk *d_chunks = arena.array<dense_chunk>(chunks.size());
    if (!d_chunks) rc = CCMP_EHIP;
    if (rc == CCMP_OK) e = hipMemcpyAsync(d_chunks, chunks.data(), chunks.size() * sizeof(dense_chunk), hipMemcpyHostToDevice, st);
    if (rc == CCMP_OK && e == hipSuccess) e = ccmp_launch::dense_pack(d_chunks, chunks.size(), h->d_rows, rows, h->seg_newton, slots, st);
  }
  if (rc == CCMP_OK && e == hipSuccess && F) e = ccmp_launch::dense_arc(h->d_rows, h->path_first, F, h->arc, h->length, st);
  if (rc == CCMP_OK && e == hipSuccess && scene && F) {
    if (rows) rc = ccmp_clearance_batch(ctx, p, scene, h->d_rows, nullptr, rows, margin, h->clearance, nullptr, nullptr, st);
    if (rc == CCMP_OK) e = ccmp_launch::dense_clearance_summary(h->clearance, h->path_first, F, margin, h->min_clear, h->min_row, h->first_blocked, st);
  }
  const hipError_t es = hipStreamSynchronize(st); // the call is synchronous: the host arrays above and the arena go when it returns
  if (rc == CCMP_OK && e != hipSuccess) rc = hip_fail(e, "ccmp_path_densify");
  if (rc == CCMP_OK && es != hipSuccess) rc = hip_fail(es, "ccmp_path_densify: hipStreamSynchronize");
  if (rc != CCMP_OK) { ccmp_dense_paths_destroy(h); return rc; }
  *out = h;
  return CCMP_OK;
}

}  // namespace

int ccmp_host::densify_rows(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints,
                            const std::vector<int32_t> &len, size_t F, int max_len, const ccmp_dense_opts &o, ccmp_dense_paths **out, hipStream_t st)
{
  return densify(ctx, p, scene, margin, path_joints, len, F, max_len, o, out, st);
}

extern "C" {

void ccmp_dense_opts_default(ccmp_dense_opts *opts)
{
  if (!opts) return;
  opts->flags = 0;
  opts->chunk_states = 16;
  opts->round_budget = 128;
  opts->max_calls = 4096;
}

int ccmp_path_densify(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                      size_t F, int max_len, const ccmp_dense_opts *opts, ccmp_dense_paths **out, void *hip_stream)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out) return CCMP_EINVAL;
  const ccmp_dense_opts o = opts_or(opts, ccmp_dense_opts_default);
  { const int rc = densify_checks(ctx, p, scene, margin, path_joints, path_len, F, max_len, o); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<int32_t> len;
  { const int rc = read_lens(path_len, F, max_len, st, &len); if (rc != CCMP_OK) return rc; }
  return densify(ctx, p, scene, margin, path_joints, len, F, max_len, o, out, st);
}

int ccmp_path_densify_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints,
                           const int32_t *path_len, size_t F, int max_len, const ccmp_dense_opts *opts, ccmp_dense_paths **out)
{
  if (out) *out = nullptr;
  if (!ctx) return no_handle();
  if (!out) return CCMP_EINVAL;
  const ccmp_dense_opts o = opts_or(opts, ccmp_dense_opts_default);
  { const int rc = densify_checks(ctx, p, scene, margin, path_joints, path_len, F, max_len, o); if (rc != CCMP_OK) return rc; }
  if (F) { const int rc = lens_ok(path_len, F, max_len); if (rc != CCMP_OK) return rc; }
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  CallArena mem(ctx, kArenaWhat); // the uploaded waypoints; released when the call returns (the result holds its own rows)
  double *d_joints = nullptr;
  if (F) {
    const size_t n = F * (size_t)max_len * 14;
    d_joints = mem.array<double>(n);
    if (!mem.ok()) return CCMP_EHIP;
    StagedCall sg(ctx, __func__);
    sg.up(d_joints, path_joints, n * sizeof(double));
    const int rc = sg.finish(CCMP_OK);
    if (rc != CCMP_OK) return rc;
  }
  return densify(ctx, p, scene, margin, d_joints, std::vector<int32_t>(path_len, path_len + F), F, max_len, o, out, ctx->stream);
}

int ccmp_dense_paths_info(const ccmp_dense_paths *h, size_t *F, int *max_len, size_t *rows, int *calls)
{
  if (!h) return CCMP_EINVAL;
  if (F) *F = h->F;
  if (max_len) *max_len = h->max_len;
  if (rows) *rows = h->rows;
  if (calls) *calls = h->calls;
  return CCMP_OK;
}

static int dense_copy(ccmp_dense_paths *h, double *rows_out, int32_t *path_first, int32_t *seg_first, uint8_t *seg_ok, int32_t *seg_newton, double *arc,
                      double *length, double *clearance, double *min_clear, int32_t *min_row, int32_t *first_blocked, hipMemcpyKind kind, hipStream_t st)
{
  const size_t R = h->rows, S = h->slots, F = h->F;
  if (rows_out && R) HIP_TRY(hipMemcpyAsync(rows_out, h->d_rows, R * 14 * sizeof(double), kind, st));
  if (path_first) HIP_TRY(hipMemcpyAsync(path_first, h->path_first, (F + 1) * sizeof(int32_t), kind, st));
  if (seg_first && S) HIP_TRY(hipMemcpyAsync(seg_first, h->seg_first, S * sizeof(int32_t), kind, st));
  if (seg_ok && S) HIP_TRY(hipMemcpyAsync(seg_ok, h->seg_ok, S, kind, st));
  if (seg_newton && S) HIP_TRY(hipMemcpyAsync(seg_newton, h->seg_newton, S * sizeof(int32_t), kind, st));
  if (arc && R) HIP_TRY(hipMemcpyAsync(arc, h->arc, R * sizeof(double), kind, st));
  if (length && F) HIP_TRY(hipMemcpyAsync(length, h->length, F * sizeof(double), kind, st));
  if (clearance && R) HIP_TRY(hipMemcpyAsync(clearance, h->clearance, R * sizeof(double), kind, st));
  if (min_clear && F) HIP_TRY(hipMemcpyAsync(min_clear, h->min_clear, F * sizeof(double), kind, st));
  if (min_row && F) HIP_TRY(hipMemcpyAsync(min_row, h->min_row, F * sizeof(int32_t), kind, st));
  if (first_blocked && F) HIP_TRY(hipMemcpyAsync(first_blocked, h->first_blocked, F * sizeof(int32_t), kind, st));
  return CCMP_OK;
}

int ccmp_dense_paths_copy(ccmp_dense_paths *h, double *rows_out, int32_t *path_first, int32_t *seg_first, uint8_t *seg_ok, int32_t *seg_newton, double *arc,
                          double *length, double *clearance, double *min_clear, int32_t *min_row, int32_t *first_blocked, void *hip_stream)
{
  if (!h) return no_handle();
  if (!h->has_scene && (clearance || min_clear || min_row || first_blocked)) return CCMP_EINVAL;
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  return dense_copy(h, rows_out, path_first, seg_first, seg_ok, seg_newton, arc, length, clearance, min_clear, min_row, first_blocked, hipMemcpyDeviceToDevice,
                    (hipStream_t)hip_stream);
}

int ccmp_dense_paths_copy_host(ccmp_dense_paths *h, double *rows_out, int32_t *path_first, int32_t *seg_first, uint8_t *seg_ok, int32_t *seg_newton,
                               double *arc, double *length, double *clearance, double *min_clear, int32_t *min_row, int32_t *first_blocked)
{
  if (!h) return no_handle();
  if (!h->has_scene && (clearance || min_clear || min_row || first_blocked)) return CCMP_EINVAL;
  if (!ccmp_host::context_alive(h->ctx)) return CCMP_EINVAL;
  DeviceGuard guard(h->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(h->ctx, __func__); // nothing staged: the copies (one list for both forms, dense_copy) come straight from the result
  const int rc = dense_copy(h, rows_out, path_first, seg_first, seg_ok, seg_newton, arc, length, clearance, min_clear, min_row, first_blocked,
                            hipMemcpyDeviceToHost, h->ctx->stream);
  return sg.finish(rc);
}

void ccmp_dense_paths_destroy(ccmp_dense_paths *h) { result_destroy(h); }

int ccmp_dense_layout_ref(const int32_t *path_len, size_t F, int max_len, const int32_t *seg_states, int flags, int32_t *path_first, int32_t *seg_first,
                          size_t *rows)
{
  if (!rows || (flags & ~CCMP_DENSE_DISTINCT) != 0 || max_len < 1) return CCMP_EINVAL;
  if (F > 0 && !path_len) return CCMP_EINVAL;
  if (F > kMaxRows / (size_t)max_len) return CCMP_EINVAL;
  return layout(path_len, F, max_len, seg_states, flags & CCMP_DENSE_DISTINCT, path_first, seg_first, rows);
}

int ccmp_dense_arc_ref(const double *rows, const int32_t *path_first, size_t F, double *arc, double *length)
{
  if (!path_first || path_first[0] < 0) return CCMP_EINVAL;
  for (size_t f = 0; f < F; f++)
    if (path_first[f + 1] < path_first[f]) return CCMP_EINVAL;
  if (path_first[F] > path_first[0] && (!rows || !arc)) return CCMP_EINVAL;
  for (size_t f = 0; f < F; f++) {
    double a = 0.0;
    for (int32_t r = path_first[f]; r < path_first[f + 1]; r++) {
      if (r > path_first[f]) a = ccmp::dense_arc_step(a, ccmp_joint_distance(rows + (size_t)(r - 1) * 14, rows + (size_t)r * 14));
      arc[r] = a;
    }
    if (length) length[f] = a;
  }
  return CCMP_OK;
}

}  // extern "C"
