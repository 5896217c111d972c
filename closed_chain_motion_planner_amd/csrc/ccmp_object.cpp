// ccmp_object.cpp — the head of growTree in the C ABI (include/ccmp.h: ccmp_object_*, ccmp_pose_interpolate).  The arithmetic is
// csrc/ccmp_object.h, one text: the *_ref entries run it here on the host (no device; the checker of the GPU tests and the CPU contender
// of tools/measure.py object), the *_batch entries launch object_valid_kernel / object_propose_kernel (ccmp_kernels_object.hip) on it.
// Every check runs before the first launch; the kernels need no workspace.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_launch.h"
#include "ccmp_object.h"
#include "ccmp_plan.h"
#include "ccmp_resident.h"
#include "ccmp_stage.h"

using namespace ccmp_host;

struct ccmp_object {
  int device = 0;
  ccmp_ctx *ctx = nullptr; // the context it was created on: its resident service kernel is stopped before the object's hipFree, as for scenes
  int M = 0, n_boxes = 0;
  size_t plane = 0;        // doubles per coordinate plane (M rounded up to 32: 256-byte rows)
  ccmp::object_boxes boxes;
  ccmp::object_sphere sphere;
  double *tri = nullptr;   // device, [9][plane]
};

namespace {

// the mesh and the boxes of a create / _ref call -> what the kernels take
int object_checks(const double *tri, int M, const ccmp_box *boxes, int n_boxes, ccmp::object_boxes *B, ccmp::object_sphere *S)
{
  if (M < 1 || M > CCMP_OBJECT_MAX_TRIANGLES || n_boxes < 1 || n_boxes > CCMP_MAX_BOXES || !tri || !boxes) return CCMP_EINVAL;
  memset(B, 0, sizeof *B);
  for (int b = 0; b < n_boxes; b++) {
    const ccmp_box &x = boxes[b];
    ccmp::object_box &o = B->b[b];
    double mag = 0.0;
    for (int k = 0; k < 3; k++) {
      if (!std::isfinite(x.c[k]) || !std::isfinite(x.half[k]) || x.half[k] < 0.0) return CCMP_EINVAL;
      o.c[k] = x.c[k];
      o.h[k] = x.half[k];
      mag += std::fabs(x.c[k]) + x.half[k];
    }
    for (int k = 0; k < 9; k++) {
      if (!std::isfinite(x.R[k])) return CCMP_EINVAL;
      o.R[k] = x.R[k];
    }
    o.mag = mag;
  }
  double lo[3], hi[3], big = 0.0;
  for (size_t w = 0; w < (size_t)M * 9; w++) {
    const double v = tri[w];
    if (!std::isfinite(v)) return CCMP_EINVAL;
    const int k = (int)(w % 3);
    if (w < 3 || v < lo[k]) lo[k] = v;
    if (w < 3 || v > hi[k]) hi[k] = v;
    if (std::fabs(v) > big) big = std::fabs(v);
  }
  for (int k = 0; k < 3; k++) S->c[k] = 0.5 * lo[k] + 0.5 * hi[k];
  double r2 = 0.0;
  for (size_t w = 0; w < (size_t)M * 9; w += 3) {
    const double d0 = tri[w] - S->c[0], d1 = tri[w + 1] - S->c[1], d2 = tri[w + 2] - S->c[2];
    const double q = d0 * d0 + d1 * d1 + d2 * d2;
    if (q > r2) r2 = q;
  }
  S->r = std::sqrt(r2) * (1.0 + 1e-6) + 1e-9 * (1.0 + big); // never below the true radius (ccmp_object.h: broad phase)
  if (!std::isfinite(S->r)) return CCMP_EINVAL;
  return CCMP_OK;
}

int draw_checks(int to_stride, double t, double sigma, const double *lo, const double *hi, int attempts, uint64_t rng_seed, uint64_t first_index, double inflate,
                ccmp::object_draw *D)
{
  if ((to_stride != 0 && to_stride != 8) || attempts < 1 || attempts > CCMP_OBJECT_MAX_ATTEMPTS || !lo || !hi) return CCMP_EINVAL;
  if (!std::isfinite(t) || !std::isfinite(sigma) || sigma < 0.0 || !std::isfinite(inflate) || inflate < 0.0) return CCMP_EINVAL;
  if (ccmp::object_rot_dev(sigma) > ccmp::kObjectRotDevMax) return CCMP_EINVAL;
  for (int k = 0; k < 3; k++) {
    if (std::isnan(lo[k]) || std::isnan(hi[k]) || lo[k] > hi[k]) return CCMP_EINVAL;
    D->lo[k] = lo[k];
    D->hi[k] = hi[k];
  }
  D->t = t;
  D->sigma = sigma;
  D->inflate = inflate;
  D->rng_seed = rng_seed;
  D->first_index = first_index;
  D->attempts = attempts;
  D->to_stride = to_stride;
  return CCMP_OK;
}

bool inflate_ok(double inflate) { return std::isfinite(inflate) && inflate >= 0.0; }
constexpr size_t kMaxBlocks = (size_t)1 << 31; // one block per pose / grow index

ccmp_launch::ObjectCall call_of(const ccmp_object *o) { return ccmp_launch::ObjectCall{&o->boxes, &o->sphere, o->tri, o->M, o->plane, o->n_boxes}; }

// what every device form checks about its handles; CCMP_OK or the code to return
int handles_ok(const ccmp_ctx *ctx, const ccmp_object *obj)
{
  if (!ctx) return no_handle();
  if (!obj || obj->device != ctx->device) return CCMP_EINVAL;
  return CCMP_OK;
}

void nan_row(double *row)
{
  for (int i = 0; i < 7; i++) row[i] = __builtin_nan("");
  row[7] = 0.0;
}

}  // namespace

extern "C" {

void ccmp_pose_interpolate(const double a[8], const double b[8], double t, double out[8]) { ccmp::pose_interpolate(a, b, t, out); }

int ccmp_object_create(ccmp_ctx *ctx, const double *tri, int M, const ccmp_box *boxes, int n_boxes, ccmp_object **out)
{
  if (!out) return CCMP_EINVAL;
  *out = nullptr;
  ccmp_object *o = new (std::nothrow) ccmp_object();
  if (!o) return CCMP_ENOMEM;
  { const int rc = object_checks(tri, M, boxes, n_boxes, &o->boxes, &o->sphere); if (rc != CCMP_OK) { delete o; return rc; } }
  if (!ctx) { delete o; return no_handle(); }
  o->device = ctx->device;
  o->M = M;
  o->n_boxes = n_boxes;
  o->plane = ((size_t)M + 31) & ~(size_t)31;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) { delete o; return CCMP_ENODEV; }
  ccmp_host::quiesce(ctx);
  double *rows = nullptr;
  const size_t row_bytes = (size_t)M * 9 * sizeof(double), plane_bytes = o->plane * 9 * sizeof(double);
  hipError_t e = hipMalloc((void **)&o->tri, plane_bytes);
  if (e == hipSuccess) e = hipMalloc((void **)&rows, row_bytes);
  if (e == hipSuccess) e = hipMemsetAsync(o->tri, 0, plane_bytes, ctx->stream); // the planes' padding; in stream order ahead of the kernel below
  if (e == hipSuccess) e = hipMemcpy(rows, tri, row_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = ccmp_launch::object_planes(rows, M, o->plane, o->tri, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (rows) (void)hipFree(rows);
  if (e != hipSuccess) {
    if (o->tri) (void)hipFree(o->tri);
    delete o;
    return hip_fail(e, "ccmp_object_create");
  }
  o->ctx = ctx;
  *out = o;
  return CCMP_OK;
}

void ccmp_object_destroy(ccmp_object *obj)
{
  if (!obj) return;
  {
    DeviceGuard guard(obj->device);
    if (obj->ctx && ccmp_host::context_alive(obj->ctx)) ccmp_host::quiesce(obj->ctx);
    if (obj->tri) (void)hipFree(obj->tri);
  }
  delete obj;
}

int ccmp_object_num_triangles(const ccmp_object *obj) { return obj ? obj->M : 0; }

int ccmp_object_valid_ref(const double *tri, int M, const ccmp_box *boxes, int n_boxes, const double *poses, size_t T, double inflate, int broad_phase,
                          uint8_t *valid, uint32_t *hit_mask)
{
  ccmp::object_boxes B;
  ccmp::object_sphere S;
  { const int rc = object_checks(tri, M, boxes, n_boxes, &B, &S); if (rc != CCMP_OK) return rc; }
  if (!inflate_ok(inflate) || T >= kMaxBlocks) return CCMP_EINVAL;
  if (T == 0) return CCMP_OK;
  if (!poses || !valid) return CCMP_EINVAL;
  for (size_t t = 0; t < T; t++) {
    bool finite;
    const uint32_t mask = ccmp::object_pose_mask(poses + t * 8, tri, M, S, B, n_boxes, inflate, broad_phase != 0, &finite);
    valid[t] = finite && mask == 0u ? 1 : 0;
    if (hit_mask) hit_mask[t] = mask;
  }
  return CCMP_OK;
}

int ccmp_object_valid_batch(ccmp_ctx *ctx, const ccmp_object *obj, const double *poses, size_t T, double inflate, uint8_t *valid, uint32_t *hit_mask,
                            void *hip_stream)
{
  { const int rc = handles_ok(ctx, obj); if (rc != CCMP_OK) return rc; }
  if (!inflate_ok(inflate) || T >= kMaxBlocks) return CCMP_EINVAL;
  if (T == 0) return CCMP_OK;
  if (!poses || !valid) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  HIP_TRY(ccmp_launch::object_valid(call_of(obj), poses, T, inflate, valid, hit_mask, (hipStream_t)hip_stream));
  return CCMP_OK;
}

// the same on host buffers: synchronous on the context's stream
int ccmp_object_valid_host(ccmp_ctx *ctx, const ccmp_object *obj, const double *poses, size_t T, double inflate, uint8_t *valid, uint32_t *hit_mask)
{
  { const int rc = handles_ok(ctx, obj); if (rc != CCMP_OK) return rc; }
  if (!inflate_ok(inflate) || T >= kMaxBlocks) return CCMP_EINVAL;
  if (T == 0) return CCMP_OK;
  if (!poses || !valid) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  StagedCall sg(ctx, __func__);
  const size_t off_p = sg.add(T * 8 * sizeof(double)), off_m = sg.add(hit_mask ? T * sizeof(uint32_t) : 0), off_v = sg.add(T);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_p, poses, T * 8 * sizeof(double));
  if (sg.copy_ok())
    sg.note(ccmp_launch::object_valid(call_of(obj), sg.at<const double>(off_p), T, inflate, sg.at<uint8_t>(off_v), sg.at<uint32_t>(off_m, hit_mask), ctx->stream));
  sg.down(valid, off_v, T);
  sg.down(hit_mask, off_m, T * sizeof(uint32_t));
  return sg.finish(CCMP_OK); // waits on the error path too: the staging block must be quiet
}

int ccmp_object_propose_ref(const double *tri, int M, const ccmp_box *boxes, int n_boxes, const double *from_poses, const double *to_poses, int to_stride,
                            size_t G, double t, double sigma, const double lo[3], const double hi[3], int attempts, uint64_t rng_seed, uint64_t first_index,
                            double inflate, double *pose_out, int32_t *which, double *cand_pose, uint8_t *cand_valid)
{
  ccmp::object_boxes B;
  ccmp::object_sphere S;
  ccmp::object_draw D;
  { const int rc = object_checks(tri, M, boxes, n_boxes, &B, &S); if (rc != CCMP_OK) return rc; }
  { const int rc = draw_checks(to_stride, t, sigma, lo, hi, attempts, rng_seed, first_index, inflate, &D); if (rc != CCMP_OK) return rc; }
  if (G >= kMaxBlocks) return CCMP_EINVAL;
  if (G == 0) return CCMP_OK;
  if (!from_poses || !to_poses || !pose_out || !which) return CCMP_EINVAL;
  const bool report = cand_pose || cand_valid;
  for (size_t g = 0; g < G; g++) {
    int chosen = -1;
    for (int a = 0; a < attempts; a++) {
      double cand[8];
      ccmp::object_candidate(from_poses + g * 8, to_poses + g * (size_t)to_stride, D, (uint64_t)g, a, cand);
      bool finite;
      const uint32_t mask = ccmp::object_pose_mask(cand, tri, M, S, B, n_boxes, inflate, true, &finite);
      const bool ok = finite && mask == 0u;
      const size_t c = g * (size_t)attempts + (size_t)a;
      if (cand_pose) memcpy(cand_pose + c * 8, cand, sizeof cand);
      if (cand_valid) cand_valid[c] = ok ? 1 : 0;
      if (ok && chosen < 0) {
        chosen = a;
        memcpy(pose_out + g * 8, cand, sizeof cand);
      }
      if (chosen >= 0 && !report) break;
    }
    which[g] = chosen;
    if (chosen < 0) nan_row(pose_out + g * 8);
  }
  return CCMP_OK;
}

int ccmp_object_propose_batch(ccmp_ctx *ctx, const ccmp_object *obj, const double *from_poses, const double *to_poses, int to_stride, size_t G, double t,
                              double sigma, const double lo[3], const double hi[3], int attempts, uint64_t rng_seed, uint64_t first_index, double inflate,
                              double *pose_out, int32_t *which, double *cand_pose, uint8_t *cand_valid, void *hip_stream)
{
  { const int rc = handles_ok(ctx, obj); if (rc != CCMP_OK) return rc; }
  ccmp::object_draw D;
  { const int rc = draw_checks(to_stride, t, sigma, lo, hi, attempts, rng_seed, first_index, inflate, &D); if (rc != CCMP_OK) return rc; }
  if (G >= kMaxBlocks) return CCMP_EINVAL;
  if (G == 0) return CCMP_OK;
  if (!from_poses || !to_poses || !pose_out || !which) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  HIP_TRY(ccmp_launch::object_propose(call_of(obj), D, from_poses, to_poses, G, pose_out, which, cand_pose, cand_valid, (hipStream_t)hip_stream));
  return CCMP_OK;
}

// the same on host buffers: synchronous on the context's stream
int ccmp_object_propose_host(ccmp_ctx *ctx, const ccmp_object *obj, const double *from_poses, const double *to_poses, int to_stride, size_t G, double t,
                             double sigma, const double lo[3], const double hi[3], int attempts, uint64_t rng_seed, uint64_t first_index, double inflate,
                             double *pose_out, int32_t *which, double *cand_pose, uint8_t *cand_valid)
{
  { const int rc = handles_ok(ctx, obj); if (rc != CCMP_OK) return rc; }
  ccmp::object_draw D;
  { const int rc = draw_checks(to_stride, t, sigma, lo, hi, attempts, rng_seed, first_index, inflate, &D); if (rc != CCMP_OK) return rc; }
  if (G >= kMaxBlocks) return CCMP_EINVAL;
  if (G == 0) return CCMP_OK;
  if (!from_poses || !to_poses || !pose_out || !which) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const size_t C = G * (size_t)attempts, gb = G * 8 * sizeof(double), tb = (to_stride ? G : 1) * 8 * sizeof(double); // stride 0: one target for all
  StagedCall sg(ctx, __func__);
  const size_t off_f = sg.add(gb), off_t = sg.add(tb), off_o = sg.add(gb), off_w = sg.add(G * sizeof(int32_t)), off_cp = sg.add(cand_pose ? C * 8 * sizeof(double) : 0),
               off_cv = sg.add(cand_valid ? C : 0);
  { const int rc = sg.alloc(); if (rc != CCMP_OK) return rc; }
  sg.up(off_f, from_poses, gb);
  sg.up(off_t, to_poses, tb);
  if (sg.copy_ok())
    sg.note(ccmp_launch::object_propose(call_of(obj), D, sg.at<const double>(off_f), sg.at<const double>(off_t), G, sg.at<double>(off_o), sg.at<int32_t>(off_w),
                                        sg.at<double>(off_cp, cand_pose), sg.at<uint8_t>(off_cv, cand_valid), ctx->stream));
  sg.down(pose_out, off_o, gb);
  sg.down(which, off_w, G * sizeof(int32_t));
  sg.down(cand_pose, off_cp, C * 8 * sizeof(double));
  sg.down(cand_valid, off_cv, C);
  return sg.finish(CCMP_OK); // waits on the error path too: the staging block must be quiet
}

}  // extern "C"

// what the planner's loop (ccmp_plan.cpp; declared in ccmp_plan.h) checks of an object before its first launch
namespace ccmp_host {
int object_device(const ccmp_object *obj) { return obj->device; }
}  // namespace ccmp_host
