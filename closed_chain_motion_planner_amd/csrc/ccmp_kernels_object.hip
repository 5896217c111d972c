// ccmp_kernels_object.hip — the head of growTree on the device (csrc/ccmp_object.h holds the arithmetic, one text for host and device):
// object_valid_kernel, the mesh-against-workspace test of one pose per 256-lane block with the triangles strided over the lanes, and
// object_propose_kernel, interpolate -> Gaussian draw -> that test, attempt by attempt, one block per grow index.  Built with the k-NN
// unit's flags (build.py); no scratch (_SCRATCH_RULES), two words of LDS.
//
// What is uniform: the pose (read at an address formed from blockIdx and kernel arguments, or computed from such values by every lane
// alike), its rotation matrix, the boxes (a kernel argument) and the set of boxes that survived the broad phase — so the loop over the
// boxes, the loop over the chunks and every exit are taken by a block as a whole, and each barrier is met by all 256 lanes.  What
// differs per lane is its triangle alone.
#include <hip/hip_runtime.h>

#include "ccmp_launch.h"
#include "ccmp_object.h"

namespace {

constexpr int kThreads = ccmp_launch::kObjectThreads;

// The block's hit mask of one pose whose frame (R, p) is finite.  tri: nine planes of `plane` doubles (x0 y0 z0 x1 ... z2), triangle m
// at plane index m.  early == false: every chunk runs and the mask is complete.  early == true: the block leaves after the first chunk in
// which any lane hit (the reference's early `return false`); the mask is then that chunk's and earlier ones', non-zero exactly when the
// complete one is.  lds: two words.  Every lane returns the same value.  At most ceil(M / 256) <= 64 chunks.
__device__ __forceinline__ uint32_t block_hit_mask(const double *__restrict__ tri, int M, size_t plane, const double *R, const double *p,
                                                   const ccmp::object_boxes &B, int n_boxes, uint32_t live, double inflate, bool early, unsigned int *lds)
{
  if (threadIdx.x == 0) { lds[0] = 0u; lds[1] = 0u; }
  __syncthreads();
  uint32_t wave_mask = 0u, block_mask = 0u;
  if (live != 0u) {
    int chunk = 0;
    for (int base = 0; base < M; base += kThreads, chunk++) {
      const int m = base + (int)threadIdx.x;
      uint32_t mine = 0u;
      if (m < M) {
        double w0[3], w1[3], w2[3];
        ccmp::object_to_world(R, p, tri[m], tri[plane + m], tri[2 * plane + m], w0);
        ccmp::object_to_world(R, p, tri[3 * plane + m], tri[4 * plane + m], tri[5 * plane + m], w1);
        ccmp::object_to_world(R, p, tri[6 * plane + m], tri[7 * plane + m], tri[8 * plane + m], w2);
        for (int b = 0; b < n_boxes; b++)
          if (((live >> b) & 1u) && ccmp::tri_box_hit(w0, w1, w2, B.b[b], inflate)) mine |= 1u << b;
      }
      for (int b = 0; b < n_boxes; b++)
        if (__builtin_amdgcn_ballot_w64(((mine >> b) & 1u) != 0u) != 0ull) wave_mask |= 1u << b;
      if (early) {
        // chunk c publishes in word c & 1: a wavefront that is already in chunk c + 1 writes the other word, and none reaches chunk
        // c + 2 before all have read word c & 1 behind this barrier.  The block goes on only while both words are still 0.
        unsigned int *word = lds + (chunk & 1);
        if ((threadIdx.x & 63) == 0 && wave_mask != 0u) atomicOr(word, wave_mask);
        __syncthreads();
        block_mask = *word;
        if (block_mask != 0u) break;
      }
    }
  }
  if (!early) {
    if ((threadIdx.x & 63) == 0 && wave_mask != 0u) atomicOr(lds, wave_mask);
    __syncthreads();
    block_mask = lds[0];
  }
  __syncthreads(); // the words are cleared again by the next test of this block
  return block_mask;
}

// One block per pose.  hit_mask != NULL: the complete mask; NULL: the early form.  valid is the same in both.
__global__ __launch_bounds__(kThreads) void object_valid_kernel(const ccmp::object_boxes B, const ccmp::object_sphere S, const double *__restrict__ tri, int M,
                                                                unsigned long long plane, int n_boxes, const double *__restrict__ poses, double inflate,
                                                                uint8_t *__restrict__ valid, uint32_t *__restrict__ hit_mask)
{
  __shared__ unsigned int lds[2];
  const size_t t = blockIdx.x;
  double pose[8], R[9], p[3];
#pragma unroll
  for (int i = 0; i < 8; i++) pose[i] = poses[t * 8 + i];
  if (!ccmp::object_frame(pose, R, p)) {
    if (threadIdx.x == 0) {
      valid[t] = 0;
      if (hit_mask) hit_mask[t] = 0u;
    }
    return;
  }
  const uint32_t live = ccmp::object_live_boxes(pose, R, p, S, B, n_boxes, inflate, true);
  const uint32_t mask = block_hit_mask(tri, M, (size_t)plane, R, p, B, n_boxes, live, inflate, hit_mask == nullptr, lds);
  if (threadIdx.x == 0) {
    valid[t] = mask == 0u ? 1 : 0;
    if (hit_mask) hit_mask[t] = mask;
  }
}

// One block per grow index g.  Every lane forms the same candidate of attempt a (uniform arithmetic on uniform values); the block tests
// it; the first valid attempt is the result.  With cand_pose / cand_valid every attempt runs and is reported.  At most 16 attempts.
__global__ __launch_bounds__(kThreads) void object_propose_kernel(const ccmp::object_boxes B, const ccmp::object_sphere S, const ccmp::object_draw D,
                                                                  const double *__restrict__ tri, int M, unsigned long long plane, int n_boxes,
                                                                  const double *__restrict__ from_poses, const double *__restrict__ to_poses,
                                                                  double *__restrict__ pose_out, int32_t *__restrict__ which, double *__restrict__ cand_pose,
                                                                  uint8_t *__restrict__ cand_valid)
{
  __shared__ unsigned int lds[2];
  const size_t g = blockIdx.x;
  const bool report = cand_pose != nullptr || cand_valid != nullptr;
  double from[8], to[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    from[i] = from_poses[g * 8 + i];
    to[i] = to_poses[g * (size_t)D.to_stride + i];
  }
  int chosen = -1;
  for (int a = 0; a < D.attempts; a++) {
    double cand[8], R[9], p[3];
    ccmp::object_candidate(from, to, D, (uint64_t)g, a, cand);
    bool ok = ccmp::object_frame(cand, R, p);
    if (ok) {
      const uint32_t live = ccmp::object_live_boxes(cand, R, p, S, B, n_boxes, D.inflate, true);
      ok = block_hit_mask(tri, M, (size_t)plane, R, p, B, n_boxes, live, D.inflate, true, lds) == 0u;
    }
    if (threadIdx.x == 0) {
      const size_t c = g * (size_t)D.attempts + (size_t)a;
      if (cand_pose)
        for (int i = 0; i < 8; i++) cand_pose[c * 8 + i] = cand[i];
      if (cand_valid) cand_valid[c] = ok ? 1 : 0;
      if (ok && chosen < 0)
        for (int i = 0; i < 8; i++) pose_out[g * 8 + i] = cand[i];
    }
    if (ok && chosen < 0) chosen = a;
    if (chosen >= 0 && !report) break;
  }
  if (threadIdx.x == 0) {
    which[g] = chosen;
    if (chosen < 0) {
      for (int i = 0; i < 7; i++) pose_out[g * 8 + i] = __builtin_nan("");
      pose_out[g * 8 + 7] = 0.0;
    }
  }
}

// [M][9] rows -> nine planes (what ccmp_object_create runs once)
__global__ __launch_bounds__(kThreads) void object_planes_kernel(const double *__restrict__ rows, int M, unsigned long long plane, double *__restrict__ planes)
{
  const size_t w = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (w >= (size_t)M * 9) return;
  planes[(w % 9) * plane + w / 9] = rows[w];
}

}  // namespace

namespace ccmp_launch {

hipError_t object_planes(const double *rows, int M, size_t plane, double *planes, hipStream_t st)
{
  hipLaunchKernelGGL(object_planes_kernel, dim3((unsigned int)(((size_t)M * 9 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, rows, M, (unsigned long long)plane, planes);
  return hipGetLastError();
}

hipError_t object_valid(const ObjectCall &c, const double *poses, size_t T, double inflate, uint8_t *valid, uint32_t *hit_mask, hipStream_t st)
{
  hipLaunchKernelGGL(object_valid_kernel, dim3((unsigned int)T), dim3(kThreads), 0, st, *c.boxes, *c.sphere, c.tri, c.M, (unsigned long long)c.plane, c.n_boxes, poses,
                     inflate, valid, hit_mask);
  return hipGetLastError();
}

hipError_t object_propose(const ObjectCall &c, const ccmp::object_draw &D, const double *from_poses, const double *to_poses, size_t G, double *pose_out,
                          int32_t *which, double *cand_pose, uint8_t *cand_valid, hipStream_t st)
{
  hipLaunchKernelGGL(object_propose_kernel, dim3((unsigned int)G), dim3(kThreads), 0, st, *c.boxes, *c.sphere, D, c.tri, c.M, (unsigned long long)c.plane, c.n_boxes,
                     from_poses, to_poses, pose_out, which, cand_pose, cand_valid);
  return hipGetLastError();
}

}  // namespace ccmp_launch
