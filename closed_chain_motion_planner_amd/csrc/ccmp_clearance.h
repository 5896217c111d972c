/* ccmp_clearance.h — the clearance of ONE state against a proxy scene (oracle/ccmp_oracle.c: orc_clearance), computed by NT
 * cooperating threads: the extend step's 128-thread block (ccmp_kernels_geo_scene.hip: geodesic_scene_kernel) or one 16-lane row
 * of a wavefront (ccmp_kernels_fast.hip: geodesic_row16_scene_kernel).  The arithmetic is ccmp_scene_math.h's, the one text every
 * form of the clearance runs; here is the work split, the barriers and the reduction:
 *   1  threads 0..13: the rotation of joint `tid` (scene_joint_rot);
 *   2  threads 0..5: row tid % 3 of the chain of arm tid / 3 (scene_chain_row), keeping the arm's eight frames in LDS;
 *   3  thread s (s = tid, tid + NT, ...): world centre of sphere s from its frame (scene_place);
 *   4  thread t takes the tested pairs t, t + NT, ... (scene_pair_clearance) and keeps the smallest signed distance; the minimum is
 *      reduced over the NT threads and every thread returns it (NaN if a joint value is not finite, as the oracle).
 * The including scope provides shfl_f64; everything here sits in the including unit's anonymous namespace. */
#ifndef CCMP_CLEARANCE_H
#define CCMP_CLEARANCE_H
#include "ccmp_scene_math.h"

namespace {

// LDS a caller provides, in doubles: the arms' frames (2 x 8 x (R, o)), the centres (the joints' rotations share their space:
// they are dead once the frames exist) and, for NT > 64, one partial minimum per wavefront
constexpr int kClrFrames = 2 * ccmp::kSceneArmFrames, kClrCentres = ccmp::kSceneCentres;

// the threads of one caller meet: a block barrier, or (a 16-lane row: one wavefront, whose LDS accesses complete in order) a
// compiler barrier only
template <int NT>
__device__ __forceinline__ void clearance_sync()
{
  if constexpr (NT > 64) __syncthreads();
  else asm volatile("" ::: "memory");
}

// x: the state's 14 joint values in LDS (unchanged until the routine returns); fr, cen, red: kClrFrames, kClrCentres and NT / 64
// doubles of LDS (red unused for NT <= 64); tid: 0..NT-1; lane: the thread's lane in its wavefront
template <int NT>
__device__ __forceinline__ double state_clearance(const ccmp_consts &K, const ccmp::scene_dev *__restrict__ S, const double *x, double *fr,
                                                  double *cen, double *red, int tid, int lane)
{
  double *const rj = cen; // [14][9]
  if (tid < 14) {
    const int arm = tid >= 7 ? 1 : 0;
    ccmp::scene_joint_rot(K, arm, tid - 7 * arm, x[tid], rj + 9 * tid);
  }
  clearance_sync<NT>();
  if (tid < 6) {
    const int arm = tid >= 3 ? 1 : 0;
    ccmp::scene_chain_row(K, arm, tid - 3 * arm, rj + 63 * arm, fr + ccmp::kSceneArmFrames * arm);
  }
  clearance_sync<NT>();
  const int ns = S->n_spheres, np = S->n_pairs;
  for (int s = tid; s < ns; s += NT) {
    const int slot = S->slot[s];
    const double c[3] = {S->c[s][0], S->c[s][1], S->c[s][2]};
    double wv[3];
    ccmp::scene_place(K, slot, c, fr + ccmp::kSceneArmFrames * ccmp::scene_slot_arm(slot), wv);
    cen[3 * s] = wv[0]; cen[3 * s + 1] = wv[1]; cen[3 * s + 2] = wv[2];
  }
  clearance_sync<NT>();
  double best = __builtin_inf();
  for (int p = tid; p < np; p += NT) {
    const double clr = ccmp::scene_pair_clearance(S, cen, p);
    if (clr < best) best = clr;
  }
#pragma unroll
  for (int m = (NT < 64 ? NT : 64) / 2; m >= 1; m >>= 1) { // minimum over the row / wavefront
    const double v = shfl_f64(best, lane ^ m);
    if (v < best) best = v;
  }
  if constexpr (NT > 64) {
    if (lane == 0) red[tid >> 6] = best;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NT / 64; k++) {
      const double v = red[k];
      if (v < best) best = v;
    }
  }
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 14; k++)
    if (!ccmp::scene_finite(x[k])) finite = false;
  return finite ? best : __builtin_nan("");
}

} // namespace
#endif /* CCMP_CLEARANCE_H */
