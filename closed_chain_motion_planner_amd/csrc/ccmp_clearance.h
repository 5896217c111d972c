/* ccmp_clearance.h — the clearance of ONE state against a proxy scene (oracle/ccmp_oracle.c: orc_clearance), computed by NT
 * cooperating threads: the extend step's 128-thread block (ccmp_kernels_geo_scene.hip: geodesic_scene_kernel) or one 16-lane row
 * of a wavefront (ccmp_kernels_fast.hip: geodesic_row16_scene_kernel).  (clearance_state_kernel, which also reports the pair,
 * keeps its own body.)  Canonical rounding model (-ffp-contract=off -DCCMP_USE_FMA): the same operations on the same
 * operands as the oracle, hence its bits whatever NT is (the minimum of a set of doubles is exact).
 *   1  threads 0..13: the rotation of joint `tid` (its sine and cosine, then ccmp_kin.h: rot_sc — joint_step's own operations);
 *   2  threads 0..5: row tid % 3 of the chain of arm tid / 3 — joint_step's origin update and product on those rotations, and
 *      the hand frame's, are row by row: row r of a frame needs only row r of the one before — keeping the arm's eight frames
 *      (bodies 0..6 after each joint, the hand) in LDS;
 *   3  thread s (s = tid, tid + NT, ...): world centre of sphere s = t_wb (o + R c) from its frame;
 *   4  thread t takes the tested pairs t, t + NT, ... and keeps the smallest signed distance; the minimum is reduced over the
 *      NT threads and every thread returns it (NaN if a joint value is not finite, as the oracle).
 * The including scope provides rot_sc, mulvec_acc, mulTvec, dot3, dot3acc, ccmp_sincos, ccmp_sqrt, ccmp_abs and shfl_f64;
 * everything here sits in the including unit's anonymous namespace. */
#ifndef CCMP_CLEARANCE_H
#define CCMP_CLEARANCE_H
#include "ccmp_scene.h"

namespace {

// LDS a caller provides, in doubles: the arms' frames (2 x 8 x (R, o)), the centres (the joints' rotations share their space:
// they are dead once the frames exist) and, for NT > 64, one partial minimum per wavefront
constexpr int kClrFrames = 2 * 8 * 12, kClrCentres = CCMP_MAX_SPHERES * 3;

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
    const int arm = tid >= 7 ? 1 : 0, i = tid - 7 * arm;
    double s, c;
    ccmp_sincos(x[tid], &s, &c);
    rot_sc(K.axis[arm][i], K.aprod[arm][i], s, c, rj + 9 * tid);
  }
  clearance_sync<NT>();
  if (tid < 6) { // PandaModel's chain (ccmp_kin.h: joint_step, the general form), the frames of orc_proxy_centres
    const int arm = tid >= 3 ? 1 : 0, r = tid - 3 * arm;
    double R[3] = {r == 0 ? 1.0 : 0.0, r == 1 ? 1.0 : 0.0, r == 2 ? 1.0 : 0.0}, o = 0.0; // row r of R, component r of o
    for (int i = 0; i < 7; i++) {
      const double *Rj = rj + 9 * (arm * 7 + i), *off = K.offset[arm][i];
      o = dot3acc(o, R[0], off[0], R[1], off[1], R[2], off[2]); // mulvec_acc(R, offset, o)
      double Rn[3];
#pragma unroll
      for (int j = 0; j < 3; j++) Rn[j] = dot3(R[0], Rj[j], R[1], Rj[3 + j], R[2], Rj[6 + j]); // mul33(R, Rj, Rn)
      R[0] = Rn[0]; R[1] = Rn[1]; R[2] = Rn[2];
      double *f = fr + (arm * 8 + i) * 12;
      f[3 * r] = R[0]; f[3 * r + 1] = R[1]; f[3 * r + 2] = R[2];
      f[9 + r] = o;
    }
    const double *ee = K.ee[arm], *Rt = K.R_tool[arm]; // hand frame: getTranslation / getRotation
    double *f = fr + (arm * 8 + 7) * 12;
    f[9 + r] = dot3acc(o, R[0], ee[0], R[1], ee[1], R[2], ee[2]);
#pragma unroll
    for (int j = 0; j < 3; j++) f[3 * r + j] = dot3(R[0], Rt[j], R[1], Rt[3 + j], R[2], Rt[6 + j]);
  }
  clearance_sync<NT>();
  const int ns = S->n_spheres, np = S->n_pairs;
  for (int s = tid; s < ns; s += NT) {
    const int slot = S->slot[s];
    const double c[3] = {S->c[s][0], S->c[s][1], S->c[s][2]};
    double wv[3];
    if (slot == ccmp::kSceneSlots - 1) { // world frame
      wv[0] = c[0]; wv[1] = c[1]; wv[2] = c[2];
    } else {
      const int arm = slot >= 9 ? 1 : 0, k = slot - 9 * arm;
      double v[3];
      if (k == 8) { // the arm's base: only t_wb applies
        v[0] = c[0]; v[1] = c[1]; v[2] = c[2];
      } else {
        const double *f = fr + (arm * 8 + k) * 12;
        v[0] = f[9]; v[1] = f[10]; v[2] = f[11];
        mulvec_acc(f, c, v);
      }
      wv[0] = K.base_p[arm][0]; wv[1] = K.base_p[arm][1]; wv[2] = K.base_p[arm][2];
      mulvec_acc(K.base_R[arm], v, wv);
    }
    cen[3 * s] = wv[0]; cen[3 * s + 1] = wv[1]; cen[3 * s + 2] = wv[2];
  }
  clearance_sync<NT>();
  double best = __builtin_inf();
  for (int p = tid; p < np; p += NT) {
    const unsigned ij = S->pair_ij[p];
    const int i = (int)(ij & 0xffu), j = (int)(ij >> 8);
    const double a0 = cen[3 * i], a1 = cen[3 * i + 1], a2 = cen[3 * i + 2];
    double d2;
    if (j < CCMP_MAX_SPHERES) {
      const double d0 = a0 - cen[3 * j], d1 = a1 - cen[3 * j + 1], dz = a2 - cen[3 * j + 2];
      d2 = dot3(d0, d0, d1, d1, dz, dz);
    } else {
      const int b = j - CCMP_MAX_SPHERES;
      const double d[3] = {a0 - S->box_c[b][0], a1 - S->box_c[b][1], a2 - S->box_c[b][2]};
      double l[3], e[3];
      mulTvec(S->box_R[b], d, l); // into the box's axes
#pragma unroll
      for (int k = 0; k < 3; k++) {
        const double a = ccmp_abs(l[k]) - S->box_half[b][k];
        e[k] = a > 0.0 ? a : 0.0;
      }
      d2 = dot3(e[0], e[0], e[1], e[1], e[2], e[2]);
    }
    const double clr = ccmp_sqrt(d2) - S->pair_rsum[p];
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
    if (!(x[k] - x[k] == 0.0)) finite = false;
  return finite ? best : __builtin_nan("");
}

} // namespace
#endif /* CCMP_CLEARANCE_H */
