/* ccmp_scene_math.h — the arithmetic of the proxy scene's clearance (oracle/ccmp_oracle.c: orc_clearance), ONE text for every form of it:
 * the tile and per-state kernels (ccmp_kernels_scene.hip), the extend step's state_clearance<NT> (ccmp_clearance.h), the vetted IK's
 * ik_vet_kernel (ccmp_kernels_ik_vet.hip) and the *_ref forms on the host (ccmp_ik.cpp).  Canonical rounding model (-ffp-contract=off
 * -DCCMP_USE_FMA): the same operations on the same operands as the oracle, so a caller chooses its work split — who computes which joint,
 * row, sphere or pair — and nothing else; the minimum of a set of doubles is exact, hence the oracle's bits whatever the split.
 *
 * Frames.  An arm has eight frames in its base, kSceneFrame doubles each (R row-major, then o): bodies 0..6 after each joint and the
 * hand (PandaModel::getTranslation / getRotation).  Frame slot 9 a + k is frame k of arm a, 9 a + 8 arm a's base, kSceneSlots - 1 the
 * world (ccmp_scene.h).  They come from ccmp_kin.h: joint_step, either whole (scene_arm_frames, one thread) or row by row
 * (scene_joint_rot, then scene_chain_row for r = 0, 1, 2 — row r of a frame needs only row r of the one before): the same operations,
 * tests/test_scene_math_host.py holds the two against each other byte for byte on the host. */
#ifndef CCMP_SCENE_MATH_H
#define CCMP_SCENE_MATH_H
#include "ccmp_kin.h"
#include "ccmp_scene.h"

namespace ccmp {

constexpr int kSceneFrame = 12;                    /* a frame in the arm's base: R (9, row-major), o (3) */
constexpr int kSceneArmFrames = 8 * kSceneFrame;   /* one arm: bodies 0..6 after each joint, the hand */
constexpr int kSceneCentres = CCMP_MAX_SPHERES * 3; /* world centres by stored sphere index */

CCMP_HD bool scene_finite(double x) { return x - x == 0.0; } /* the oracle's test: false on NaN and on an infinity */

/* ---- frame to world ------------------------------------------------------------------------------------------------------------------ */
/* v = o + R c: a point of the frame (R, o), in the arm's base */
CCMP_HD void scene_frame_to_base(const double *R, const double *o, const double *c, double *v)
{
  v[0] = o[0]; v[1] = o[1]; v[2] = o[2];
  mulvec_acc(R, c, v);
}
/* w = t_wb v: a point of arm `arm`'s base, in the world */
CCMP_HD void scene_base_to_world(const ccmp_consts &K, int arm, const double *v, double *w)
{
  w[0] = K.base_p[arm][0]; w[1] = K.base_p[arm][1]; w[2] = K.base_p[arm][2];
  mulvec_acc(K.base_R[arm], v, w);
}
/* world centre of a sphere on frame slot `slot` with centre c in that frame: t_wb (o + R c); f = that slot's own frame (not read for a
 * base or the world) */
CCMP_HD void scene_place_on(const ccmp_consts &K, int slot, const double *c, const double *f, double *w)
{
  if (slot == kSceneSlots - 1) { /* world frame */
    w[0] = c[0]; w[1] = c[1]; w[2] = c[2];
    return;
  }
  const int arm = scene_slot_arm(slot);
  double v[3];
  if (slot - 9 * arm == 8) { /* the arm's base: only t_wb applies */
    v[0] = c[0]; v[1] = c[1]; v[2] = c[2];
  } else {
    scene_frame_to_base(f, f + 9, c, v);
  }
  scene_base_to_world(K, arm, v, w);
}
/* the same for a caller that holds the eight frames fr of the sphere's arm (both arms' frames: fr + kSceneArmFrames * scene_slot_arm(slot));
 * a base or the world reads none, so any frame in range stands for theirs */
CCMP_HD void scene_place(const ccmp_consts &K, int slot, const double *c, const double *fr, double *w)
{
  scene_place_on(K, slot, c, fr + kSceneFrame * ((slot - 9 * scene_slot_arm(slot)) & 7), w);
}

/* ---- distances ----------------------------------------------------------------------------------------------------------------------- */
/* squared distance of the point (a[0], a[stride], a[2 stride]) to box b (0 inside).  The point comes as its place in the caller's centre
 * array, whatever its layout ([sphere][3], or the tile kernel's [sphere][component][lane]), and is read here beside the box's own data:
 * handed over as three values, the tile kernel's loads move and its instruction stream is no longer the one that was measured. */
CCMP_HD double scene_box_d2(const scene_dev *S, int b, const double *a, int stride)
{
  const double d[3] = {a[0] - S->box_c[b][0], a[stride] - S->box_c[b][1], a[2 * stride] - S->box_c[b][2]};
  double l[3], e[3];
  mulTvec(S->box_R[b], d, l); /* into the box's axes */
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double a = ccmp_abs(l[k]) - S->box_half[b][k];
    e[k] = a > 0.0 ? a : 0.0;
  }
  return dot3(e[0], e[0], e[1], e[1], e[2], e[2]);
}
/* signed distance of tested pair p of the scene's table; cen = world centres by stored sphere index, [sphere][3] */
CCMP_HD double scene_pair_clearance(const scene_dev *S, const double *cen, int p)
{
  const unsigned ij = S->pair_ij[p];
  const int i = (int)(ij & 0xffu), j = (int)(ij >> 8);
  const double *a = cen + 3 * i;
  double d2;
  if (j < CCMP_MAX_SPHERES) {
    const double d0 = a[0] - cen[3 * j], d1 = a[1] - cen[3 * j + 1], dz = a[2] - cen[3 * j + 2];
    d2 = dot3(d0, d0, d1, d1, dz, dz);
  } else {
    d2 = scene_box_d2(S, j - CCMP_MAX_SPHERES, a, 1);
  }
  return ccmp_sqrt(d2) - S->pair_rsum[p];
}

/* ---- the chain, row by row (state_clearance<NT>, ik_vet_kernel: one thread per joint, then one per row) -------------------------------- */
/* the rotation of joint i of arm `arm` at angle x: its sine and cosine, then rot_sc — joint_step's own operations */
CCMP_HD void scene_joint_rot(const ccmp_consts &K, int arm, int i, double x, double *rj9)
{
  double s, c;
  ccmp_sincos(x, &s, &c);
  rot_sc(K.axis[arm][i], K.aprod[arm][i], s, c, rj9);
}
/* row r of the arm's eight frames from its joints' rotations rj [7][9]: joint_step's origin update and product, and the hand frame's,
 * on row r of R and component r of o */
CCMP_HD void scene_chain_row(const ccmp_consts &K, int arm, int r, const double *rj, double *fr)
{
  double R[3] = {r == 0 ? 1.0 : 0.0, r == 1 ? 1.0 : 0.0, r == 2 ? 1.0 : 0.0}, o = 0.0;
  for (int i = 0; i < 7; i++) {
    const double *Rj = rj + 9 * i, *off = K.offset[arm][i];
    o = dot3acc(o, R[0], off[0], R[1], off[1], R[2], off[2]); /* mulvec_acc(R, offset, o) */
    double Rn[3];
#pragma unroll
    for (int j = 0; j < 3; j++) Rn[j] = dot3(R[0], Rj[j], R[1], Rj[3 + j], R[2], Rj[6 + j]); /* mul33(R, Rj, Rn) */
    R[0] = Rn[0]; R[1] = Rn[1]; R[2] = Rn[2];
    double *f = fr + i * kSceneFrame;
    f[3 * r] = R[0]; f[3 * r + 1] = R[1]; f[3 * r + 2] = R[2];
    f[9 + r] = o;
  }
  const double *ee = K.ee[arm], *Rt = K.R_tool[arm]; /* hand frame: getTranslation / getRotation */
  double *f = fr + 7 * kSceneFrame;
  f[9 + r] = dot3acc(o, R[0], ee[0], R[1], ee[1], R[2], ee[2]);
#pragma unroll
  for (int j = 0; j < 3; j++) f[3 * r + j] = dot3(R[0], Rt[j], R[1], Rt[3 + j], R[2], Rt[6 + j]);
}

/* ---- one thread walks it all (the *_ref entry points) ---------------------------------------------------------------------------------- */
/* PandaModel's chain of one arm (ccmp_kin.h: joint_step, the general form) and the hand frame */
inline void scene_arm_frames(const ccmp_consts &K, int arm, const double *q7, double *fr)
{
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
  for (int i = 0; i < 7; i++) {
    double s, c;
    ccmp_sincos(q7[i], &s, &c);
    joint_step(K, arm, i, s, c, R, o);
    for (int k = 0; k < 9; k++) fr[i * kSceneFrame + k] = R[k];
    for (int k = 0; k < 3; k++) fr[i * kSceneFrame + 9 + k] = o[k];
  }
  double *f = fr + 7 * kSceneFrame;
  f[9] = o[0]; f[10] = o[1]; f[11] = o[2];
  mulvec_acc(R, K.ee[arm], f + 9);
  mul33(R, K.R_tool[arm], f);
}

/* the clearance of ONE arm (ccmp_ik_vet.h): the smallest signed distance over arm `arm`'s pair list, +inf for an empty one */
inline double scene_arm_clearance(const ccmp_consts &K, const scene_dev &S, const scene_arm_dev &A, int arm, const double *q7)
{
  for (int i = 0; i < 7; i++)
    if (!scene_finite(q7[i])) return __builtin_nan("");
  double fr[kSceneArmFrames], cen[kSceneCentres];
  scene_arm_frames(K, arm, q7, fr);
  for (int s = 0; s < S.n_spheres; s++) {
    const int m = scene_moving_arm(S.slot[s]);
    if (m >= 0 && m != arm) continue; /* moving on the other arm: in none of this arm's pairs */
    scene_place(K, S.slot[s], S.c[s], fr, cen + 3 * s);
  }
  double best = __builtin_inf();
  for (int n = 0; n < A.n_pairs[arm]; n++) {
    const double clr = scene_pair_clearance(&S, cen, A.pair[arm][n]);
    if (clr < best) best = clr;
  }
  return best;
}

/* ccmp_clearance of a 14-joint state (oracle/ccmp_oracle.c: orc_clearance) */
inline double scene_state_clearance(const ccmp_consts &K, const scene_dev &S, const double *x)
{
  for (int i = 0; i < 14; i++)
    if (!scene_finite(x[i])) return __builtin_nan("");
  double fr[2 * kSceneArmFrames], cen[kSceneCentres];
  scene_arm_frames(K, 0, x, fr);
  scene_arm_frames(K, 1, x + 7, fr + kSceneArmFrames);
  for (int s = 0; s < S.n_spheres; s++) scene_place(K, S.slot[s], S.c[s], fr + kSceneArmFrames * scene_slot_arm(S.slot[s]), cen + 3 * s);
  double best = __builtin_inf();
  for (int p = 0; p < S.n_pairs; p++) {
    const double clr = scene_pair_clearance(&S, cen, p);
    if (clr < best) best = clr;
  }
  return best;
}

}  /* namespace ccmp */
#endif /* CCMP_SCENE_MATH_H */
