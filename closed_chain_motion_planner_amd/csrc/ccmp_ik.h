/* ccmp_ik.h — pose-targeted inverse kinematics of one arm, and the rule around it that growTree's sampleCalibGoal applies, one text for
 * host and device in the rounding model of ccmp_detmath.h (compiled with -ffp-contract=off -DCCMP_USE_FMA: only the FMAs written here
 * exist).  ccmp_pose_ik_ref runs it on the host, ik_solve_kernel / ik_select_kernel (ccmp_kernels_ik.hip) on the device: the same bits.
 *
 * The reference (jy_ConstrainedValidStateSampler.h:147-189, ik_task.cpp:16-28, panda_tracik.cpp:62-78): per arm a the hand target is
 * T_w7 = T_obj * t_o7[a]; TRAC-IK solves from the neighbour's seven joints, and where that fails from 14 Gaussian configurations around
 * mid-range (sigma 0.3, clamped to the limits), of which the converged one closest to the seed is kept; both arms must succeed; the first
 * neighbour that succeeds wins (stefanBiPRM.cpp:294-302).  TRAC-IK itself (KDL + NLopt, two racing threads, a time limit) is not
 * reproducible and is NOT restated: where the reference calls CartToJnt stands a damped-least-squares Newton solver of this project's
 * own, on the projector's forward kinematics (ccmp_kin.h).  What is restated is the rule around it.
 *
 * The solver, for one arm and one start configuration q (clamped into [lb + joint_eps, ub - joint_eps] = K.lbe / K.ube):
 *   target   R_t = R_obj * t_o7_R[a], p_t = p_obj + R_obj * t_o7_p[a]; R_obj from the pose's quaternion by Eigen's toRotationMatrix
 *            arithmetic, not normalised (utils.h:22)
 *   error    six components in the world frame: p_t - p, and the rotation vector of R_e = R_t R^T: v = 1/2 (R_e32 - R_e23, R_e13 - R_e31,
 *            R_e21 - R_e12), n = |v|, c = 1/2 (tr R_e - 1), theta = atan2(n, c) on ccmp_atan (pi - atan(n / -c) for c < 0), e_rot =
 *            v * (theta / n), and v itself when n = 0
 *   test     converged: all six |e_i| < eps, strictly; tested before every step and after the last
 *   step     e clamped in norm to err_clamp; taken into the arm's base frame (e_b = t_wb.linear()^T e, an orthogonal change that
 *            leaves the damped solution the same); dq = J^T (J J^T + lambda^2 I)^-1 e_b with the geometric Jacobian of the chain walk
 *            in that frame — column i = (a_i x (p_hand - o_i), a_i), a_i = R_i axis_i — and an unrolled 6x6 LDL^T; q += dq, clamped as
 *            above.  J is never stored: one walk accumulates J J^T column by column, a second forms J^T y from the kept sines and
 *            cosines.
 *   bound    at most max_rounds steps.
 * Candidates of (target t, seed slot s, arm a): candidate 0 starts from the slot's seven seed joints; candidate r = 1..R from
 * ambient_gaussian(K, rng_seed, ((first_index + t) S + s) R + (r - 1), 7 a + i, (lb_i + ub_i) / 2, sigma).  The arm takes candidate 0 if it
 * converged, else the converged restart with the smallest squared joint distance to the UNCLAMPED seed (an FMA chain in joint order;
 * ties to the lowest r), else it fails.  A slot succeeds if both arms do; a slot whose seed has a non-finite entry (any of the 14) is
 * skipped; the target's result is the first successful slot in the order given; otherwise a NaN row, ok = 0, which = -1.  A total
 * order over candidates: no launch shape can change the result. */
#ifndef CCMP_IK_H
#define CCMP_IK_H
#include "ccmp_kin.h"

namespace ccmp {

/* t_o7 of both arms (ccmp_problem::t_o7_R / t_o7_p): a kernel argument of the IK kernels alone — ccmp_consts is the kernarg of every hot kernel */
struct ik_arms {
  double R[2][9];
  double p[2][3];
};
/* ccmp_ik_opts as the kernels take it */
struct ik_params {
  double eps, lambda2 /* lambda * lambda */, err_clamp, sigma;
  int32_t restarts, max_rounds;
};

constexpr int kIkNotConverged = -1, kIkSkipped = -2; /* a record's `rounds` */

CCMP_HD bool ik_finite(double x) { return ccmp_abs(x) <= 1.7976931348623157e308; } /* false on NaN */
CCMP_HD double ik_clamp(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

/* Eigen Quaternion::toRotationMatrix on (x, y, z, w), no normalisation */
CCMP_HD void ik_quat_to_R(const double *q, double *R)
{
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
  R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

/* the hand target of an arm, T_obj * t_o7: pose[8] (x y z qx qy qz qw pad) -> Rt (9), pt (3) */
CCMP_HD void ik_target(const double *pose, const double *toR, const double *top, double *Rt, double *pt)
{
  double Ro[9];
  ik_quat_to_R(pose + 3, Ro);
  mul33(Ro, toR, Rt);
  pt[0] = pose[0]; pt[1] = pose[1]; pt[2] = pose[2];
  mulvec_acc(Ro, top, pt);
}

#define CCMP_IK_JOINTS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6)
/* On the device the scheduler may not move instructions across this point.  It stands between the joints of the two walks of a step:
 * their columns are independent, and interleaved for latency they hold all their temporaries at once — 256 registers and 36 bytes of
 * scratch instead of 190 and none at two wavefronts per SIMD.  No effect on any value. */
#if defined(__HIP_DEVICE_COMPILE__)
#define CCMP_IK_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define CCMP_IK_FENCE()
#endif

/* forward kinematics from kept sines and cosines: world pose of the hand frame (Rw, pw) and the hand point in the arm's base frame (ph) */
template <bool STOCK>
CCMP_HD void ik_fk(const ccmp_consts &K, int arm, const double *s, const double *c, double *Rw, double *pw, double *ph)
{
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rn[9], o[3] = {0, 0, 0};
#define CCMP_IK_STEP(I)                                                                          \
  chain_step<I, STOCK>(K.offset[arm][I], K.axis[arm][I], K.aprod[arm][I], s[I], c[I], R, Rn, o); \
  _Pragma("unroll") for (int k = 0; k < 9; k++) R[k] = Rn[k];
  CCMP_IK_JOINTS(CCMP_IK_STEP)
#undef CCMP_IK_STEP
  tool_pose_t<STOCK>(K, arm, R, o, Rw, pw);
  ph[0] = o[0]; ph[1] = o[1]; ph[2] = o[2];
  mulvec_acc_nz<STOCK ? kStockEe : 7>(R, K.ee[arm], ph);
}

/* the six error components in the world frame */
CCMP_HD void ik_error(const double *Rt, const double *pt, const double *Rw, const double *pw, double *e)
{
  const double pi = 3.14159265358979323846;
  e[0] = pt[0] - pw[0]; e[1] = pt[1] - pw[1]; e[2] = pt[2] - pw[2];
  double Re[9]; /* Rt * Rw^T */
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) Re[3 * i + j] = dot3(Rt[3 * i], Rw[3 * j], Rt[3 * i + 1], Rw[3 * j + 1], Rt[3 * i + 2], Rw[3 * j + 2]);
  const double v0 = 0.5 * (Re[7] - Re[5]), v1 = 0.5 * (Re[2] - Re[6]), v2 = 0.5 * (Re[3] - Re[1]);
  const double n = ccmp_sqrt(dot3(v0, v0, v1, v1, v2, v2));
  const double c = 0.5 * (((Re[0] + Re[4]) + Re[8]) - 1.0);
  double k = 1.0;
  if (n > 0.0) {
    const double theta = c < 0.0 ? pi - ccmp_atan2_nn(n, -c) : ccmp_atan2_nn(n, c);
    k = ccmp_div_lean(theta, n);
  }
  e[3] = v0 * k; e[4] = v1 * k; e[5] = v2 * k;
}

CCMP_HD bool ik_converged(const double *e, double eps)
{
  return ccmp_abs(e[0]) < eps && ccmp_abs(e[1]) < eps && ccmp_abs(e[2]) < eps && ccmp_abs(e[3]) < eps && ccmp_abs(e[4]) < eps && ccmp_abs(e[5]) < eps;
}

constexpr int ik_tri(int i, int j) { return i * (i + 1) / 2 + j; } /* lower triangle, j <= i */

/* y = A^-1 b for the symmetric positive definite A (lower triangle, 21 entries; destroyed): LDL^T, forward, diagonal, backward */
CCMP_HD void ik_solve6(double *A, const double *b, double *y)
{
  double d[6], inv[6];
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double w[6];
    double dj = A[ik_tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; k++) {
      w[k] = A[ik_tri(j, k)] * d[k];
      dj = CCMP_FMA(-w[k], A[ik_tri(j, k)], dj);
    }
    d[j] = dj;
    inv[j] = ccmp_div_lean(1.0, dj);
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double v = A[ik_tri(i, j)];
#pragma unroll
      for (int k = 0; k < j; k++) v = CCMP_FMA(-A[ik_tri(i, k)], w[k], v);
      A[ik_tri(i, j)] = v * inv[j];
    }
  }
  double z[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double v = b[i];
#pragma unroll
    for (int k = 0; k < i; k++) v = CCMP_FMA(-A[ik_tri(i, k)], z[k], v);
    z[i] = v;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double v = z[i] * inv[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) v = CCMP_FMA(-A[ik_tri(k, i)], y[k], v);
    y[i] = v;
  }
}

/* column I of the geometric Jacobian in the base frame at the walk's present (R, o): o is joint I's origin, R the frame in front of
 * its rotation; a = R axis_I (for a stock z joint the third column of R: the products with the exact 0, 0, 1 add nothing) */
template <int I, bool STOCK>
CCMP_HD void ik_column(const double *ax, const double *R, const double *o, const double *ph, double *col)
{
  double a0, a1, a2;
  if (STOCK && kStockZ[I]) { a0 = R[2]; a1 = R[5]; a2 = R[8]; }
  else {
    a0 = dot3(R[0], ax[0], R[1], ax[1], R[2], ax[2]);
    a1 = dot3(R[3], ax[0], R[4], ax[1], R[5], ax[2]);
    a2 = dot3(R[6], ax[0], R[7], ax[1], R[8], ax[2]);
  }
  const double r0 = ph[0] - o[0], r1 = ph[1] - o[1], r2 = ph[2] - o[2];
  col[0] = a1 * r2 - a2 * r1;
  col[1] = a2 * r0 - a0 * r2;
  col[2] = a0 * r1 - a1 * r0;
  col[3] = a0; col[4] = a1; col[5] = a2;
}

/* One round on q[7] against the hand target of the object pose `pose` (t_o7 of the arm: toR, top): the test, and unless it holds — and
 * `step` allows — one step.  Returns true if converged (q untouched).  The target is formed here, every round, from the twelve values it
 * depends on: twenty-four registers that need not live across the walks. */
template <bool STOCK>
CCMP_HD bool ik_round(const ccmp_consts &K, int arm, const ik_params &P, const double *pose, const double *toR, const double *top, double *q, bool step)
{
  double s[7], c[7], ph[3], e[6];
#pragma unroll
  for (int i = 0; i < 7; i++) ccmp_sincos(q[i], &s[i], &c[i]);
  {
    double Rw[9], pw[3], Rt[9], pt[3];
    ik_fk<STOCK>(K, arm, s, c, Rw, pw, ph);
    ik_target(pose, toR, top, Rt, pt);
    ik_error(Rt, pt, Rw, pw, e);
  }
  if (ik_converged(e, P.eps)) return true;
  if (!step) return false;
  /* the error clamped in norm, then in the base frame */
  double n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) n2 = CCMP_FMA(e[k], e[k], n2);
  const double n = ccmp_sqrt(n2);
  if (n > P.err_clamp) {
    const double f = ccmp_div_lean(P.err_clamp, n);
#pragma unroll
    for (int k = 0; k < 6; k++) e[k] = e[k] * f;
  }
  double eb[6];
  mulTvec(K.base_R[arm], e, eb);
  mulTvec(K.base_R[arm], e + 3, eb + 3);
  /* first walk: A = J J^T + lambda^2 I */
  double A[21];
#pragma unroll
  for (int i = 0; i < 6; i++)
#pragma unroll
    for (int j = 0; j <= i; j++) A[ik_tri(i, j)] = i == j ? P.lambda2 : 0.0;
  {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rn[9], o[3] = {0, 0, 0}, col[6];
#define CCMP_IK_STEP(I)                                                                                 \
  mulvec_acc_nz<STOCK ? kStockOff[I] : 7>(R, K.offset[arm][I], o);                                      \
  ik_column<I, STOCK>(K.axis[arm][I], R, o, ph, col);                                                   \
  _Pragma("unroll") for (int i = 0; i < 6; i++)                                                         \
    _Pragma("unroll") for (int j = 0; j <= i; j++) A[ik_tri(i, j)] = CCMP_FMA(col[i], col[j], A[ik_tri(i, j)]); \
  if (I < 6) {                                                                                          \
    chain_rot<I, STOCK>(K.axis[arm][I], K.aprod[arm][I], s[I], c[I], R, Rn);                            \
    _Pragma("unroll") for (int k = 0; k < 9; k++) R[k] = Rn[k];                                         \
  }                                                                                                     \
  CCMP_IK_FENCE();
    CCMP_IK_JOINTS(CCMP_IK_STEP)
#undef CCMP_IK_STEP
  }
  double y[6];
  ik_solve6(A, eb, y);
  /* second walk: dq_i = column i . y, then the step and the clamp */
  {
    double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rn[9], o[3] = {0, 0, 0}, col[6];
#define CCMP_IK_STEP(I)                                                                                 \
  mulvec_acc_nz<STOCK ? kStockOff[I] : 7>(R, K.offset[arm][I], o);                                      \
  ik_column<I, STOCK>(K.axis[arm][I], R, o, ph, col);                                                   \
  {                                                                                                     \
    double dq = 0.0;                                                                                    \
    _Pragma("unroll") for (int k = 0; k < 6; k++) dq = CCMP_FMA(col[k], y[k], dq);                      \
    q[I] = ik_clamp(q[I] + dq, K.lbe[I], K.ube[I]);                                                     \
  }                                                                                                     \
  if (I < 6) {                                                                                          \
    chain_rot<I, STOCK>(K.axis[arm][I], K.aprod[arm][I], s[I], c[I], R, Rn);                            \
    _Pragma("unroll") for (int k = 0; k < 9; k++) R[k] = Rn[k];                                         \
  }                                                                                                     \
  CCMP_IK_FENCE();
    CCMP_IK_JOINTS(CCMP_IK_STEP)
#undef CCMP_IK_STEP
  }
  return false;
}

/* Start configuration of candidate r of (target index `ts` = (first_index + t) S + s, arm) into q[7], and the squared distance
 * bookkeeping's reference, the unclamped seed.  seed7: the slot's seven joints of this arm. */
CCMP_HD void ik_start(const ccmp_consts &K, const ik_params &P, uint64_t rng_seed, uint64_t ts, int arm, int r, const double *seed7, double *q)
{
#pragma unroll
  for (int i = 0; i < 7; i++) {
    double v = seed7[i];
    if (r > 0) v = ambient_gaussian(K, rng_seed, ts * (uint64_t)P.restarts + (uint64_t)(r - 1), 7 * arm + i, 0.5 * (K.lb[i] + K.ub[i]), P.sigma);
    q[i] = ik_clamp(v, K.lbe[i], K.ube[i]);
  }
}

/* squared joint distance to the (unclamped) seed: an FMA chain in joint order */
CCMP_HD double ik_seed_d2(const double *q, const double *seed7)
{
  double d2 = 0.0;
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const double d = q[i] - seed7[i];
    d2 = CCMP_FMA(d, d, d2);
  }
  return d2;
}

/* Records of a call, candidate index c = ((t S + s) 2 + a) (1 + R) + r: q [c][7], rounds [c] (rounds taken, kIkNotConverged,
 * kIkSkipped), d2 [c].  The rule over them for target t -> q_out[14], ok, which. */
CCMP_HD void ik_select(const double *rec_q, const int32_t *rec_rounds, const double *rec_d2, size_t t, int S, int R, double *q_out, uint8_t *ok,
                       int32_t *which)
{
  for (int s = 0; s < S; s++) {
    size_t pick[2];
    bool both = true;
    for (int a = 0; a < 2; a++) {
      const size_t base = ((t * (size_t)S + (size_t)s) * 2 + (size_t)a) * (size_t)(1 + R);
      bool have = false;
      size_t best = base;
      if (rec_rounds[base] >= 0) have = true;
      else {
        for (int r = 1; r <= R; r++) {
          if (rec_rounds[base + r] < 0) continue;
          if (!have || rec_d2[base + r] < rec_d2[best]) { best = base + r; have = true; }
        }
      }
      pick[a] = best;
      both = both && have;
    }
    if (!both) continue;
    for (int a = 0; a < 2; a++)
      for (int i = 0; i < 7; i++) q_out[7 * a + i] = rec_q[pick[a] * 7 + i];
    *ok = 1;
    *which = s;
    return;
  }
  for (int i = 0; i < 14; i++) q_out[i] = __builtin_nan("");
  *ok = 0;
  *which = -1;
}

} /* namespace ccmp */
#endif /* CCMP_IK_H */
