/* ccmp_object.h — the head of growTree: which object pose to grow to, and whether the object's mesh is free of the static workspace there.
 * One text for host and device in the rounding model of ccmp_detmath.h (compiled with -ffp-contract=off -DCCMP_USE_FMA: only the FMAs
 * written here exist).  ccmp_object_*_ref runs it on the host, object_valid_kernel / object_propose_kernel (ccmp_kernels_object.hip) on
 * the device: the same bits.
 *
 * The reference (stefanBiPRM.cpp:255-276, :733-752; stefanFCL.h:115-138): growTree interpolates the object pose 30 % from the nearest
 * vertex towards the goal, draws an SE(3) Gaussian sample around it (sigma 0.2, two attempts), asks stefan_checker_->isValid and only
 * then grows; checkForSolution walks nine interpolated poses 0.1 i towards the goal and stops at the first one refused; isFeasible tests
 * the object's triangle mesh, moved by the pose, against six static boxes and answers "no" at the first that collides.
 *
 * RESTATED from OMPL's published definitions (ompl/base/spaces/src/SO3StateSpace.cpp, RealVectorStateSpace.cpp, SE3StateSpace.cpp, BSD):
 *   SE3StateSpace::interpolate       position a + (b - a) t; rotation SO3StateSpace::interpolate: theta = arcLength(a, b); theta >
 *                                    DBL_EPSILON: d = 1 / sin(theta), s0 = sin((1 - t) theta), s1 = sin(t theta), s1 negated when the
 *                                    plain dot product of the quaternions is < 0, q = (qa s0 + qb s1) d; else q = qa.  No normalisation.
 *   CompoundStateSampler::sampleGaussian with SE3's weights: RealVectorStateSampler::sampleGaussian (mean + sigma N(0,1), clamped into
 *                                    the bounds) and SO3StateSampler::sampleGaussian (rotDev = 2 sigma / sqrt(3); (x, y, z) = rotDev N(0,1)^3,
 *                                    theta = |(x, y, z)|; theta < DBL_EPSILON: the mean; else q = q_mean (x) (s x, s y, s z, c) with
 *                                    s = sin(theta / 2) / theta, c = cos(theta / 2), by quaternionProduct).
 * NOT RESTATED: OMPL's random numbers — the deviates are Box-Muller on two counter-based uniforms exactly as ccmp::ambient_gaussian forms
 * them, counters seed ^ (index 12 + 2 j) and seed ^ (index 12 + 2 j + 1), j = 0..5; OMPL's uniform fall-back for a wide rotation (the
 * entry points refuse rotDev > 1.44 instead); FCL's BVH and GJK — the mesh test is an exact triangle-against-oriented-box
 * separating-axis test of this project's own.  It answers the same geometric question and is not comparable with FCL beyond that.
 *
 * Term orders (every sum is an FMA chain, left to right as listed, starting from the first product or the stated addend):
 *   world vertex      w_i = fma(R_i2, v_2, fma(R_i1, v_1, fma(R_i0, v_0, p_i))); R from the pose's quaternion by ik_quat_to_R (Eigen's
 *                     toRotationMatrix, not normalised: utils.h:22)
 *   box frame         d = w - c (plain), u_i = fma(R_2i, d_2, fma(R_1i, d_1, R_0i d_0))                         (R^T d)
 *   edges             e0 = u1 - u0, e1 = u2 - u1, e2 = u0 - u2 (plain)
 *   normal            n = e0 x e1, each component a b - c d as fma(a, b, -(c d)); projection fma(n_2, u0_2, fma(n_1, u0_1, n_0 u0_0)); radius
 *                     fma(h_2, |n_2|, fma(h_1, |n_1|, h_0 |n_0|))
 *   cross axes        box axis i x edge j: for i = 0: (0, -e_z, e_y), i = 1: (e_z, 0, -e_x), i = 2: (-e_y, e_x, 0); projection of vertex k
 *                     fma(a_q, u_kq, a_p u_kp) over the two non-zero components p < q; radius fma(h_q, |a_q|, h_p |a_p|)
 *   Gaussian rotation theta^2 = fma(z, z, fma(y, y, x x)); quaternion product: x = fma(-mz, qy, fma(my, qz, fma(mx, qw, mw qx))),
 *                     y = fma(-mx, qz, fma(mz, qx, fma(my, qw, mw qy))), z = fma(-my, qx, fma(mx, qy, fma(mz, qw, mw qz))),
 *                     w = fma(-mz, qz, fma(-my, qy, fma(-mx, qx, mw qw)))   (m the mean, q the perturbation: OMPL's operand order)
 * The separating-axis test uses unnormalised axes, no division and no square root; triangle and box are separated only by a strict >:
 * touching is a hit.  A null axis (a degenerate triangle) has projection 0 and radius 0, and 0 > 0 is false: it never separates.
 *
 * Broad phase: the mesh's bounding sphere (centre: the middle of the vertices' bounding box; radius: the largest distance to a vertex,
 * times 1 + 1e-6, plus 1e-9 (1 + largest |coordinate|)), moved by the pose — its radius times |1 - |q|^2| + |q|^2, the largest stretch of
 * the unnormalised rotation matrix, plus 1e-9 (1 + |p|_1 + |c_box|_1 + |h_box|_1 + |inflate|) for the rounding of the narrow phase's own
 * coordinates.  A box whose squared distance to the moved centre exceeds the squared radius cannot be reached by any vertex and is
 * skipped for the whole pose.  The slack is six and more orders of magnitude above any rounding in these sums: the broad phase never
 * changes an answer (tests hold it to that with the flag of ccmp_object_valid_ref). */
#ifndef CCMP_OBJECT_H
#define CCMP_OBJECT_H
#include "ccmp_ik.h"
#include "ccmp_pose.h"

namespace ccmp {

constexpr int kObjectMaxBoxes = 8;
constexpr double kObjectEps = 2.220446049250313e-16; /* DBL_EPSILON */
constexpr double kObjectRotDevMax = 1.44;            /* the entry points refuse a sigma beyond it */

/* one workspace box as the kernels take it: 136 bytes */
struct object_box {
  double c[3];
  double R[9]; /* row-major, box axes -> world */
  double h[3];
  double mag;  /* |c|_1 + |h|_1: scale of the broad phase's absolute slack */
  double reserved;
};
/* the kernel argument of the object kernels alone (ccmp_consts is not touched) */
struct object_boxes {
  object_box b[kObjectMaxBoxes];
};
/* the mesh's bounding sphere in the object frame, radius with its slack */
struct object_sphere {
  double c[3];
  double r;
};
/* what a propose call hands the kernel besides the poses */
struct object_draw {
  double t, sigma, lo[3], hi[3], inflate;
  unsigned long long rng_seed, first_index;
  int32_t attempts, to_stride;
};

CCMP_HD double object_rot_dev(double sigma) { return ccmp_div_lean(2.0 * sigma, 1.7320508075688772); }

/* SE3StateSpace::interpolate on pose rows */
CCMP_HD void pose_interpolate(const double *a, const double *b, double t, double *out)
{
#pragma unroll
  for (int i = 0; i < 3; i++) out[i] = CCMP_FMA(b[i] - a[i], t, a[i]);
  const double theta = ccmp_pose_rot(a[3], a[4], a[5], a[6], b[3], b[4], b[5], b[6]);
  if (theta > kObjectEps) {
    double st, ct, s0, s1, c_;
    ccmp_sincos(theta, &st, &ct);
    const double d = ccmp_div_lean(1.0, st);
    ccmp_sincos((1.0 - t) * theta, &s0, &c_);
    ccmp_sincos(t * theta, &s1, &c_);
    const double dq = a[3] * b[3] + a[4] * b[4] + a[5] * b[5] + a[6] * b[6];
    if (dq < 0.0) s1 = -s1;
#pragma unroll
    for (int i = 3; i < 7; i++) out[i] = (a[i] * s0 + b[i] * s1) * d;
  } else {
#pragma unroll
    for (int i = 3; i < 7; i++) out[i] = a[i];
  }
  out[7] = 0.0;
}

/* unit deviate j of draw `index`: ambient_gaussian's Box-Muller on this stream's counters */
CCMP_HD double object_deviate(uint64_t seed, uint64_t index, int j)
{
  const uint64_t r1 = splitmix64(seed ^ (index * 12ULL + 2ULL * (uint64_t)j));
  const uint64_t r2 = splitmix64(seed ^ (index * 12ULL + 2ULL * (uint64_t)j + 1ULL));
  const double u1 = (double)((r1 >> 11) + 1ULL) * 1.1102230246251565e-16; /* (0,1] */
  const double u2 = (double)(r2 >> 11) * 1.1102230246251565e-16;          /* [0,1) */
  double s, c;
  ccmp_sincos(6.283185307179586 * u2, &s, &c);
  return ccmp_sqrt(-2.0 * ccmp_log(u1)) * c;
}

/* the compound sampleGaussian of SE3 around `mean`; sigma == 0 returns the mean (theta = 0 keeps its rotation) */
CCMP_HD void pose_gaussian(const double *mean, double sigma, const double *lo, const double *hi, uint64_t seed, uint64_t index, double *out)
{
#pragma unroll
  for (int j = 0; j < 3; j++) out[j] = ik_clamp(CCMP_FMA(object_deviate(seed, index, j), sigma, mean[j]), lo[j], hi[j]);
  const double rd = object_rot_dev(sigma);
  const double x = rd * object_deviate(seed, index, 3), y = rd * object_deviate(seed, index, 4), z = rd * object_deviate(seed, index, 5);
  const double theta = ccmp_sqrt(CCMP_FMA(z, z, CCMP_FMA(y, y, x * x)));
  const double mx = mean[3], my = mean[4], mz = mean[5], mw = mean[6];
  if (theta < kObjectEps) {
    out[3] = mx; out[4] = my; out[5] = mz; out[6] = mw;
  } else {
    double sh, c;
    ccmp_sincos(0.5 * theta, &sh, &c);
    const double s = ccmp_div_lean(sh, theta);
    const double qx = s * x, qy = s * y, qz = s * z, qw = c;
    out[3] = CCMP_FMA(-mz, qy, CCMP_FMA(my, qz, CCMP_FMA(mx, qw, mw * qx)));
    out[4] = CCMP_FMA(-mx, qz, CCMP_FMA(mz, qx, CCMP_FMA(my, qw, mw * qy)));
    out[5] = CCMP_FMA(-my, qx, CCMP_FMA(mx, qy, CCMP_FMA(mz, qw, mw * qz)));
    out[6] = CCMP_FMA(-mz, qz, CCMP_FMA(-my, qy, CCMP_FMA(-mx, qx, mw * qw)));
  }
  out[7] = 0.0;
}

/* candidate `a` of grow index g: interpolate, then draw */
CCMP_HD void object_candidate(const double *from, const double *to, const object_draw &D, uint64_t g, int a, double *out)
{
  double mid[8];
  pose_interpolate(from, to, D.t, mid);
  pose_gaussian(mid, D.sigma, D.lo, D.hi, D.rng_seed, (D.first_index + g) * (uint64_t)D.attempts + (uint64_t)a, out);
}

/* pose -> R (9), p (3); false when a component is not finite (nothing is tested then) */
CCMP_HD bool object_frame(const double *pose, double *R, double *p)
{
  bool finite = true;
#pragma unroll
  for (int i = 0; i < 7; i++) finite = finite && ik_finite(pose[i]);
  ik_quat_to_R(pose + 3, R);
  p[0] = pose[0]; p[1] = pose[1]; p[2] = pose[2];
  return finite;
}

/* R v + p */
CCMP_HD void object_to_world(const double *R, const double *p, double v0, double v1, double v2, double *w)
{
#pragma unroll
  for (int i = 0; i < 3; i++) w[i] = CCMP_FMA(R[3 * i + 2], v2, CCMP_FMA(R[3 * i + 1], v1, CCMP_FMA(R[3 * i], v0, p[i])));
}

/* the boxes a pose can reach at all: bit b set = box b goes to the narrow phase */
CCMP_HD uint32_t object_live_boxes(const double *pose, const double *R, const double *p, const object_sphere &S, const object_boxes &B, int n_boxes,
                                   double inflate, bool broad_phase)
{
  const uint32_t all = (1u << n_boxes) - 1u;
  if (!broad_phase) return all;
  double c[3];
  object_to_world(R, p, S.c[0], S.c[1], S.c[2], c);
  const double n2 = CCMP_FMA(pose[6], pose[6], CCMP_FMA(pose[5], pose[5], CCMP_FMA(pose[4], pose[4], pose[3] * pose[3])));
  const double stretch = ccmp_abs(1.0 - n2) + n2;
  const double pmag = (ccmp_abs(p[0]) + ccmp_abs(p[1])) + (ccmp_abs(p[2]) + ccmp_abs(inflate));
  uint32_t live = 0;
  for (int b = 0; b < n_boxes; b++) {
    const object_box &X = B.b[b];
    const double rad = CCMP_FMA(S.r, stretch, 1e-9 * ((1.0 + pmag) + X.mag));
    const double d0 = c[0] - X.c[0], d1 = c[1] - X.c[1], d2 = c[2] - X.c[2];
    double dist2 = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double u = CCMP_FMA(X.R[6 + i], d2, CCMP_FMA(X.R[3 + i], d1, X.R[i] * d0));
      const double e = ccmp_abs(u) - (X.h[i] + inflate);
      if (e > 0.0) dist2 = CCMP_FMA(e, e, dist2);
    }
    if (!(dist2 > rad * rad)) live |= 1u << b; /* NaN anywhere: the box stays */
  }
  return live;
}

CCMP_HD double object_min3(double a, double b, double c) { const double m = a < b ? a : b; return m < c ? m : c; }
CCMP_HD double object_max3(double a, double b, double c) { const double m = a > b ? a : b; return m > c ? m : c; }

/* the narrow phase: triangle (world vertices w0, w1, w2) against box X with half extents h + inflate; true unless one of the 13 axes
 * separates them strictly */
CCMP_HD bool tri_box_hit(const double *w0, const double *w1, const double *w2, const object_box &X, double inflate)
{
  double u[3][3]; /* vertex k, box axis i */
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double *w = k == 0 ? w0 : (k == 1 ? w1 : w2);
    const double d0 = w[0] - X.c[0], d1 = w[1] - X.c[1], d2 = w[2] - X.c[2];
#pragma unroll
    for (int i = 0; i < 3; i++) u[k][i] = CCMP_FMA(X.R[6 + i], d2, CCMP_FMA(X.R[3 + i], d1, X.R[i] * d0));
  }
  const double h[3] = {X.h[0] + inflate, X.h[1] + inflate, X.h[2] + inflate};
  bool sep = false;
  /* the box axes */
#pragma unroll
  for (int i = 0; i < 3; i++) sep = sep || object_min3(u[0][i], u[1][i], u[2][i]) > h[i] || object_max3(u[0][i], u[1][i], u[2][i]) < -h[i];
  double e[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    e[0][i] = u[1][i] - u[0][i];
    e[1][i] = u[2][i] - u[1][i];
    e[2][i] = u[0][i] - u[2][i];
  }
  /* the triangle's normal */
  {
    const double n0 = CCMP_FMA(e[0][1], e[1][2], -(e[0][2] * e[1][1]));
    const double n1 = CCMP_FMA(e[0][2], e[1][0], -(e[0][0] * e[1][2]));
    const double n2 = CCMP_FMA(e[0][0], e[1][1], -(e[0][1] * e[1][0]));
    const double d = CCMP_FMA(n2, u[0][2], CCMP_FMA(n1, u[0][1], n0 * u[0][0]));
    const double r = CCMP_FMA(h[2], ccmp_abs(n2), CCMP_FMA(h[1], ccmp_abs(n1), h[0] * ccmp_abs(n0)));
    sep = sep || ccmp_abs(d) > r;
  }
  /* box axis i x edge j: components p < q are the two that are not i */
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int p = i == 0 ? 1 : 0, q = i == 2 ? 1 : 2;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      /* axis_i x e: i = 0: (0, -e2, e1); i = 1: (e2, 0, -e0); i = 2: (-e1, e0, 0) */
      const double ap = i == 0 ? -e[j][2] : (i == 1 ? e[j][2] : -e[j][1]);
      const double aq = i == 0 ? e[j][1] : (i == 1 ? -e[j][0] : e[j][0]);
      const double p0 = CCMP_FMA(aq, u[0][q], ap * u[0][p]);
      const double p1 = CCMP_FMA(aq, u[1][q], ap * u[1][p]);
      const double p2 = CCMP_FMA(aq, u[2][q], ap * u[2][p]);
      const double r = CCMP_FMA(h[q], ccmp_abs(aq), h[p] * ccmp_abs(ap));
      sep = sep || object_min3(p0, p1, p2) > r || object_max3(p0, p1, p2) < -r;
    }
  }
  return !sep;
}

/* the pose rule on the host: hit mask of one pose over M triangles [M][9] in the object frame; *finite_out = the pose was tested */
CCMP_HD uint32_t object_pose_mask(const double *pose, const double *tri, int M, const object_sphere &S, const object_boxes &B, int n_boxes, double inflate,
                                  bool broad_phase, bool *finite_out)
{
  double R[9], p[3];
  *finite_out = object_frame(pose, R, p);
  if (!*finite_out) return 0u;
  const uint32_t live = object_live_boxes(pose, R, p, S, B, n_boxes, inflate, broad_phase);
  uint32_t mask = 0;
  if (live == 0u) return 0u;
  for (int m = 0; m < M; m++) {
    const double *v = tri + (size_t)m * 9;
    double w0[3], w1[3], w2[3];
    object_to_world(R, p, v[0], v[1], v[2], w0);
    object_to_world(R, p, v[3], v[4], v[5], w1);
    object_to_world(R, p, v[6], v[7], v[8], w2);
    for (int b = 0; b < n_boxes; b++)
      if (((live >> b) & 1u) && tri_box_hit(w0, w1, w2, B.b[b], inflate)) mask |= 1u << b;
  }
  return mask;
}

} /* namespace ccmp */
#endif /* CCMP_OBJECT_H */
