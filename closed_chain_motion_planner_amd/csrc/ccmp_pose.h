/* ccmp_pose.h — the object pose of a roadmap vertex and the planner's tree metric on it, one text for host and device, in the
 * rounding model of ccmp_detmath.h (compiled with -ffp-contract=off: only the FMAs written here exist).
 *
 * The reference ranks its tree on the object pose alone: stefanBiPRM.h:194-201 sets the nearest-neighbour structure's distance
 * function to obj_space_->distance(components[1], components[1]) (the joint-space line above it is commented out), and every
 * connectionStrategy_(...) call ranks on it (stefanBiPRM.cpp:292,390,457).  obj_space_ is an ompl::base::SE3StateSpace with its
 * default subspace weights 1 and 1.  OMPL is not a dependency of this project; what is restated below are its published
 * definitions (ompl/base/spaces/src/SO3StateSpace.cpp, ompl/base/src/StateSpace.cpp, BSD licence):
 *
 *   CompoundStateSpace::distance    sum over the subspaces of weight_i * subspace_i->distance(...)       — here 1 * R^3 + 1 * SO(3)
 *   RealVectorStateSpace::distance  sqrt(sum of squared differences), accumulated in component order    — x, y, z
 *   SO3StateSpace::distance         arcLength(a, b): dq = fabs(a.x*b.x + a.y*b.y + a.z*b.z + a.w*b.w);
 *                                   dq > 1.0 - MAX_QUATERNION_NORM_ERROR (1e-9) ? 0.0 : acos(dq)
 *
 * Quaternions are NOT normalised (OMPL does not either).  The accumulations are the FMA chains of orc_distance
 * (oracle/ccmp_oracle.c), the square root is ccmp_sqrt (correctly rounded) and acos(dq), 0 <= dq <= 1 - 1e-9, is
 * atan2(sqrt(1 - dq^2), dq) on ccmp_atan2_nn with 1 - dq^2 from one FMA (a single rounding).  A NaN anywhere gives NaN: every
 * comparison below is false on it and it reaches the sum.
 *
 * A pose is 8 doubles (64 bytes, 16-byte aligned rows): x y z qx qy qz qw pad.  The pad is written as 0 and never read.
 *
 * The pose of a joint state (stefanBiPRM.cpp:338, utils.h:37-46): IKTask::compute_t_wo of the left arm, then Eigen's
 * Quaterniond(Matrix3d) — ccmp_kin.h: quat_of, the trace / largest-diagonal branches exactly as oracle/ccmp_oracle.c: R_to_quat
 * restates them (plain multiplications and additions, no FMA, one correctly rounded square root and one quotient). */
#ifndef CCMP_POSE_H
#define CCMP_POSE_H
#include "ccmp_kin.h"

#define CCMP_POSE_STRIDE 8
#define CCMP_POSE_ROT_CUTOFF (1.0 - 1e-9) /* OMPL: 1.0 - MAX_QUATERNION_NORM_ERROR */

/* squared translation part: the chain of orc_distance over x, y, z (what the k-NN kernels' pre-filter compares) */
CCMP_HD double ccmp_pose_d2(double ax, double ay, double az, double bx, double by, double bz)
{
  const double ex = ax - bx, ey = ay - by, ez = az - bz;
  double d2 = 0.0;
  d2 = CCMP_FMA(ex, ex, d2);
  d2 = CCMP_FMA(ey, ey, d2);
  d2 = CCMP_FMA(ez, ez, d2);
  return d2;
}

/* SO3StateSpace::arcLength from the eight quaternion components, (x, y, z, w) each */
CCMP_HD double ccmp_pose_rot(double ax, double ay, double az, double aw, double bx, double by, double bz, double bw)
{
  double dot = 0.0;
  dot = CCMP_FMA(ax, bx, dot);
  dot = CCMP_FMA(ay, by, dot);
  dot = CCMP_FMA(az, bz, dot);
  dot = CCMP_FMA(aw, bw, dot);
  const double dq = ccmp_abs(dot);
  if (dq > CCMP_POSE_ROT_CUTOFF) return 0.0;
  return ccmp_atan2_nn(ccmp_sqrt(CCMP_FMA(-dq, dq, 1.0)), dq); /* NaN: the comparison above fails and the NaN comes through */
}

/* SE3StateSpace::distance with weights 1 and 1 */
CCMP_HD double ccmp_pose_dist(const double *a, const double *b)
{
  return ccmp_sqrt(ccmp_pose_d2(a[0], a[1], a[2], b[0], b[1], b[2])) + ccmp_pose_rot(a[3], a[4], a[5], a[6], b[3], b[4], b[5], b[6]);
}

/* t_wo = R (9, row-major) then p (3), as ccmp_compute_t_wo_batch writes it -> pose[8] */
CCMP_HD void ccmp_pose_of_t_wo(const double *t_wo, double *pose)
{
  double q[4];
  ccmp::quat_of(t_wo, q);
  pose[0] = t_wo[9];
  pose[1] = t_wo[10];
  pose[2] = t_wo[11];
  pose[3] = q[0];
  pose[4] = q[1];
  pose[5] = q[2];
  pose[6] = q[3];
  pose[7] = 0.0;
}

#endif /* CCMP_POSE_H */
