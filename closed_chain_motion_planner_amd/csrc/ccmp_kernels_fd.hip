// ccmp_kernels_fd.hip — gfx950 kernels in the canonical (bit-reproducible) rounding model.
//
// Built with -ffp-contract=off -DCCMP_USE_FMA: the only fused operations are the CCMP_FMA calls in
// ccmp_detmath.h / ccmp_kin.h / this file, the same ones oracle/ccmp_oracle.c (det build) performs,
// so every kernel here is expected to agree with the CPU oracle BIT FOR BIT.
//
// Hot kernel: project_fd_kernel — KinematicChainConstraint::project with the reference's
// finite-difference Jacobian (include/closed_chain_motion_planner/base/constraints/
// ConstraintFunction.h:57-82 + OMPL's default Constraint::jacobian).
//
// Work decomposition: one wavefront = 10 independent samples x 6 lanes.
// The 6 lanes of a group are the 6 evaluation points of OMPL's 7-point central stencil
// (+h,+2h,+3h,-h,-2h,-3h) of ONE Jacobian column; the wave walks the 14 columns in lock-step, so
// arm/joint indices are wave-uniform and every kinematic constant is an SGPR operand.  A perturbed
// evaluation reuses the unperturbed prefix of the chain (bit-identical to recomputing it) from LDS
// and recomputes only the suffix.  Joint state, sines/cosines, prefix frames, tool poses, stencil
// values and the 2x14 Jacobian of each sample are staged in LDS (one 165-double record per group; odd
// stride => the 10 groups hit distinct banks, lanes of a group broadcast).  Groups pull samples from
// a global atomic queue (optionally in longest-predicted-first order, ccmp_kernels_scout.hip), so a
// group whose sample converges early refills while its neighbours keep iterating (iteration counts
// spread 15..250); when the queue runs dry the samples still in flight are handed to the
// wave-per-sample kernel (ccmp_kernels_wave.hip).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccmp_fd_common.h"

using namespace ccmp;

namespace {

constexpr int kGroup = 6;             // lanes per sample = stencil evaluations per column
constexpr int kGroupsPerWave = 10;    // 60 of 64 lanes busy
// LDS record of one group (in doubles).  The prefix frames are kept for ONE arm at a time (the
// second arm's chain is re-run before its columns: +343 operations per iteration, -84 doubles of
// LDS per sample).  A consumed prefix slot (12 doubles) then holds the 6 lanes' residual pairs of
// that column until the arm's stencil is combined; arm 0's Jacobian entries go to kJ0, arm 1's into
// arm 0's (by then dead) sin/cos slots.  165 x 8 B x 10 groups = 13.2 KB per wave -> 12 waves per CU.
constexpr int kX = 0;                 // x[14]        current iterate
constexpr int kSC = 14;               // sc[14][2]    sin, cos of every joint of x
constexpr int kPre = 42;              // pre[7][12]   chain frame in front of joint j of the current arm: R(9), o(3);
                                      //              once consumed: (f0, f1) of the 6 stencil points of column j
constexpr int kEE = 126;              // ee[2][12]    world tool pose of each arm at x: R(9), p(3)
constexpr int kJ0 = 150;              // J[:, 0..6]   interleaved (row0, row1) per column of arm 0
constexpr int kRec = 165;             // 164 used; odd stride keeps the 10 groups on distinct LDS banks.  13200 B per wave:
                                      // the allocation granule is 512 B, 12 x 13312 = 159744 <= 160 KiB (two more doubles
                                      // per group would round to 13824 and cost a wave per CU)

#ifndef CCMP_FD_WAVES_PER_SIMD
#define CCMP_FD_WAVES_PER_SIMD 3
#endif

// One arm's chain at x (sines/cosines from LDS) in the general instantiations (calibrated arms, tilted bases), whole in every
// lane; the STOCK instantiations run chain_rows below instead.  With STORE the writer lane keeps the frame in front of every
// joint (R before the joint's rotation, o including the joint's offset) in LDS.  A loop: unrolled, the general formulas spill.
template <int ARM, bool STORE>
__device__ __forceinline__ void chain_at_x(const ccmp_consts &K, double *rec, bool writer, double *T)
{
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
  for (int i = 0; i < 7; i++) {
    double Rj[9], Rn[9];
    mulvec_acc(R, K.offset[ARM][i], o);
    if (STORE && writer) {
#pragma unroll
      for (int k = 0; k < 9; k++) rec[kPre + i * 12 + k] = R[k];
#pragma unroll
      for (int k = 0; k < 3; k++) rec[kPre + i * 12 + 9 + k] = o[k];
    }
    rot_sc(K.axis[ARM][i], K.aprod[ARM][i], rec[kSC + 2 * (ARM * 7 + i)], rec[kSC + 2 * (ARM * 7 + i) + 1], Rj);
    mul33(R, Rj, Rn);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
  }
  tool_pose_t<false>(K, ARM, R, o, &T[0], &T[9]);
}

// A general joint (1, 3, 5, 6) of the stock Panda in the STOCK instantiations: Rn = R * Rot(axis_i, angle).  X0: the short form
// rot_sc_x0 (7 operations for rot_sc's 13, the same bits: ccmp_kin.h).  It is exact only away from angle 0, so the choice is made
// ONCE per Newton round and wavefront (ccmp_fd_newton_phase1.inc: rot_x0_round_ok on every joint of every sample the wavefront
// iterates on — the test covers the six stencil points of each column as well) and selects between two copies of the round's
// kinematics, piece by piece (ccmp_fd_newton_phase2.inc).  Measured: a test and a scalar branch at every rotation instead cost
// more than the short form saved (+2.2 %: the branches cut the scheduler's regions where a rotation overlaps the product in
// front of it); the two copies pay -2.7 % (DESIGN_experiments.md §5.6).
template <bool X0>
__device__ __forceinline__ void stock_rot_mul(const ccmp_consts &K, int i, double s, double c, const double *R, double *Rn)
{
  double Rj[9];
  if constexpr (X0) rot_sc_x0(K.axis[0][i], K.aprod[0][i], s, c, Rj);
  else rot_sc(K.axis[0][i], K.aprod[0][i], s, c, Rj);
  mul33(R, Rj, Rn);
}

// ---- the chains at x, one matrix ROW per lane (STOCK instantiation: twin arms, diag(+-1) base frames) ---------------
// Row r of (R * Rj) needs row r of R only, and o[r] += R[r,:] * offset likewise: lane `row` of an arm's three lanes
// carries one row of the running frame (3 + 1 doubles) and does a third of every product — per element the same
// operations on the same operands as mul33 / mulvec_acc, hence the same bits.  Lanes 0..2 of a group run arm 0,
// lanes 3..5 arm 1, side by side (both arms read arm 0's constants: they are bit-identical, K.twin_arms); only the
// joint's rotation matrix (13 operations) is computed by every lane.  175 + 19 operations per lane for BOTH chains
// and tool poses instead of 2 x (343 + 48) when every lane ran both chains whole.  The lanes of arm `store_arm` keep
// the frame in front of every joint in LDS (R row before the joint's rotation, o including the joint's offset) for
// that arm's Jacobian columns; with TOOL every lane also leaves its row of the arm's world tool pose in LDS.
template <bool TOOL, bool X0, int I>
__device__ __forceinline__ void chain_rows_from(const ccmp_consts &K, double *rec, const double *sc, int row, bool store,
                                                double &R0, double &R1, double &R2, double &o)
{
  if constexpr (I < 7) {
    constexpr int NZ = kStockOff[I];
    if (NZ & 1) o = CCMP_FMA(R0, K.offset[0][I][0], o);
    if (NZ & 2) o = CCMP_FMA(R1, K.offset[0][I][1], o);
    if (NZ & 4) o = CCMP_FMA(R2, K.offset[0][I][2], o);
    if (store) {
      rec[kPre + I * 12 + 3 * row] = R0;
      rec[kPre + I * 12 + 3 * row + 1] = R1;
      rec[kPre + I * 12 + 3 * row + 2] = R2;
      rec[kPre + I * 12 + 9 + row] = o;
    }
    const double s = sc[2 * I], c = sc[2 * I + 1];
    double n0, n1, n2;
    if constexpr (kStockZ[I] != 0) { // mul_zrot, one row
      const double t = 1.0 - c;
      const double w = t + c;
      const double ns = -s;
      n0 = CCMP_FMA(R1, s, R0 * c);
      n1 = CCMP_FMA(R1, c, R0 * ns);
      n2 = R2 * w;
    } else { // rot_sc (X0: its short form, see stock_rot_mul) + one row of mul33
      double Rj[9];
      if constexpr (X0) rot_sc_x0(K.axis[0][I], K.aprod[0][I], s, c, Rj);
      else rot_sc(K.axis[0][I], K.aprod[0][I], s, c, Rj);
      n0 = dot3(R0, Rj[0], R1, Rj[3], R2, Rj[6]);
      n1 = dot3(R0, Rj[1], R1, Rj[4], R2, Rj[7]);
      n2 = dot3(R0, Rj[2], R1, Rj[5], R2, Rj[8]);
    }
    R0 = n0; R1 = n1; R2 = n2;
    chain_rows_from<TOOL, X0, I + 1>(K, rec, sc, row, store, R0, R1, R2, o);
  }
}
template <bool TOOL, bool X0>
__device__ __forceinline__ void chain_rows(const ccmp_consts &K, double *rec, int arm, int row, bool live, int store_arm,
                                           double d_lane, double bp_lane)
{
  double R0 = row == 0 ? 1.0 : 0.0, R1 = row == 1 ? 1.0 : 0.0, R2 = row == 2 ? 1.0 : 0.0, o = 0.0;
  chain_rows_from<TOOL, X0, 0>(K, rec, rec + kSC + 14 * arm, row, live && arm == store_arm, R0, R1, R2, o);
  if constexpr (TOOL) { // tool_pose_t<true>, diag(+-1) base frame, one row
    double pf = o;
    if (kStockEe & 1) pf = CCMP_FMA(R0, K.ee[0][0], pf);
    if (kStockEe & 2) pf = CCMP_FMA(R1, K.ee[0][1], pf);
    if (kStockEe & 4) pf = CCMP_FMA(R2, K.ee[0][2], pf);
    const double *Rt = K.R_tool[0];
    const double f0 = dot3(R0, Rt[0], R1, Rt[3], R2, Rt[6]);
    const double f1 = dot3(R0, Rt[1], R1, Rt[4], R2, Rt[7]);
    const double f2 = dot3(R0, Rt[2], R1, Rt[5], R2, Rt[8]);
    if (live) {
      double *T = rec + kEE + 12 * arm;
      T[3 * row] = d_lane * f0;
      T[3 * row + 1] = d_lane * f1;
      T[3 * row + 2] = d_lane * f2;
      T[9 + row] = CCMP_FMA(d_lane, pf, bp_lane);
    }
  }
}

// ---- suffix steps of the stock Panda (STOCK instantiation) -----------------------------------------------------------
// The joints alternate: 0, 2, 4 rotate about exactly (0, 0, 1); 1, 3, 5 and 6 about a general axis; most offset
// components are exactly zero (ccmp_kin.h: kStockZ, kStockOff).  With run-time (wave-uniform) joint indices the steps
// come in three shapes, each skipping only products with components that are exact zeros for EVERY joint it serves
// (a product with an exact zero that is not skipped adds an exact zero: same bits either way):
//   z step       joints 2, 4     o += R[:,0] off.x + R[:,2] off.z  (joint 2: off.x == 0),  R = R * Rz(q)
//   general step joints 1, 3, 5  o += R[:,0] off.x                 (joints 1, 5: off.x == 0), R = R * Rot(axis, q)
//   last step    joint 6         o += R[:,0] off.x,                                           R = R * Rot(axis, q)
__device__ __forceinline__ void stock_z_step(const ccmp_consts &K, int i, double s, double c, const double *R, double *Rn, double *o)
{
  const double ox = K.offset[0][i][0], oz = K.offset[0][i][2];
#pragma unroll
  for (int r = 0; r < 3; r++) o[r] = CCMP_FMA(R[3 * r + 2], oz, CCMP_FMA(R[3 * r], ox, o[r]));
  mul_zrot(R, s, c, Rn);
}
template <bool X0>
__device__ __forceinline__ void stock_g_step(const ccmp_consts &K, int i, double s, double c, const double *R, double *Rn, double *o)
{
  const double ox = K.offset[0][i][0];
#pragma unroll
  for (int r = 0; r < 3; r++) o[r] = CCMP_FMA(R[3 * r], ox, o[r]);
  stock_rot_mul<X0>(K, i, s, c, R, Rn);
}

// OMPL's default Constraint::jacobian, evaluation part, for the 7 columns of one arm: each lane evaluates
// its stencil point of column j from the cached prefix frame and parks the residual pair in LDS.  X0 (STOCK only): the general
// joints' rotations in their short form (stock_rot_mul).
template <int ARM, bool STOCK, bool X0 = false>
__device__ __forceinline__ void jacobian_columns(const ccmp_consts &K, double *rec, bool live, int r, bool plus, int nstep)
{
  double To[12]; // the other arm's (unperturbed) tool pose: 24 VGPRs that save 12 LDS reads per column (-6.5 %, A/B)
#pragma unroll
  for (int k = 0; k < 12; k++) To[k] = rec[kEE + (1 - ARM) * 12 + k];
  // arm 0's columns: chain_residual's ti = R2^T p2 is arm 1's alone — once here, in place of p2 (no register added)
  if (ARM == 0) {
    double ti[3];
    mulTvec(&To[0], &To[9], ti);
#pragma unroll
    for (int k = 0; k < 3; k++) To[9 + k] = ti[k];
  }
  constexpr bool kOtherP = ARM == 1; // arm 0's columns hold ti in place of the other arm's translation
  // STOCK: twin arms on diag(+-1) base frames (launchers).  This arm's +-1 factors go into the other arm's pose once, here,
  // instead of into this arm's nine rotation entries at every stencil point (ccmp_kin.h: tool_pose_fold)
  if constexpr (STOCK) fold_other_pose<kOtherP>(K, ARM, To);
  for (int j = 0; j < 7; j++) {
    const double xj = rec[kX + ARM * 7 + j];
    const double axj = ccmp_abs(xj);
    const double h = 1.4901161193847656e-08 * (axj >= 1 ? axj : 1); // sqrt(eps)*max(1,|x_j|)
    const double hh = plus ? h : -h;
    double y = xj + hh;                 // y1[j] += h   /  y2[j] -= h
    if (nstep >= 2) y = y + hh;
    if (nstep >= 3) y = y + hh;
    double R[9], o[3], s, c;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rec[kPre + j * 12 + k];
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = rec[kPre + j * 12 + 9 + k];
    if constexpr (X0) ccmp_sincos_inr(y, &s, &c); // an in-range round: |y| <= 512 + 3 h, no range test (ccmp_detmath.h)
    else ccmp_sincos(y, &s, &c);
    const double *sc = rec + kSC + 2 * ARM * 7;
    if constexpr (STOCK) {
      // twin arms: arm 0's constants serve both.  Joint indices are wave-uniform scalars; the branches are scalar.
      // The frame ends every step in R (R -> Rn -> R, or in place): no register copies between steps.
      double Rn[9];
      int i = j + 1;
      if ((j & 1) == 0 && j < 6) { // joints 0, 2, 4: R = R * Rz(y), row by row in place (mul_zrot's operations)
        const double t = 1.0 - c;
        const double w = t + c;
        const double ns = -s;
#pragma unroll
        for (int rr = 0; rr < 3; rr++) {
          const double a = R[3 * rr], b = R[3 * rr + 1];
          R[3 * rr] = CCMP_FMA(b, s, a * c);
          R[3 * rr + 1] = CCMP_FMA(b, c, a * ns);
          R[3 * rr + 2] = R[3 * rr + 2] * w;
        }
      } else {
        stock_rot_mul<X0>(K, j, s, c, R, Rn);
        if (j < 6) { // j = 1, 3, 5: the next joint (2, 4 or 6) takes the frame back to R
          if (i < 6) stock_z_step(K, i, sc[2 * i], sc[2 * i + 1], Rn, R, o);
          else stock_g_step<X0>(K, 6, sc[12], sc[13], Rn, R, o);
          i++;
        } else { // j = 6: no suffix
#pragma unroll
          for (int k = 0; k < 9; k++) R[k] = Rn[k];
        }
      }
      for (; i < 5; i += 2) { // (1, 2), (3, 4): general step then z step, R -> Rn -> R
        stock_g_step<X0>(K, i, sc[2 * i], sc[2 * i + 1], R, Rn, o);
        stock_z_step(K, i + 1, sc[2 * i + 2], sc[2 * i + 3], Rn, R, o);
      }
      if (i == 5) { // (5, 6): joint 5 has no offset at all
        stock_rot_mul<X0>(K, 5, sc[10], sc[11], R, Rn);
        stock_g_step<X0>(K, 6, sc[12], sc[13], Rn, R, o);
      }
    } else {
      {
        double Rj[9], Rn[9];
        rot_sc(K.axis[ARM][j], K.aprod[ARM][j], s, c, Rj);
        mul33(R, Rj, Rn);
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = Rn[k];
      }
      {
        // suffix joints two at a time, R -> Rn -> R: no register copies of the frame between steps (61 instead of
        // 76 instructions per joint; -0.6 % run time, A/B)
        int i = j + 1;
        if ((7 - i) & 1) {
          joint_step(K, ARM, i, sc[2 * i], sc[2 * i + 1], R, o);
          i++;
        }
        for (; i < 7; i += 2) {
          double Rj[9], Rn[9];
          mulvec_acc(R, K.offset[ARM][i], o);
          rot_sc(K.axis[ARM][i], K.aprod[ARM][i], sc[2 * i], sc[2 * i + 1], Rj);
          mul33(R, Rj, Rn);
          mulvec_acc(Rn, K.offset[ARM][i + 1], o);
          rot_sc(K.axis[ARM][i + 1], K.aprod[ARM][i + 1], sc[2 * i + 2], sc[2 * i + 3], Rj);
          mul33(Rn, Rj, R);
        }
      }
    }
    double Tw[12], t[2];
    if constexpr (STOCK) tool_pose_fold<STOCK>(K, ARM, R, o, &Tw[0], &Tw[9]);
    else tool_pose_t<STOCK>(K, ARM, R, o, &Tw[0], &Tw[9]);
    if constexpr (X0) { // ... and the quaternion's root and quotient without their guards, its case once per wavefront (ccmp_kin.h: quat_of_t)
      if (ARM == 0) chain_residual_t<true, true>(K, &Tw[0], &Tw[9], &To[0], &To[9], t, nullptr, nullptr);
      else chain_residual_t<false, true>(K, &To[0], &To[9], &Tw[0], &Tw[9], t, nullptr, nullptr);
    } else if (ARM == 0) chain_residual_ti(K, &Tw[0], &Tw[9], &To[0], &To[9], t, nullptr, nullptr);
    else chain_residual(K, &To[0], &To[9], &Tw[0], &Tw[9], t, nullptr, nullptr);
    // park this evaluation in the prefix slot the group has just consumed (12 doubles = 6 lanes x (f0, f1));
    // the stencil is combined after the arm's 7 columns (stencil_combine) instead of through two dependent
    // ds_bpermute rounds per column
    if (live) {
      rec[kPre + 12 * j + 2 * r] = t[0];
      rec[kPre + 12 * j + 2 * r + 1] = t[1];
    }
  }
}

// out.col(j) = 1.5*m1 - 0.6*m2 + 0.1*m3 with m_s = (t1 - t2) / (y1[j] - y2[j]) for the 7 columns of one arm:
// 14 entries spread over the group's 6 lanes; y1/y2 are rebuilt by the same sequential adds the evaluations
// used.  Arm 0's entries go to kJ0, arm 1's into arm 0's (by now dead) sin/cos slots.
template <int ARM>
__device__ __forceinline__ void stencil_combine(double *rec, int r, bool live)
{
#pragma unroll
  for (int n = 0; n < 3; n++) {
    const int e = r + kGroup * n; // entry: column e >> 1, row e & 1
    if (e < 14 && live) {
      const int c = e >> 1, row = e & 1;
      const double xj = rec[kX + ARM * 7 + c];
      const double axj = ccmp_abs(xj);
      const double h = 1.4901161193847656e-08 * (axj >= 1 ? axj : 1);
      double y1 = xj, y2 = xj, m[3];
#pragma unroll
      for (int sidx = 0; sidx < 3; sidx++) {
        y1 = y1 + h;
        y2 = y2 - h;
        m[sidx] = (rec[kPre + 12 * c + 2 * sidx + row] - rec[kPre + 12 * c + 2 * (sidx + 3) + row]) / (y1 - y2);
      }
      const double Jv = CCMP_FMA(0.1, m[2], CCMP_FMA(-0.6, m[1], 1.5 * m[0]));
      if (ARM == 0) rec[kJ0 + 2 * c + row] = Jv;
      else rec[kSC + 2 * c + row] = Jv;
    }
  }
}

// MODE 0: project q_in -> q_out.  MODE 1: sampleUniform = ambient sample -> project -> enforceBounds.
// PART (ccmp_launch.h: FdPart) — which part of a call the launch is:
//   whole   the persistent, queue-fed kernel from a sample's first round to its last (every regime but the one below)
//   head    large batches without hand-over: the first head_rounds Newton rounds of EVERY sample, non-persistent: workgroup w takes
//           samples 10 w .. 10 w + 9 in index order, so the ten samples of a wavefront are of one age — far from the manifold all
//           together, for four or five rounds, and done with it; it stops BEHIND phase 1 of round head_rounds: each sample still
//           iterating there leaves its staged record (kStagedRow doubles, ccmp_launch.h: what that phase 1 computed, index, counters)
//           in row idx of `state`; one that ends earlier, or in that phase 1, is written back as ever and its row is marked finished
//           (index -1)
//   resume  the persistent kernel again, in a loop of its own that admits BEHIND the finish block: a group takes the staged record of
//           its next sample into LDS and registers and goes straight into phase 2 of the round its predecessor ended in — no group
//           sits out a phase 2 because its sample is new; it draws again (kResumeDraws times, then waits a round) where the row is
//           marked finished.  Its wavefronts hold samples of all ages, none of them far from the manifold: ccmp_atan's wave-uniform
//           first interval (ccmp_detmath.h) holds in nearly every round, where one young sample among the ten defeated it in two
//           rounds of three.
//   (STOCK instantiations.  The general ones — calibrated arms, tilted bases — keep the form the two launches had before: the head
//   dumps at the loop top of round head_rounds the hand-over's record, kPoolEntry doubles, and the resume launch refills from it at its
//   loop top, in the whole kernel's loop; their register allocation is pinned by tests/test_gpu_fd_round_facts.py.)
// The operations on a sample are the same ones in the same order whichever launches perform them: same bits.
// VARIANT = MODE + 2 * PART in ONE integer: the kernels' names keep the form project_fd_kernel<n, stock> (build.py: _SCRATCH_RULES).
using ccmp_launch::FdPart;
using ccmp_launch::kFdHead;
using ccmp_launch::kFdResume;
using ccmp_launch::kFdWhole;
constexpr int kResumeDraws = 4;
// A sample's iterate into its group's record.  From a row of 14 doubles (q_in, or the row the head left) as seven 16-B pieces: lanes
// 0..5 of the group take 96 contiguous bytes in ONE instruction, lane 0 the last piece (14 single-lane 8-B loads before: same data,
// 7x the requests).  MODE 1, head launch: the ambient draw, every lane its entries (the refill of a whole call keeps its own copy of
// these lines: through this function project_fd_kernel<1, true> came out with another register allocation).
__device__ __forceinline__ void iterate_from_row(double *rec, int r, const double *__restrict__ src)
{
  const double2 *row = reinterpret_cast<const double2 *>(src);
  const double2 a = row[r];
  rec[kX + 2 * r] = a.x;
  rec[kX + 2 * r + 1] = a.y;
  if (r == 0) {
    const double2 b = row[6];
    rec[kX + 12] = b.x;
    rec[kX + 13] = b.y;
  }
}
__device__ __forceinline__ void iterate_from_draw(const ccmp_consts &K, double *rec, int r, unsigned long long seed, unsigned long long first_index,
                                                  unsigned long long idx, double *q_ambient)
{
#pragma unroll
  for (int e = 0; e < 14; e++) {
    if (e % kGroup == r) { // e is a compile-time constant here: bounds come from SGPRs
      const double v = ambient_uniform(K, seed, first_index + idx, e);
      if (q_ambient) q_ambient[idx * 14 + e] = v;
      rec[kX + e] = v;
    }
  }
}
// head: the sample of group g of this workgroup.  It never changes, but it is NOT held across the Newton loop, and neither are the
// four row addresses that follow from it: formed where it is used, from a group index the optimiser cannot see through (as the
// lane's slots in ccmp_fd_newton_phase2.inc) — hoisted, they were the registers that the head's instantiations spilled.
__device__ __forceinline__ unsigned long long head_sample(int g)
{
  asm volatile("" : "+v"(g));
  return (unsigned long long)blockIdx.x * kGroupsPerWave + (unsigned long long)g;
}
// head -> resume: a group's staged record (ccmp_launch.h: kStagedRow) to and from its row of `state`.  The LDS part is 75 pieces of 16 B:
// lane r of the group moves pieces r, r + 6, ... — 96 contiguous bytes per group and instruction, as iterate_from_row's; the four pieces
// behind it (residual pair, index and counters, norms, the group's say in x0) are written by lane 0 and read by every lane for itself.
using ccmp_launch::kStagedF;
using ccmp_launch::kStagedLds;
using ccmp_launch::kStagedNorm;
using ccmp_launch::kStagedRow;
using ccmp_launch::kStagedTag;
using ccmp_launch::kStagedX0;
static_assert(kStagedLds == kJ0 && kX == 0, "the staged part of a record is everything in front of the Jacobian's slots");
constexpr int kStagedPieces = kStagedLds / 2;
__device__ __forceinline__ void stage_to_row(const double *rec, int r, double *__restrict__ dst, unsigned long long idx, double f0, double f1,
                                             int iter, int updates, double norm1, double norm2, bool x0_off)
{
  double2 *row = reinterpret_cast<double2 *>(dst);
  for (int p = r; p < kStagedPieces; p += kGroup) {
    double2 a;
    a.x = rec[2 * p];
    a.y = rec[2 * p + 1];
    row[p] = a;
  }
  if (r == 0) {
    double2 f, tag, nrm, flag;
    f.x = f0; f.y = f1;
    tag.x = __longlong_as_double((long long)idx); tag.y = __hiloint2double(updates, iter);
    nrm.x = norm1; nrm.y = norm2;
    flag.x = x0_off ? 1.0 : 0.0; flag.y = 0.0;
    row[kStagedF / 2] = f;
    row[kStagedTag / 2] = tag;
    row[kStagedNorm / 2] = nrm;
    row[kStagedX0 / 2] = flag;
  }
}
__device__ __forceinline__ void stage_from_row(double *rec, int r, const double *__restrict__ src)
{
  // (the lane's piece index goes through a value the optimiser cannot see through, as head_sample's group index: the thirteen LDS
  // offsets that follow from it were otherwise formed once, in front of the resume loop, and held across it — registers the kernel does
  // not have.  From one base the pieces are immediate offsets.)
  asm volatile("" : "+v"(r));
  const double2 *row = reinterpret_cast<const double2 *>(src) + r;
  double *dst = rec + 2 * r;
  constexpr int kFull = kStagedPieces / kGroup; // 12 pieces that every lane has, one more for the first kStagedPieces % kGroup lanes
  double2 a[kFull + 1];
#pragma unroll
  for (int k = 0; k < kFull; k++) a[k] = row[kGroup * k];
  const bool last = r < kStagedPieces - kGroup * kFull;
  if (last) a[kFull] = row[kGroup * kFull];
#pragma unroll
  for (int k = 0; k < kFull; k++) {
    dst[2 * kGroup * k] = a[k].x;
    dst[2 * kGroup * k + 1] = a[k].y;
  }
  if (last) {
    dst[2 * kGroup * kFull] = a[kFull].x;
    dst[2 * kGroup * kFull + 1] = a[kFull].y;
  }
}
template <int VARIANT, bool STOCK>
__global__ __launch_bounds__(64, CCMP_FD_WAVES_PER_SIMD) void project_fd_kernel(
    const ccmp_consts K, const double *__restrict__ q_in, double *__restrict__ q_out, uint8_t *__restrict__ ok_out,
    uint16_t *__restrict__ iters_out, double *__restrict__ q_ambient, unsigned long long B, unsigned long long *queue,
    unsigned long long seed, unsigned long long first_index, double *__restrict__ pool, unsigned long long *pool_count,
    int dump_threshold, const unsigned int *__restrict__ order, const uint16_t *__restrict__ pred, int long_remaining,
    unsigned long long pool_records, double *__restrict__ state, int head_rounds)
{
  constexpr int MODE = VARIANT & 1, PART = VARIANT >> 1;
  // rows of `state`: staged records between the STOCK head and resume, the hand-over's record between the general ones
  constexpr int kStateRow = STOCK ? kStagedRow : kPoolEntry, kStateTag = STOCK ? kStagedTag : 14;
  if constexpr (PART != kFdWhole) pool = nullptr; // neither part hands over (ccmp_policy.cpp): the text below that does folds away
  __shared__ double lds[kGroupsPerWave * kRec];
  const int lane = threadIdx.x;
  const int g = lane / kGroup;                // 0..10; lanes 60..63 form the idle "group 10"
  const int r = lane - kGroup * g;            // evaluation point 0..5 inside the group
  const bool live = g < kGroupsPerWave;
  const int leader = live ? kGroup * g : 0;
  double *rec = lds + (live ? g : 0) * kRec;  // idle lanes alias group 0 for reads, never write
  const bool writer = live && r == 0;
  const bool plus = r < 3;                    // y1 side of the stencil; r>=3 is the y2 side
  const int nstep = (plus ? r : r - 3) + 1;   // how many h-steps this lane's point is away
  // chains at x by rows (STOCK): lane r of a group carries row r % 3 of arm r / 3; its entry of the arm's diag(+-1)
  // base rotation and of the base translation are the only lane-dependent constants
  const int arm_l = plus ? 0 : 1, row_l = plus ? r : r - 3;
  double d_lane = 0.0, bp_lane = 0.0;
  if constexpr (STOCK) {
    d_lane = arm_l ? (row_l == 0 ? K.base_R[1][0] : (row_l == 1 ? K.base_R[1][4] : K.base_R[1][8]))
                   : (row_l == 0 ? K.base_R[0][0] : (row_l == 1 ? K.base_R[0][4] : K.base_R[0][8]));
    bp_lane = arm_l ? (row_l == 0 ? K.base_p[1][0] : (row_l == 1 ? K.base_p[1][1] : K.base_p[1][2]))
                    : (row_l == 0 ? K.base_p[0][0] : (row_l == 1 ? K.base_p[0][1] : K.base_p[0][2]));
  }

  unsigned long long idx = 0;
  int iter = 0, updates = 0;
  double norm1 = 0.0, norm2 = 0.0;
  bool active = false, drained = false;
  int round = 0; // head: Newton rounds done, the same for all ten samples
  if constexpr (PART == kFdHead) { // the group's one sample, taken in front of the loop: nothing of the draw is live across it
    idx = head_sample(g);
    if (live && idx < B) {
      active = true;
      if (MODE == 0) iterate_from_row(rec, r, q_in + idx * 14);
      else iterate_from_draw(K, rec, r, seed, first_index, idx, q_ambient);
    }
  }

#define CCMP_FD_BP bp_lane
#define CCMP_FD_X0_ROWS 1
  // ---- resume: admit -> phase 2 -> phase 1 -> finish -> admit -> ...  Every row it admits holds a sample behind ITS phase 1, so a
  // group whose sample ends in phase 1 of a round is written back and its successor runs phase 2 of that same round (refilled at the
  // loop top, as the whole kernel does, the group sat out the four fifths of a round that phase 2 is)
  if constexpr (PART == kFdResume && STOCK) {
    double f0c = 0.0, f1c = 0.0;       // the group's residual pair, from phase 1 (or the row) into phase 2
    bool x0c = K.rot_x0 != 0; // phase 1's x0 over the groups that go on, for phase 2
    for (;;) {
      // ---- admission: the whole kernel's tickets; a row marked finished (the head has written the sample back) costs a draw, and
      // after kResumeDraws of them the group waits a round
      bool admitted = false;
      for (int draw = 0; draw < kResumeDraws; draw++) {
        const bool want = live && !active && !drained;
        if (__builtin_amdgcn_ballot_w64(want) == 0ull) break;
        unsigned long long t = 0;
        if (want && r == 0) t = atomicAdd(queue, 1ull);
        t = shfl_u64(t, leader);
        if (want) {
          if (t < B) {
            idx = order ? (unsigned long long)order[t] : t;
            const double2 tag = reinterpret_cast<const double2 *>(state + idx * kStagedRow)[kStagedTag / 2];
            if (__double_as_longlong(tag.x) >= 0) {
              active = true; admitted = true;
              iter = __double2loint(tag.y); updates = __double2hiint(tag.y);
            }
          } else drained = true;
        }
      }
      bool adm_off = false;
      if (admitted) { // the record into the group's LDS, the rest into the lanes' registers (one address per group: a broadcast)
        const double *src = state + idx * kStagedRow;
        const double2 *row = reinterpret_cast<const double2 *>(src);
        const double2 f = row[kStagedF / 2], nrm = row[kStagedNorm / 2];
        f0c = f.x; f1c = f.y; norm1 = nrm.x; norm2 = nrm.y;
        adm_off = src[kStagedX0] != 0.0;
        stage_from_row(rec, r, src);
      }
      // the round's x0 covers the samples admitted into it: the flags that THEIR phase 1 computed, in the head
      x0c = x0c && __builtin_amdgcn_ballot_w64(adm_off) == 0ull;
      if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
        // (finished rows only leave the groups without a sample and the queue not yet dry — draw again)
        if (__builtin_amdgcn_ballot_w64(live && !drained) != 0ull) continue;
        break;
      }
      __syncthreads();
      {
        const bool x0 = x0c, cont = active; // every sample a group holds here is behind a loop test that said go on
        const double f0 = f0c, f1 = f1c;
#include "ccmp_fd_newton_phase2.inc"
      }
#include "ccmp_fd_newton_phase1.inc"
#include "ccmp_fd_project_finish.inc"
      f0c = f0; f1c = f1;
      x0c = K.rot_x0 != 0 && __builtin_amdgcn_ballot_w64(cont && x0_off) == 0ull;
      __syncthreads(); // the write-back has read the records that the admission overwrites
    }
    return;
  }

  for (;;) {
    // ---- refill: groups without a sample pull the next index from the global queue ----------
    if constexpr (PART == kFdResume) {
      // (general instantiation) the same tickets, the sample's state from its row of `state`: x in 16-B pieces as below, the index and
      // the counters by every lane of the group for itself (one address: a broadcast)
      for (int draw = 0; draw < kResumeDraws; draw++) {
        const bool want = live && !active && !drained;
        if (__builtin_amdgcn_ballot_w64(want) == 0ull) break;
        unsigned long long t = 0;
        if (want && r == 0) t = atomicAdd(queue, 1ull);
        t = shfl_u64(t, leader);
        if (want) {
          if (t < B) {
            idx = order ? (unsigned long long)order[t] : t;
            const double2 *row = reinterpret_cast<const double2 *>(state + idx * kPoolEntry);
            const double2 tag = row[7], nrm = row[8];
            if (__double_as_longlong(tag.x) >= 0) { // (a row marked finished: the head has written the sample back)
              active = true;
              iter = __double2loint(tag.y); updates = __double2hiint(tag.y); norm1 = nrm.x; norm2 = nrm.y;
              iterate_from_row(rec, r, state + idx * kPoolEntry);
            }
          } else drained = true;
        }
      }
    } else if constexpr (PART == kFdWhole) {
      const bool want = live && !active && !drained;
      unsigned long long t = 0;
      if (want && r == 0) t = atomicAdd(queue, 1ull);
      t = shfl_u64(t, leader);
      if (want) {
        if (t < B) {
          idx = order ? (unsigned long long)order[t] : t; // ticket -> sample: longest-predicted-first when scheduled
          active = true; iter = 0; updates = 0; norm1 = 0.0; norm2 = 0.0;
          if (MODE == 0) iterate_from_row(rec, r, q_in + idx * 14);
          else {
#pragma unroll
            for (int e = 0; e < 14; e++) {
              if (e % kGroup == r) { // e is a compile-time constant here: bounds come from SGPRs
                const double v = ambient_uniform(K, seed, first_index + idx, e);
                if (q_ambient) q_ambient[idx * 14 + e] = v;
                rec[kX + e] = v;
              }
            }
          }
        } else drained = true;
      }
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      // (resume: ten finished rows in a row leave the groups without a sample and the queue not yet dry — draw again)
      if (PART == kFdResume && __builtin_amdgcn_ballot_w64(live && !drained) != 0ull) continue;
      break;
    }
    __syncthreads();
    // ---- head, general instantiation: the loop top of round head_rounds, where the next thing that happens to a sample is function(x)
    // + the loop test — the samples still iterating leave their records (the hand-over's, in row idx) and the wavefront retires
    if constexpr (PART == kFdHead && !STOCK) {
      if (round == head_rounds) {
        idx = head_sample(g);
        if (active) {
          double *ent = state + idx * kPoolEntry;
          for (int e = r; e < 14; e += kGroup) ent[e] = rec[kX + e];
          if (r == 0) {
            ent[14] = __longlong_as_double((long long)idx);
            ent[15] = __hiloint2double(updates, iter);
            ent[16] = norm1;
            ent[17] = norm2;
          }
        }
        break;
      }
      round++;
    }
    // ---- hand-over: once the queue is empty the samples still in flight go to the straggler pool
    // (x, index, counters — everything else is recomputed from x) and the wave retires; the
    // wave-per-sample kernel finishes them.  State is dumped at the loop top, where the next thing
    // that happens to a sample is function(x) + the loop test — exactly where the other kernel starts.
    // every wave looks at the queue head once per iteration, so that all waves retire within one
    // iteration of the queue running dry (not only those that happen to finish a sample)
    bool dry = __builtin_amdgcn_ballot_w64(drained) != 0ull;
    if (pool != nullptr && !dry) {
      unsigned long long head = 0;
      if (lane == 0) head = __hip_atomic_load(queue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      head = shfl_u64(head, 0);
      dry = head >= B;
    }
    // occupancy-driven hand-over (dump_threshold > 10: its excess over 10 is a percentage): with the queue dry the waves
    // keep iterating while the samples in flight — B minus the finished count in queue[3] — still fill that share of
    // the launch's group slots, and all hand over together once they do not
    if (pool != nullptr && dry && dump_threshold > 10) {
      unsigned long long done = 0;
      if (lane == 0) done = __hip_atomic_load(queue + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      done = shfl_u64(done, 0);
      const unsigned long long in_flight = B - done, slots = (unsigned long long)gridDim.x * kGroupsPerWave;
      if (in_flight * 100ull >= slots * (unsigned long long)(dump_threshold - 10)) dry = false;
    }
    if (pool != nullptr && dry &&
        __builtin_popcountll(__builtin_amdgcn_ballot_w64(active && r == 0)) <= dump_threshold) {
      // Two classes (round 3): samples the scout predicts to need long_remaining or more further iterations fill the pool
      // from the front, the others from the back, and the latency kernel takes the front first — the hand-over's longest
      // samples start at once instead of wherever the order of the dumps put them (a 200-round sample that started one
      // millisecond into the latency kernel's two was the end of a 32768-sample batch).  One reservation per wavefront
      // and class.  pool_records == 0: one class, filled from the front.
      bool is_long = true;
      if (pool_records != 0ull) is_long = active && pred != nullptr && (int)pred[idx] - iter >= long_remaining;
      const unsigned long long mL = __builtin_amdgcn_ballot_w64(active && r == 0 && is_long);
      const unsigned long long mS = __builtin_amdgcn_ballot_w64(active && r == 0 && !is_long);
      unsigned long long bL = 0, bS = 0;
      if (lane == 0) {
        if (mL) bL = atomicAdd(pool_count, (unsigned long long)__builtin_popcountll(mL));
        if (mS) bS = atomicAdd(pool_count + 5, (unsigned long long)__builtin_popcountll(mS));
      }
      bL = shfl_u64(bL, 0);
      bS = shfl_u64(bS, 0);
      const unsigned long long below = (1ull << leader) - 1ull;
      const unsigned long long slot = is_long ? bL + (unsigned long long)__builtin_popcountll(mL & below)
                                              : pool_records - 1ull - (bS + (unsigned long long)__builtin_popcountll(mS & below));
      if (active) {
        double *ent = pool + slot * kPoolEntry;
        for (int e = r; e < 14; e += kGroup) ent[e] = rec[kX + e];
        if (r == 0) {
          ent[14] = __longlong_as_double((long long)idx);
          ent[15] = __hiloint2double(updates, iter);
          ent[16] = norm1;
          ent[17] = norm2;
        }
      }
      break;
    }

#include "ccmp_fd_newton_phase1.inc"
#include "ccmp_fd_project_finish.inc"
    // ---- head, STOCK: behind function(x) + the loop test of round head_rounds the samples still iterating leave their staged records —
    // what phase 1 has just computed of them, and the counters behind the loop test's increment — in row idx, and the wavefront retires
    if constexpr (PART == kFdHead && STOCK) {
      if (round == head_rounds) {
        const bool off = ((__builtin_amdgcn_ballot_w64(x0_off) >> leader) & 0x3Full) != 0ull; // the group's say in phase 1's x0
        idx = head_sample(g);
        if (cont) stage_to_row(rec, r, state + idx * kStagedRow, idx, f0, f1, iter, updates, norm1, norm2, off);
        break;
      }
      round++;
    }
    if (__builtin_amdgcn_ballot_w64(cont) == 0ull) continue; // nobody iterates: straight to refill
    __syncthreads(); // prefix frames / tool poses written by the writer lane are visible to the group

#include "ccmp_fd_newton_phase2.inc"
#undef CCMP_FD_BP
#undef CCMP_FD_X0_ROWS
  }
}


// geodesic_group_kernel — the extend step (jy_ProjectedStateSpace::discreteGeodesic, src/base/jy_ProjectedStateSpace.cpp:
// 32-96) on the THROUGHPUT layout: ten edges x six lanes per wavefront, the Newton iteration of project_fd_kernel (the same
// device functions in the same order: same bits), and at the point where that kernel writes a finished sample back, the
// reference's bookkeeping between two projections — jointValid, the four break tests, the state list, the next
// interpolated state (geodesic_flat_kernel's, statement for statement: ccmp_kernels_geo.hip) — instead.  A Newton round
// costs this layout ~1 250 wave-instructions per edge against the latency kernel's ~2 700, and ~12 times the latency: it
// serves the SHORT edges of a bulk call (round budget, thousands of edges), beside geodesic_flat_kernel, which takes the
// front of the FP32 scout's longest-first order on the side stream (ccmp_api.cpp: geodesic_common).  interpolate == true
// semantics; first calls only (carry_out / round_budget as in the latency kernel; no carry_in); checkMotion's isSatisfied(to) comes from
// a launch in front of this one (target_ok).
// Per-edge state lives in the group's LDS record behind the projector's 165 doubles: previous accepted state (14), dist,
// running length, bound (3), and three counters — 185 doubles per group, 10 wavefronts per CU.
// (The two halves of the Newton round are ONE text, included into both kernels' loops: ccmp_fd_newton_phase1.inc / _phase2.inc.  Shared
// through functions instead, the general instantiations of both kernels came out with 2.3 KB of scratch — the allocator lost the
// scoping of the pose arrays; textual inclusion leaves both allocations as they were: 167 / 168 registers, no scratch for the stock
// instantiations.  What does spill is listed, and bounded at build time, in build.py: _SCRATCH_RULES.)
constexpr int kGPrev = kRec, kGDist = kRec + 14, kGCnt = kRec + 17, kRecG = kRec + 20; // odd stride like kRec
static_assert(kRecG % 2 == 1, "odd record stride: the ten groups stay on distinct LDS banks");

// WrapperStateSpace::interpolate through KinematicChainSpace::interpolate (KinematicChain.h:145-171), one joint
// (ccmp_detmath.h: ccmp_joint_interpolate, the one text)
__device__ __forceinline__ double geo_interpolate(double fr, double tg, double tt) { return ccmp_joint_interpolate(fr, tg, tt); }

#ifndef CCMP_GEO_GROUP_WAVES_PER_SIMD
#define CCMP_GEO_GROUP_WAVES_PER_SIMD CCMP_FD_WAVES_PER_SIMD
#endif
template <bool STOCK>
__global__ __launch_bounds__(64, CCMP_GEO_GROUP_WAVES_PER_SIMD) void geodesic_group_kernel(
    const ccmp_consts K, const double delta, const double lambda, const double *__restrict__ from, const double *__restrict__ to,
    unsigned long long E, int max_states, double *__restrict__ states, int *__restrict__ n_states, uint8_t *__restrict__ ok_out,
    int *__restrict__ newton_iters, unsigned long long *queue, const unsigned int *__restrict__ order,
    double *__restrict__ carry_out, int round_budget, double *__restrict__ pool, unsigned long long *pool_count, int handover_pct,
    const uint8_t *__restrict__ target_ok)
{
  __shared__ double lds[kGroupsPerWave * kRecG];
  __shared__ double lane_bp[64]; // the lane's base-frame offset (bp_lane below): parked here instead of in scratch
  const int lane = threadIdx.x;
  const int g = lane / kGroup;
  const int r = lane - kGroup * g;
  const bool live = g < kGroupsPerWave;
  const int leader = live ? kGroup * g : 0;
  double *rec = lds + (live ? g : 0) * kRecG; // idle lanes alias group 0 for reads, never write
  const bool writer = live && r == 0;
  const bool plus = r < 3;
  const int nstep = (plus ? r : r - 3) + 1;
  const int arm_l = plus ? 0 : 1, row_l = plus ? r : r - 3;
  double d_lane = 0.0, bp_lane = 0.0;
  if constexpr (STOCK) {
    d_lane = arm_l ? (row_l == 0 ? K.base_R[1][0] : (row_l == 1 ? K.base_R[1][4] : K.base_R[1][8]))
                   : (row_l == 0 ? K.base_R[0][0] : (row_l == 1 ? K.base_R[0][4] : K.base_R[0][8]));
    bp_lane = arm_l ? (row_l == 0 ? K.base_p[1][0] : (row_l == 1 ? K.base_p[1][1] : K.base_p[1][2]))
                    : (row_l == 0 ? K.base_p[0][0] : (row_l == 1 ? K.base_p[0][1] : K.base_p[0][2]));
  }
  lane_bp[lane] = bp_lane;
  // The lane's address offsets into from / to / states and its bit masks never change either, but they are NOT held across the
  // Newton loop: under the bound of three wavefronts per SIMD the allocator parked them in scratch.  They are recomputed where they
  // are used — once per edge or projection — from a lane index the optimiser cannot see through, which keeps it from hoisting them
  // back out of the loop.
  auto lane_opaque = [](int v) {
    asm volatile("" : "+v"(v));
    return v;
  };

  unsigned long long edge = 0;
  int iter = 0, updates = 0;
  double norm1 = 0.0, norm2 = 0.0;
  bool active = false, drained = false;

  for (;;) {
    // ---- refill: a group without an edge takes the next ticket and sets the edge up (the reference's prologue) ----------
    {
      const bool want = live && !active && !drained;
      unsigned long long t = 0;
      if (want && r == 0) t = atomicAdd(queue, 1ull);
      t = shfl_u64(t, leader);
      if (want) {
        if (t < E) {
          edge = order ? (unsigned long long)order[t] : t;
          const double *fr = from + edge * 14ull, *tg = to + edge * 14ull;
          double *out = states + edge * (unsigned long long)max_states * 14ull;
          double acc = 0.0; // RealVectorStateSpace::distance(from, to): serial sum in the canonical order, every lane for itself
#pragma unroll
          for (int i = 0; i < 14; i++) {
            const double diff = fr[i] - tg[i];
            acc = CCMP_FMA(diff, diff, acc);
          }
          const double dist = ccmp_sqrt(acc);
          const double total = 0.0, maxd = dist * lambda;
          // target_ok (checkMotion, src/planner/stefanBiPRM.cpp:397-398): isSatisfied(to) of every edge, tested by a launch in front of
          // this one — an edge whose target fails is not traversed (n = 1, ok = 0), as in geodesic_flat_kernel
          const bool tgt = target_ok == nullptr || target_ok[edge] != 0;
          const bool enter = tgt && dist > delta; // (continuations — carry_in — are few edges and stay on geodesic_flat_kernel)
          const double tt = delta / dist;
          for (int e = lane_opaque(r); e < 14; e += kGroup) {
            const double a = fr[e];
            rec[kGPrev + e] = a;
            if (max_states > 0) out[e] = a; // geodesic->push_back(cloneState(from))
            if (enter) rec[kX + e] = geo_interpolate(a, tg[e], tt);
          }
          if (r == 0) {
            rec[kGDist] = dist;
            rec[kGDist + 1] = total;
            rec[kGDist + 2] = maxd;
            int *cnt = reinterpret_cast<int *>(rec + kGCnt);
            cnt[0] = 1; cnt[1] = 0; cnt[2] = 0; // states listed, Newton updates, Newton rounds of this call
          }
          if (enter) {
            active = true; iter = 0; updates = 0; norm1 = 0.0; norm2 = 0.0;
          } else if (r == 0) { // within delta already (or a continuation that has arrived): nothing to traverse
            n_states[edge] = 1;
            ok_out[edge] = (uint8_t)(tgt && dist <= delta);
            if (newton_iters) newton_iters[edge] = 0;
            if (carry_out) { carry_out[2ull * edge] = total; carry_out[2ull * edge + 1ull] = maxd; }
            if (pool) atomicAdd(queue + 3, 1ull); // finished edges: what the hand-over rule below counts down from
          }
        } else drained = true;
      }
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) {
      if (__builtin_amdgcn_ballot_w64(live && !drained) == 0ull) break; // nothing in flight and the queue is empty
      continue;                                                          // edges that needed no traversal: take the next tickets
    }
    __syncthreads();
    // ---- hand-over (as project_fd_kernel's): once the ticket queue is dry and the edges still in flight — E minus the finished
    // count in queue[3], which starts at the front's length — no longer fill handover_pct % of this launch's group slots, every
    // wavefront dumps its live edges at the loop top — iterate, previous state, running distances, counters: the next thing that
    // happens to them is function(x) + the loop test, where geodesic_flat_kernel's Newton routine starts — and retires; latency
    // blocks launched behind this kernel finish them.  A wavefront whose ten edges are of similar predicted length empties all at
    // once; what is left near the end are stragglers on mostly idle wavefronts, at a twelfth of the latency kernel's pace.
    if (pool != nullptr) {
      unsigned long long head = 0, fin_count = 0;
      if (lane == 0) {
        head = __hip_atomic_load(queue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fin_count = __hip_atomic_load(queue + 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      head = shfl_u64(head, 0);
      fin_count = shfl_u64(fin_count, 0);
      const unsigned long long in_flight = E - fin_count, slots = (unsigned long long)gridDim.x * kGroupsPerWave;
      if (head >= E && in_flight * 100ull < slots * (unsigned long long)handover_pct) {
        const unsigned long long m = __builtin_amdgcn_ballot_w64(active && r == 0);
        unsigned long long base = 0;
        if (lane == 0 && m) base = atomicAdd(pool_count, (unsigned long long)__builtin_popcountll(m));
        base = shfl_u64(base, 0);
        if (active) {
          double *ent = pool + (base + (unsigned long long)__builtin_popcountll(m & ((1ull << lane_opaque(leader)) - 1ull))) * (unsigned long long)kGeoPoolEntry;
          for (int e = lane_opaque(r); e < 14; e += kGroup) { ent[e] = rec[kX + e]; ent[14 + e] = rec[kGPrev + e]; }
          if (r == 0) {
            const int *cnt = reinterpret_cast<const int *>(rec + kGCnt);
            ent[28] = rec[kGDist]; ent[29] = rec[kGDist + 1]; ent[30] = rec[kGDist + 2];
            ent[31] = __longlong_as_double((long long)edge);
            ent[32] = __hiloint2double(cnt[0], cnt[1]);   // states listed, Newton updates of the finished projections
            ent[33] = __hiloint2double(cnt[2], iter);     // Newton rounds of the finished projections, loop counter of this one
            ent[34] = __hiloint2double(0, updates);
            ent[35] = norm1; ent[36] = norm2;
          }
        }
        break;
      }
    }

#define CCMP_FD_BP lane_bp[lane_opaque(lane)]
#define CCMP_FD_X0_ROWS 0
#include "ccmp_fd_newton_phase1.inc"
    // ---- a projection has ended: the reference's bookkeeping between two projections (jy_ProjectedStateSpace.cpp:65-90) --
    {
      const bool fin = active && !cont;
      bool bad = false;
      if (fin) {
#pragma unroll
        for (int e = 0; e < 14; e++) {
          if (e % kGroup == r) {
            const double v = rec[kX + e];
            if (v < K.lbe[e % 7]) bad = true;
            if (v > K.ube[e % 7]) bad = true;
          }
        }
      }
      const unsigned long long badmask = __builtin_amdgcn_ballot_w64(bad);
      if (fin) {
        const bool jv = ((badmask >> leader) & 0x3Full) == 0ull;         // jointValid(x)
        const bool conv = (norm1 < K.tol_pos) && (norm2 < K.tol_rot);     // project's return test
        int *cnt = reinterpret_cast<int *>(rec + kGCnt);
        int n = cnt[0], its = cnt[1] + updates;
        const int rounds = cnt[2] + updates + 1;
        double dist = rec[kGDist], total = rec[kGDist + 1];
        const double maxd = rec[kGDist + 2];
        const double *tg = to + edge * 14ull;
        double *out = states + edge * (unsigned long long)max_states * 14ull;
        double s_acc = 0.0, d_acc = 0.0; // distance(previous, scratch), distance(scratch, to): two serial sums side by side
#pragma unroll
        for (int i = 0; i < 14; i++) {
          const double xi = rec[kX + i];
          const double ds = rec[kGPrev + i] - xi, dd = xi - tg[i];
          s_acc = CCMP_FMA(ds, ds, s_acc);
          d_acc = CCMP_FMA(dd, dd, d_acc);
        }
        bool done = true, fits = true, suspended = false;
        do {
          if (!(conv && jv)) break;                        // not on manifold
          const double step = ccmp_sqrt(s_acc), newDist = ccmp_sqrt(d_acc);
          double delta_o = delta; // (opaque: the product below is otherwise formed once, in front of the loop, and parked in scratch)
          asm volatile("" : "+v"(delta_o));
          if (step > lambda * delta_o) break;              // deviated
          const double total_before = total;
          total += step;
          if (total > maxd) break;                         // wandered too far
          if (newDist >= dist) break;                      // no closer than before
          if (n >= max_states) { fits = false; n = max_states + 1; total = total_before; its -= updates; break; } // list full
          dist = newDist;
          for (int e = lane_opaque(r); e < 14; e += kGroup) out[(unsigned long long)n * 14ull + e] = rec[kX + e];
          n++;
          if (!(dist >= delta)) break;                     // arrived
          if (round_budget > 0 && rounds >= round_budget) { suspended = true; break; } // this call's share of the edge is spent
          done = false;
        } while (0);
        if (done) {
          if (r == 0) {
            n_states[edge] = n;
            ok_out[edge] = suspended ? (uint8_t)2 : (uint8_t)(fits && dist <= delta);
            if (newton_iters) newton_iters[edge] = its;
            if (carry_out) { carry_out[2ull * edge] = total; carry_out[2ull * edge + 1ull] = maxd; }
            if (pool) atomicAdd(queue + 3, 1ull);
          }
          active = false;
        } else { // the accepted state becomes `previous`; the next scratch state is interpolated towards the target
          const double tt = delta / dist;
          for (int e = lane_opaque(r); e < 14; e += kGroup) {
            const double a = rec[kX + e];
            rec[kGPrev + e] = a;
            rec[kX + e] = geo_interpolate(a, tg[e], tt);
          }
          if (r == 0) {
            cnt[0] = n; cnt[1] = its; cnt[2] = rounds;
            rec[kGDist] = dist;
            rec[kGDist + 1] = total;
          }
          iter = 0; updates = 0; norm1 = 0.0; norm2 = 0.0;
        }
      }
    }
    if (__builtin_amdgcn_ballot_w64(cont) == 0ull) continue; // nobody iterates: back to the top (refill, next function(x))
    __syncthreads();

#include "ccmp_fd_newton_phase2.inc"
#undef CCMP_FD_BP
#undef CCMP_FD_X0_ROWS
  }
}


// Workspace words (queue heads, counters, the scout's histogram) are cleared by a kernel, not by hipMemsetAsync: a kernel
// node is what a stream capture records and every replay of the graph executes (with hipMemsetAsync the first replay of a
// captured call worked and every later one found the queues exhausted and the histogram still full).
__global__ void clear_words_kernel(unsigned int *__restrict__ w, unsigned int n)
{
  const unsigned int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) w[i] = 0u;
}

// ---- simple per-lane kernels (one sample per lane; all bit-identical to the oracle) -------------
// publish the completion word of a single-state call behind its result (pinned host memory, polled by the host)
__device__ __forceinline__ void publish_done(unsigned int *done_flag, unsigned int done_seq)
{
  if (done_flag != nullptr) {
    __threadfence_system();
    __hip_atomic_store(done_flag, done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(64) void function_kernel(const ccmp_consts K, const double *__restrict__ q, double *__restrict__ f, size_t B,
                                                      unsigned int *done_flag, unsigned int done_seq)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double x[14], out[2];
#pragma unroll
  for (int e = 0; e < 14; e++) x[e] = q[i * 14 + e];
  residual(K, x, out);
  f[2 * i] = out[0];
  f[2 * i + 1] = out[1];
  publish_done(done_flag, done_seq);
}

// KinematicChainConstraint::isSatisfied (ConstraintFunction.h:114-120)
__global__ __launch_bounds__(64) void is_satisfied_kernel(const ccmp_consts K, const double *__restrict__ q, uint8_t *__restrict__ ok, size_t B,
                                                          unsigned int *done_flag, unsigned int done_seq)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double x[14], f[2];
#pragma unroll
  for (int e = 0; e < 14; e++) x[e] = q[i * 14 + e];
  residual(K, x, f);
  const bool finite = (f[0] - f[0] == 0.0) && (f[1] - f[1] == 0.0);
  ok[i] = (uint8_t)(finite && f[0] <= K.tol_pos && f[1] <= K.tol_rot);
  publish_done(done_flag, done_seq);
}

// KinematicChainConstraint::jointValid (ConstraintFunction.h:43-55)
__global__ void joint_valid_kernel(const ccmp_consts K, const double *__restrict__ q, uint8_t *__restrict__ ok, size_t B,
                                   unsigned int *done_flag, unsigned int done_seq)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  bool good = true;
  for (int e = 0; e < 14; e++) {
    const double v = q[i * 14 + e];
    const int jj = e < 7 ? e : e - 7;
    if (v < K.lbe[jj]) good = false;
    if (v > K.ube[jj]) good = false;
  }
  ok[i] = (uint8_t)good;
  publish_done(done_flag, done_seq);
}

__global__ void ambient_uniform_kernel(const ccmp_consts K, unsigned long long seed, unsigned long long first,
                                       double *__restrict__ q, size_t n /* = 14*B */)
{
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  q[t] = ambient_uniform(K, seed, first + t / 14, (int)(t % 14));
}

// sampleUniformNear / sampleGaussian ambient samples; `ref` holds one state per sample (stride 14) or a
// single state shared by all (stride 0)
__global__ void ambient_near_kernel(const ccmp_consts K, unsigned long long seed, unsigned long long first,
                                    const double *__restrict__ ref, int ref_stride, double dist, double *__restrict__ q, size_t n)
{
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t i = t / 14;
  const int j = (int)(t % 14);
  q[t] = ambient_near(K, seed, first + i, j, ref[i * (size_t)ref_stride + j], dist);
}
__global__ void ambient_gaussian_kernel(const ccmp_consts K, unsigned long long seed, unsigned long long first,
                                        const double *__restrict__ ref, int ref_stride, double stddev, double *__restrict__ q,
                                        size_t n)
{
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const size_t i = t / 14;
  const int j = (int)(t % 14);
  q[t] = ambient_gaussian(K, seed, first + i, j, ref[i * (size_t)ref_stride + j], stddev);
}

// IKTask::compute_t_wo (src/base/constraints/ik_task.cpp:10-14): object pose from the left arm's joints,
// t_wb * FK(q) * t_o7.inverse(); out[i] = R (9, row-major) then p (3)
__global__ __launch_bounds__(64) void t_wo_kernel(const ccmp_consts K, const double *__restrict__ q, int q_stride, double *__restrict__ out, size_t B)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double x[7], Rw[9], pw[3], R[9], p[3];
#pragma unroll
  for (int e = 0; e < 7; e++) x[e] = q[i * (size_t)q_stride + e];
  fk_arm(K, 0, x, Rw, pw);
  mul33(Rw, K.t_o7i_R, R);
  p[0] = pw[0]; p[1] = pw[1]; p[2] = pw[2];
  mulvec_acc(Rw, K.t_o7i_p, p);
#pragma unroll
  for (int k = 0; k < 9; k++) out[i * 12 + k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) out[i * 12 + 9 + k] = p[k];
}

__global__ void enforce_bounds_kernel(double *__restrict__ q, size_t n)
{
  size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  q[t] = wrap_pi(q[t]);
}

// Stable stream compaction of valid rows: block-local scan + one atomic per block would reorder
// blocks, so this is the ordered two-pass form: (1) per-block counts, (2) single-block exclusive
// scan of the counts, (3) scatter.  B/256 counts fit one block's loop comfortably (1024 at 262144).
__global__ void compact_count_kernel(const uint8_t *__restrict__ ok, size_t B, unsigned int *__restrict__ block_counts)
{
  __shared__ unsigned int wsum[4];
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool v = i < B && ok[i] != 0;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(v);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = (unsigned)__builtin_popcountll(m);
  __syncthreads();
  if (threadIdx.x == 0) block_counts[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}
__global__ void compact_scan_kernel(unsigned int *__restrict__ block_counts, size_t nblocks,
                                    unsigned long long *__restrict__ total)
{
  // one 1024-thread block; each thread owns a contiguous chunk
  __shared__ unsigned long long part[1024];
  const size_t per = (nblocks + 1023) / 1024;
  const size_t lo = (size_t)threadIdx.x * per, hi = lo + per < nblocks ? lo + per : nblocks;
  unsigned long long s = 0;
  for (size_t k = lo; k < hi; k++) s += block_counts[k];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long run = 0;
    for (int k = 0; k < 1024; k++) { unsigned long long v = part[k]; part[k] = run; run += v; }
    *total = run;
  }
  __syncthreads();
  unsigned long long run = part[threadIdx.x];
  for (size_t k = lo; k < hi; k++) { unsigned int v = block_counts[k]; block_counts[k] = (unsigned int)run; run += v; }
}
__global__ void compact_scatter_kernel(const double *__restrict__ q, const uint8_t *__restrict__ ok, size_t B,
                                       const unsigned int *__restrict__ block_offsets, double *__restrict__ out,
                                       size_t capacity)
{
  __shared__ unsigned int wsum[4];
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool v = i < B && ok[i] != 0;
  const unsigned long long m = __builtin_amdgcn_ballot_w64(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) wsum[w] = (unsigned)__builtin_popcountll(m);
  __syncthreads();
  unsigned int base = block_offsets[blockIdx.x];
  for (int k = 0; k < w; k++) base += wsum[k];
  if (v) {
    const unsigned int pos = base + (unsigned)__builtin_popcountll(m & ((1ull << lane) - 1ull));
    if (pos < capacity) { // rows past the capacity of `out` are dropped; the total still counts them
#pragma unroll
      for (int e = 0; e < 14; e++) out[(size_t)pos * 14 + e] = q[i * 14 + e];
    }
  }
}

} // namespace

// ---- launchers (ccmp_launch.h) ---------------------------------------------------------------------------------------------
namespace ccmp_launch {

// the extend step's short edges on the throughput layout (geodesic_group_kernel): one-wavefront workgroups, ten edges each
hipError_t geodesic_group(const GeoCall &g, int blocks, unsigned long long *queue, const unsigned int *order, double *pool,
                          unsigned long long *pool_count, int handover_pct, const uint8_t *target_ok, hipStream_t st)
{
  if (g.K->stock && g.K->twin_arms) // the STOCK instantiation also assumes twin arms on diag(+-1) base frames (chain_rows), like project_fd_kernel's
    hipLaunchKernelGGL(geodesic_group_kernel<true>, dim3(blocks), dim3(64), 0, st, *g.K, g.delta, g.lambda, g.from, g.to, (unsigned long long)g.E,
                       g.max_states, g.states, g.n_states, g.ok, g.newton_iters, queue, order, g.carry_out, g.round_budget, pool, pool_count, handover_pct, target_ok);
  else
    hipLaunchKernelGGL(geodesic_group_kernel<false>, dim3(blocks), dim3(64), 0, st, *g.K, g.delta, g.lambda, g.from, g.to, (unsigned long long)g.E,
                       g.max_states, g.states, g.n_states, g.ok, g.newton_iters, queue, order, g.carry_out, g.round_budget, pool, pool_count, handover_pct, target_ok);
  return hipGetLastError();
}

hipError_t clear_words(void *words, size_t n_u32, hipStream_t st)
{
  hipLaunchKernelGGL(clear_words_kernel, dim3((unsigned)((n_u32 + 255) / 256)), dim3(256), 0, st, (unsigned int *)words, (unsigned int)n_u32);
  return hipGetLastError();
}

// queue: the projector's block of queue words (kQTicket: this kernel's samples, kQPool: the pool's fill count)
// part: the whole call (the default), or one of the two launches of a large batch — a head launch is one one-wavefront workgroup
// per ten samples: `blocks` must say so; state: the call's B rows between head and resume, kStagedRow doubles each (general instantiations: kPoolEntry)
hipError_t project_group(const ProjectCall &c, int blocks, unsigned long long *queue, double *pool, int dump_threshold,
                         const unsigned int *order, const uint16_t *pred, int long_remaining, size_t pool_records, hipStream_t st,
                         FdPart part, double *state, int head_rounds)
{
  if (part != kFdWhole && (state == nullptr || head_rounds <= 0)) return hipErrorInvalidValue;
  if (blocks <= 0 || (part == kFdHead && (size_t)blocks != (c.B + kGroupsPerWave - 1) / kGroupsPerWave)) return hipErrorInvalidValue;
#define CCMP_LAUNCH_GROUP(VARIANT, STOCK)                                                                                                    \
  hipLaunchKernelGGL((project_fd_kernel<VARIANT, STOCK>), dim3(blocks), dim3(64), 0, st, *c.K, c.q_in, c.q_out, c.ok, c.iters, c.q_ambient, \
                     (unsigned long long)c.B, queue + kQTicket, c.seed, c.first, pool, queue + kQPool, dump_threshold, order, pred,          \
                     long_remaining, (unsigned long long)pool_records, state, head_rounds)
#define CCMP_LAUNCH_PART(MODE, STOCK)                                              \
  do {                                                                             \
    if (part == kFdHead) CCMP_LAUNCH_GROUP(MODE + 2 * kFdHead, STOCK);             \
    else if (part == kFdResume) CCMP_LAUNCH_GROUP(MODE + 2 * kFdResume, STOCK);    \
    else CCMP_LAUNCH_GROUP(MODE, STOCK);                                           \
  } while (0)
  if (c.mode == 0) {
    if (c.K->stock && c.K->twin_arms) CCMP_LAUNCH_PART(0, true);
    else CCMP_LAUNCH_PART(0, false);
  } else {
    if (!(c.K->stock && c.K->twin_arms)) return hipErrorInvalidValue; // the fused sampler exists for the stock structure only (ccmp_api.cpp: project_common)
    CCMP_LAUNCH_PART(1, true);
  }
#undef CCMP_LAUNCH_PART
#undef CCMP_LAUNCH_GROUP
  return hipGetLastError();
}

// done_flag (nullable) is honoured for B == 1 only: the single working thread publishes done_seq behind its result
hipError_t function(const ccmp_consts *K, const double *q, double *f, size_t B, unsigned int *done_flag, unsigned int done_seq, hipStream_t st)
{
  if (B != 1) done_flag = nullptr;
  hipLaunchKernelGGL(function_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, *K, q, f, B, done_flag, done_seq);
  return hipGetLastError();
}
hipError_t is_satisfied(const ccmp_consts *K, const double *q, uint8_t *ok, size_t B, unsigned int *done_flag, unsigned int done_seq,
                        hipStream_t st)
{
  if (B != 1) done_flag = nullptr;
  hipLaunchKernelGGL(is_satisfied_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, *K, q, ok, B, done_flag, done_seq);
  return hipGetLastError();
}
hipError_t joint_valid(const ccmp_consts *K, const double *q, uint8_t *ok, size_t B, unsigned int *done_flag, unsigned int done_seq,
                       hipStream_t st)
{
  if (B != 1) done_flag = nullptr;
  hipLaunchKernelGGL(joint_valid_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, *K, q, ok, B, done_flag, done_seq);
  return hipGetLastError();
}
hipError_t ambient_uniform(const ccmp_consts *K, unsigned long long seed, unsigned long long first, double *q, size_t B, hipStream_t st)
{
  size_t n = B * 14;
  hipLaunchKernelGGL(ambient_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *K, seed, first, q, n);
  return hipGetLastError();
}
hipError_t ambient_ref(const ccmp_consts *K, int kind, unsigned long long seed, unsigned long long first, const double *ref, int ref_stride,
                       double param, double *q, size_t B, hipStream_t st)
{
  size_t n = B * 14;
  if (kind == 0)
    hipLaunchKernelGGL(ambient_near_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *K, seed, first, ref,
                       ref_stride, param, q, n);
  else
    hipLaunchKernelGGL(ambient_gaussian_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, *K, seed, first, ref,
                       ref_stride, param, q, n);
  return hipGetLastError();
}
hipError_t t_wo(const ccmp_consts *K, const double *q, int q_stride, double *out, size_t B, hipStream_t st)
{
  hipLaunchKernelGGL(t_wo_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, *K, q, q_stride, out, B);
  return hipGetLastError();
}
hipError_t enforce_bounds(double *q, size_t B, hipStream_t st)
{
  size_t n = B * 14;
  hipLaunchKernelGGL(enforce_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, n);
  return hipGetLastError();
}
hipError_t compact(const double *q, const uint8_t *ok, size_t B, double *out, size_t capacity, unsigned int *block_counts,
                   unsigned long long *total, hipStream_t st)
{
  const size_t nblocks = (B + 255) / 256;
  hipLaunchKernelGGL(compact_count_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, ok, B, block_counts);
  hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, st, block_counts, nblocks, total);
  hipLaunchKernelGGL(compact_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, st, q, ok, B, block_counts, out, capacity);
  return hipGetLastError();
}

}  // namespace ccmp_launch
