// ccmp_kernels_fast.hip — analytic-Jacobian projector for gfx950 (jacobian_mode = CCMP_JAC_ANALYTIC).
//
// Same Newton iteration, stopping rule and quirks as KinematicChainConstraint::project
// (include/closed_chain_motion_planner/base/constraints/ConstraintFunction.h:57-82), but the 2x14 Jacobian is the exact
// derivative of the residual — G(2x6) times the 6x14 closed-loop geometric Jacobian, whose single-arm half the reference
// itself carries as PandaModel::getJacobianMatrix (src/kinematics/panda_rbdl.cpp:9-22, never called there) — instead of
// OMPL's 84-evaluation finite-difference stencil, and the step is SURVEY.md §7.3's x -= 0.30 J^T (J J^T)^-1 f on the 2x2
// Gram matrix (the SVD-equivalent routine of the reference arithmetic only where the two rows are nearly parallel).
// Built in the canonical rounding model (-ffp-contract=off -DCCMP_USE_FMA): bit-identical to the CPU oracle run with
// ORC_JAC_ANALYTIC (oracle/ccmp_oracle.c: orc_jacobian_analytic + orc_solve_gram restate this file's operation order),
// which is how the mode is verified.  NOT bit-comparable with the REFERENCE arithmetic: the reference iteration amplifies
// 1e-8 Jacobian differences along the trajectory, so this mode lands on a different point of the same
// manifold for ~20 % of uniform samples.  Opt-in; the default mode is the FD-faithful kernel in ccmp_kernels_fd.hip.
//
// Layout (round 6): ONE SAMPLE PER LANE PAIR, 32 samples per wavefront.  The even lane carries arm 0, the odd lane arm 1:
// each runs its own 7-joint chain (sines, cosines, frames, joint axes z_i and origins o_i in the arm's base frame) and its
// seven Jacobian columns; the two tool poses cross inside the pair by DPP quad_perm broadcasts, the three Gram sums by a
// quad_perm swap.  Half the per-lane state of a one-sample-per-lane layout (round 5: 256 VGPRs + 198 AGPRs of spill
// space, one wavefront per SIMD, 34 % VALU issue): 142 registers, three wavefronts per SIMD, no scratch, no AGPR traffic.
// Lanes whose sample is done are refilled from ticket queues while their neighbours keep iterating (iteration counts
// spread 15..250); when the queues are dry a wavefront that is mostly empty hands its live samples over (x, index,
// counters, at the loop top) to a pool that the LATENCY kernel below — sixteen lanes per sample, 2.7 us per Newton round
// where this layout needs 4 — finishes; that kernel also takes small batches alone.  The extend step in this mode is a traversal
// kernel on the latency kernel's layout and Newton round (geodesic_row16_kernel, end of the file): one launch per call, four edges
// per wavefront, the round budget, carry-in / carry-out and isSatisfied(to) inside.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ccmp_fd_common.h"
#include "ccmp_kin.h"
#include "ccmp_launch.h"
#include "ccmp_resident.h" // the resident service kernel for analytic mode, at the end of the file
#include "ccmp_solve.h"

using namespace ccmp;
using ccmp_launch::kFastQueues; // ticket words of the lane-pair kernel
using ccmp_launch::kPoolEntry;  // hand-over record
#include "ccmp_clearance.h"         // the scene variant of the extend step (the others do not use it)

namespace {

constexpr int kConstsDoubles = (int)((sizeof(ccmp_consts) + 7) / 8);

// value of the pair's even (arm 0) / odd (arm 1) lane in both lanes; the partner's value
__device__ __forceinline__ double pair_even(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0xA0 /* quad_perm:[0,0,2,2] */, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, 0xA0, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double pair_odd(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0xF5 /* quad_perm:[1,1,3,3] */, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, 0xF5, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double pair_swap(double v)
{
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_mov_dpp(lo, 0xB1 /* quad_perm:[1,0,3,2] */, 0xf, 0xf, false);
  hi = __builtin_amdgcn_mov_dpp(hi, 0xB1, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// A value the optimiser cannot see through: what is derived from it inside the Newton loop is recomputed where it is used
// instead of being hoisted in front of the loop and held (or spilled) across it.
__device__ __forceinline__ int opaque(int v)
{
  asm volatile("" : "+v"(v));
  return v;
}
// KinematicChainSpace::enforceBounds (ccmp_kin.h: wrap_pi): fmod(q, 2 pi) is q itself when |q| < 2 pi — where a Newton
// iterate practically always is — and the library call's ~120 instructions run only for the lanes beyond (same bits).
__device__ __forceinline__ double wrap_pi_near(double q)
{
  const double pi = 3.14159265358979323846;
  double v = q;
  if (!(ccmp_abs(q) < 2.0 * pi)) v = __builtin_fmod(q, 2.0 * pi);
  if (v < -pi) v += 2.0 * pi;
  else if (v >= pi) v -= 2.0 * pi;
  return v;
}
__device__ __forceinline__ int pair_swap_i(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, false); }

// Forward chain of this lane's arm in the arm's base frame, keeping every joint's axis z_i and origin o_i; joint indices are
// compile-time so that the STOCK instantiation skips the products with the stock Panda's exact zeros (ccmp_kin.h).  `ac` is
// the arm whose constants are read: the lane's own arm, or 0 for twin arms (one LDS address for the whole wavefront).
// The axes go to this lane's column of an LDS array (zs[k * 64], k = 3 i + component: consecutive lanes, consecutive words)
// — 42 more live registers across the chain otherwise; the origins stay in registers (with the stock structure joints 1
// and 5 share the origin of the joint before them, and joint 0's is a constant).
template <bool STOCK, int I>
__device__ __forceinline__ void chain_frames_from(const ccmp_consts &K, const int ac, const double *q, double *zs, double (*oj)[3],
                                                  double *R, double *o)
{
  if constexpr (I < 7) {
    asm volatile("" ::: "memory"); // the joint's constants are read from LDS here, not hoisted out of the Newton loop into registers
    // one joint after the other: the angle is made to depend on the frame the joint before left behind (no instruction
    // is emitted), or all seven sines and cosines are formed up front and the chain is interleaved across joints at
    // a cost of ~150 registers
    double qi = q[I];
    if constexpr (I > 0) asm volatile("" : "+v"(qi) : "v"(R[0]), "v"(R[4]), "v"(R[8]), "v"(o[0]), "v"(o[1]), "v"(o[2]));
    double s, c;
    ccmp_sincos(qi, &s, &c);
    mulvec_acc_nz<STOCK ? kStockOff[I] : 7>(R, K.offset[ac][I], o);
    const double *a = K.axis[ac][I];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      zs[(3 * I + k) * 64] = (STOCK && kStockZ[I]) ? R[3 * k + 2] : dot3(R[3 * k], a[0], R[3 * k + 1], a[1], R[3 * k + 2], a[2]);
      oj[I][k] = o[k];
    }
    double Rn[9];
    chain_rot<I, STOCK>(a, K.aprod[ac][I], s, c, R, Rn);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = Rn[k];
    chain_frames_from<STOCK, I + 1>(K, ac, q, zs, oj, R, o);
  }
}

// Sources: 0 q_in; 1 the ambient sampler (sampleUniform fused, output wrapped).
// STOCK: both arms carry the stock Panda's exact zeros; TWIN: and bit-identical chain constants with diag(+-1) base frames.
template <bool STOCK, bool TWIN>
__global__ __launch_bounds__(64, 3) void project_pair_kernel(const ccmp_consts K_arg, const int srcmode, const double *__restrict__ q_in,
                                                          double *__restrict__ q_out, uint8_t *__restrict__ ok_out,
                                                          uint16_t *__restrict__ iters_out, double *__restrict__ q_ambient,
                                                          unsigned long long B, unsigned long long *queue, unsigned long long seed,
                                                          unsigned long long first_index, double *__restrict__ pool_out,
                                                          unsigned long long *pool_out_count, const int dump_below)
{
  // the constants as an LDS copy read by broadcast: with compile-time joint indices the compiler would otherwise hoist
  // every scalar load of the kernarg copy out of the Newton loop and spill hundreds of SGPRs into VGPR lanes; the compiler
  // barriers in chain_frames_from keep the LDS reads at their joints
  __shared__ double ktab[kConstsDoubles + 1];
  __shared__ double zpark[21 * 64];
  {
    const double *srcp = reinterpret_cast<const double *>(&K_arg);
    for (int k = threadIdx.x; k < kConstsDoubles; k += 64) ktab[k] = srcp[k];
  }
  __syncthreads();
  const ccmp_consts &K = *reinterpret_cast<const ccmp_consts *>(ktab);
  const int src = srcmode & 15;          // where the samples come from
  const bool wrap = (srcmode >> 4) == 1; // the call is a fused sampleUniform: enforceBounds on the way out
  const int lane = threadIdx.x;
  const int arm = lane & 1;
  const int ac = TWIN ? 0 : arm;
  double x[7];
  unsigned long long idx = 0;
  int iter = 0, updates = 0;
  double norm1 = 0.0, norm2 = 0.0;
  bool active = false, drained = false;
  // Work distribution: one atomic per wavefront and refill event takes as many tickets as pairs are free.  kFastQueues
  // ticket words, each owning a contiguous slice of the batch (or of the pool), keep the atomics off a single address — a
  // same-address atomic costs ~12 ns chip-wide on this part (tools/ubench/atomic_rate.hip); a wavefront starts on its own
  // word and moves on to the next ones when that slice is used up.
  const unsigned long long total = B;
  static_assert(kFastQueues == 64, "one ticket word per lane");
  int qk = blockIdx.x % kFastQueues;
  const unsigned long long below_pair = (1ull << (lane & ~1)) - 1ull;
  constexpr unsigned long long kEven = 0x5555555555555555ull;

  for (;;) {
    // ---- hand-over --------------------------------------------------------------------------------------------------
    // When the tickets are used up and at most dump_below pairs of this wavefront still carry a sample, all of them leave and
    // the wavefront retires: the latency kernel launched behind finishes them, four to a wavefront.  State at the loop top:
    // function(x) and the loop test come next.
    if (pool_out != nullptr && drained) {
      const unsigned long long lv = __builtin_amdgcn_ballot_w64(active) & kEven;
      if (lv != 0ull && __builtin_popcountll(lv) <= dump_below) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(pool_out_count, (unsigned long long)__builtin_popcountll(lv));
        base = __shfl(base, 0);
        if (active) {
          const int a7 = 7 * (opaque(lane) & 1);
          double *ent = pool_out + (base + (unsigned long long)__builtin_popcountll(lv & below_pair)) * kPoolEntry + a7;
#pragma unroll
          for (int e = 0; e < 7; e++) ent[e] = x[e];
          if (a7 == 0) {
            ent[14] = __longlong_as_double((long long)idx);
            ent[15] = __hiloint2double(updates, iter);
            ent[16] = norm1;
            ent[17] = norm2;
          }
          active = false;
        }
      }
    }
    // ---- refill -------------------------------------------------------------------------------------------------------
    unsigned long long need = __builtin_amdgcn_ballot_w64(!active && !drained) & kEven;
    while (need != 0ull) {
      const int n = __builtin_popcountll(need);
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(queue + qk, (unsigned long long)n);
      base = __shfl(base, 0); // ticket of the first free pair, relative to the word's share
      const bool mine = (need >> (lane & ~1)) & 1ull;
      const unsigned long long lo = total * (unsigned long long)qk / kFastQueues;
      const unsigned long long hi = total * (unsigned long long)(qk + 1) / kFastQueues;
      const unsigned long long t = lo + base + (unsigned long long)__builtin_popcountll(need & below_pair);
      if (mine && t < hi) {
        active = true;
        const int a7 = 7 * (opaque(lane) & 1);
        idx = t;
        iter = 0; updates = 0; norm1 = 0.0; norm2 = 0.0;
#pragma unroll
        for (int e = 0; e < 7; e++) {
          if (src == 0) x[e] = q_in[idx * 14 + a7 + e];
          else {
            x[e] = ambient_uniform_at(K, seed, first_index + idx, a7 + e, e);
            if (q_ambient) q_ambient[idx * 14 + a7 + e] = x[e];
          }
        }
      }
      need = __builtin_amdgcn_ballot_w64(!active && !drained) & kEven;
      if (need != 0ull) {
        // this slice is used up.  One load brings all kFastQueues (= 64, one per lane) ticket words: go on with the next slice
        // that still has tickets; a word only grows, so when none has any left the batch is handed out for good.  (Trying
        // the words one by one cost every wavefront 64 serial atomic round trips at the end of a launch.)
        const unsigned long long taken = __hip_atomic_load(queue + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned long long lo_l = total * (unsigned long long)lane / kFastQueues, hi_l = total * (unsigned long long)(lane + 1) / kFastQueues;
        const unsigned long long avail = __builtin_amdgcn_ballot_w64(lo_l + taken < hi_l);
        if (avail == 0ull) { drained = true; break; }
        const int r = (qk + 1) & 63;
        const unsigned long long rot = r ? ((avail >> r) | (avail << (64 - r))) : avail;
        qk = (r + __builtin_ctzll(rot)) & 63;
      }
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;

    // ---- function(x): this lane's chain with its joint frames kept for the Jacobian, tool poses crossed in the pair -----
    double oj[7][3], Rw[9], pw[3];
    double *const zs = zpark + lane;
    {
      double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, o[3] = {0, 0, 0};
      chain_frames_from<STOCK, 0>(K, ac, x, zs, oj, R, o);
      asm volatile("" ::: "memory");
      // tool_pose_t with this lane's base frame (ccmp_kin.h): TWIN bases are diag(+-1) — d_r * Rf[r][c] and
      // fma(d_r, pf[r], base_p[r]), to which the general product only adds exact zeros
      double pf[3] = {o[0], o[1], o[2]}, Rf[9];
      mulvec_acc_nz<STOCK ? kStockEe : 7>(R, K.ee[ac], pf);
      mul33(R, K.R_tool[ac], Rf);
      if (TWIN) {
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const double d = K.base_R[arm][4 * r];
#pragma unroll
          for (int c = 0; c < 3; c++) Rw[3 * r + c] = d * Rf[3 * r + c];
          pw[r] = CCMP_FMA(d, pf[r], K.base_p[arm][r]);
        }
      } else {
        mul33(K.base_R[arm], Rf, Rw);
        pw[0] = K.base_p[arm][0]; pw[1] = K.base_p[arm][1]; pw[2] = K.base_p[arm][2];
        mulvec_acc(K.base_R[arm], pf, pw);
      }
    }
    double R1[9], p1[3], R2[9], p2[3];
#pragma unroll
    for (int k = 0; k < 9; k++) { R1[k] = pair_even(Rw[k]); R2[k] = pair_odd(Rw[k]); }
#pragma unroll
    for (int k = 0; k < 3; k++) { p1[k] = pair_even(pw[k]); p2[k] = pair_odd(pw[k]); }
    double f[2], dq[4], pc[3];
    chain_residual(K, R1, p1, R2, p2, f, dq, pc);

    // ---- loop condition of ConstraintFunction.h:68, quirks included (both lanes of a pair decide alike) -------------------
    bool cont = false;
    if (active) {
      const bool c1 = f[0] > K.tol_pos;
      norm1 = c1 ? 1.0 : 0.0;
      bool resid = c1;
      if (!c1) { norm2 = f[1]; resid = f[1] > K.tol_rot; }
      if (resid) { cont = iter < K.max_iter; iter++; }
    }
    {
      const bool fin = active && !cont;
      int good = 1;
      const int a7 = 7 * (opaque(lane) & 1);
      if (fin) {
        double *row = q_out + idx * 14 + a7;
#pragma unroll
        for (int e = 0; e < 7; e++) {
          if (x[e] < K.lbe[e]) good = 0;
          if (x[e] > K.ube[e]) good = 0;
          row[e] = wrap ? wrap_pi_near(x[e]) : x[e];
        }
      }
      good &= pair_swap_i(good);
      if (fin && a7 == 0) {
        ok_out[idx] = (uint8_t)(good && (norm1 < K.tol_pos) && (norm2 < K.tol_rot));
        if (iters_out) iters_out[idx] = (uint16_t)updates;
      }
      if (fin) active = false;
    }
    if (__builtin_amdgcn_ballot_w64(cont) == 0ull) continue;

    // ---- analytic Jacobian, this lane's seven columns ----------------------------------------------------------------------
    // u = dp/|dp| (chain frame), n = axis of R_c R_0^T with w >= 0; both taken to the world frame through R_2, then into
    // this lane's arm base frame through base_R^T (oracle/ccmp_oracle.c: orc_jacobian_analytic).
    double J0[7], J1[7];
    {
      double u[3] = {0, 0, 0}, n[3] = {0, 0, 0};
      if (f[0] > 0.0) {
        const double inv = 1.0 / f[0];
#pragma unroll
        for (int k = 0; k < 3; k++) u[k] = (pc[k] - K.init_p[k]) * inv;
      }
      const double vn = ccmp_sqrt(dot3(dq[0], dq[0], dq[1], dq[1], dq[2], dq[2]));
      if (vn > 0.0) {
        const double sg = (dq[3] < 0.0 ? -1.0 : 1.0) / vn;
#pragma unroll
        for (int k = 0; k < 3; k++) n[k] = dq[k] * sg;
      }
      double aw[3], bw[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        aw[k] = dot3(R2[3 * k], u[0], R2[3 * k + 1], u[1], R2[3 * k + 2], u[2]);
        bw[k] = dot3(R2[3 * k], n[0], R2[3 * k + 1], n[1], R2[3 * k + 2], n[2]);
      }
      double al[3], bl[3], pl[3], dp[3];
#pragma unroll
      for (int k = 0; k < 3; k++) dp[k] = p1[k] - K.base_p[arm][k];
      mulTvec(K.base_R[arm], aw, al);
      mulTvec(K.base_R[arm], bw, bl);
      mulTvec(K.base_R[arm], dp, pl);
      asm volatile("" ::: "memory");
      const double sgn = (opaque(lane) & 1) ? -1.0 : 1.0; // + arm 0, - arm 1
#pragma unroll
      for (int i = 0; i < 7; i++) {
        const double zi[3] = {zs[(3 * i) * 64], zs[(3 * i + 1) * 64], zs[(3 * i + 2) * 64]};
        const double r0 = pl[0] - oj[i][0], r1 = pl[1] - oj[i][1], r2 = pl[2] - oj[i][2];
        const double cx = CCMP_FMA(zi[1], r2, -(zi[2] * r1));
        const double cy = CCMP_FMA(zi[2], r0, -(zi[0] * r2));
        const double cz = CCMP_FMA(zi[0], r1, -(zi[1] * r0));
        J0[i] = sgn * dot3(al[0], cx, al[1], cy, al[2], cz);
        J1[i] = sgn * dot3(bl[0], zi[0], bl[1], zi[1], bl[2], zi[2]);
      }
    }
    // ---- Newton step on the Gram matrix (orc_solve_gram): per-arm partial sums, added across the pair ---------------------
    double dx[7];
    {
      double pa = 0.0, pd = 0.0, pb = 0.0;
#pragma unroll
      for (int j = 0; j < 7; j++) {
        pa = CCMP_FMA(J0[j], J0[j], pa);
        pd = CCMP_FMA(J1[j], J1[j], pd);
        pb = CCMP_FMA(J0[j], J1[j], pb);
      }
      // arm 0's sum + arm 1's sum: IEEE addition commutes, both lanes hold the same bits
      const double a = pa + pair_swap(pa), d = pd + pair_swap(pd), b = pb + pair_swap(pb);
      double y0, y1;
      const bool well = gram_coeffs(a, d, b, f[0], f[1], y0, y1);
#pragma unroll
      for (int j = 0; j < 7; j++) dx[j] = CCMP_FMA(y1, J1[j], y0 * J0[j]);
      if (__builtin_amdgcn_ballot_w64(cont && !well) != 0ull) {
        // nearly parallel rows (or a NaN): the reference arithmetic's SVD-equivalent solve on the full rows, both lanes alike
        double Jf[28], dxf[14];
#pragma unroll
        for (int j = 0; j < 7; j++) {
          Jf[j] = pair_even(J0[j]); Jf[7 + j] = pair_odd(J0[j]);
          Jf[14 + j] = pair_even(J1[j]); Jf[21 + j] = pair_odd(J1[j]);
        }
        solve_minnorm(Jf, f[0], f[1], dxf);
        if (!well) {
#pragma unroll
          for (int j = 0; j < 7; j++) dx[j] = (opaque(lane) & 1) ? dxf[7 + j] : dxf[j];
        }
      }
    }
    if (cont) {
#pragma unroll
      for (int e = 0; e < 7; e++) x[e] = CCMP_FMA(-K.step, dx[e], x[e]);
      updates++;
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------
// project_row16_kernel — the analytic mode's LATENCY kernel: sixteen lanes (one DPP row) per sample, four samples per
// wavefront, one wavefront per block.  A wavefront that has its SIMD to itself pays ~4.6 cycles for ANY instruction
// (tools/ubench/), so a Newton round of the lane-pair kernel (~2 100 instructions) lasts ~5 us however few samples are
// left — 250 rounds of a sample that never converges: 1.2 ms.  Here a round is ~900 instructions on the critical path:
//   lane l < 14 owns joint l (arm l / 7): its angle, sine / cosine and joint rotation (rot_sc), its Jacobian column,
//               its component of the Newton step — the joint's constants stay in the lane's registers;
//   lane l < 6 also carries row l % 3 of arm l / 3's chain frame: per joint one row of R * Rot, its component of the
//               joint's axis z_i = R axis_i and of the joint's origin (the decomposition of the reference-arithmetic
//               throughput kernel's phase 1, ccmp_kernels_fd.hip), then one row of the tool pose;
//   all lanes   the residual, the probe vectors and the 2x2 Gram step (every lane needs their results).
// Joint rotations, axes / origins, the two tool poses and the Jacobian pass through the sample's LDS record; with one
// wavefront per block the LDS queue orders writes and reads, no barrier is needed.  Every value is produced by the same
// operations on the same operands as in the lane-pair kernel and in the oracle (general formulas: what the STOCK
// instantiations skip are products with exact zeros): bit-identical.  DIAG: both base frames are diag(+-1) (every shipped
// t_wb); otherwise the base-frame product is formed from the whole hand poses by every lane.
// Sources: 0 q_in, 1 ambient sampler, 2 the hand-over pool of the lane-pair kernel launched in front.
constexpr int qRJ = 0, qZO = 126, qT = 210, qJ = 234, qDX = 262, qRec = 277; // doubles per sample: Rot[14][9], (z, o)[14][6], poses[2][12], J[28], fallback dx[14]; odd stride

template <bool DIAG>
__global__ __launch_bounds__(64, 2) void project_row16_kernel(const ccmp_consts K_arg, const int srcmode, const double *__restrict__ q_in,
                                                              double *__restrict__ q_out, uint8_t *__restrict__ ok_out,
                                                              uint16_t *__restrict__ iters_out, double *__restrict__ q_ambient,
                                                              unsigned long long B, unsigned long long *queue, unsigned long long seed,
                                                              unsigned long long first_index, const double *__restrict__ pool_in,
                                                              const unsigned long long *__restrict__ pool_in_count)
{
  __shared__ double ktab[kConstsDoubles + 1];
  __shared__ double lds[4 * qRec];
  {
    const double *srcp = reinterpret_cast<const double *>(&K_arg);
    for (int k = threadIdx.x; k < kConstsDoubles; k += 64) ktab[k] = srcp[k];
  }
  __syncthreads();
  const ccmp_consts &K = *reinterpret_cast<const ccmp_consts *>(ktab);
  const int src = srcmode & 15;
  const bool wrap = (srcmode >> 4) == 1;
  const int lane = threadIdx.x, l = lane & 15;
  double *const rec = lds + (lane >> 4) * qRec;
  // joint role (lanes 14, 15 shadow joint 13 and never store)
  const bool jl = l < 14;
  const int lj = jl ? l : 13;
  const int aj = lj >= 7 ? 1 : 0, ij = lj - 7 * aj;
  double ax[3], ap[6];
#pragma unroll
  for (int k = 0; k < 3; k++) ax[k] = K.axis[aj][ij][k];
#pragma unroll
  for (int k = 0; k < 6; k++) ap[k] = K.aprod[aj][ij][k];
  const double lbe = K.lbe[ij], ube = K.ube[ij];
  const double sgn = aj ? -1.0 : 1.0;
  // chain role: lanes 6..15 shadow the rows of lanes 0..5 — the same operands, the same results, stored to the same words
  const int ac = (l / 3) & 1, rc = l % 3;
  double cee[3], cRt[9]; // this lane's arm: loop-invariant, kept in registers
#pragma unroll
  for (int k = 0; k < 3; k++) cee[k] = K.ee[ac][k];
#pragma unroll
  for (int k = 0; k < 9; k++) cRt[k] = K.R_tool[ac][k];
  const double cd = K.base_R[ac][4 * rc], cbp = K.base_p[ac][rc];
  const unsigned long long total = src == 2 ? *pool_in_count : B;

  double x = 0.0;
  unsigned long long idx = 0;
  int iter = 0, updates = 0;
  double norm1 = 0.0, norm2 = 0.0;
  bool active = false, drained = false;

  for (;;) {
    // ---- refill: rows without a sample take the next ticket ------------------------------------------------------------
    {
      const bool want = !active && !drained;
      unsigned long long t = 0;
      if (want && l == 0) t = atomicAdd(queue, 1ull);
      t = __shfl(t, lane & ~15);
      if (want) {
        if (t < total) {
          active = true;
          if (src == 2) {
            const double *ent = pool_in + t * kPoolEntry;
            idx = (unsigned long long)__double_as_longlong(ent[14]);
            iter = __double2hiint(ent[15]);
            updates = __double2loint(ent[15]);
            norm1 = ent[16];
            norm2 = ent[17];
            x = ent[lj];
          } else {
            idx = t;
            iter = 0; updates = 0; norm1 = 0.0; norm2 = 0.0;
            if (src == 0) x = q_in[idx * 14 + lj];
            else {
              x = ambient_uniform_at(K, seed, first_index + idx, lj, ij);
              if (q_ambient && jl) q_ambient[idx * 14 + lj] = x;
            }
          }
        } else drained = true;
      }
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;

#include "ccmp_row16_eval.inc"
    bool cont = false;
    if (active) { // ConstraintFunction.h:68, quirks included; the sixteen lanes of a row decide alike
      const bool c1 = f[0] > K.tol_pos;
      norm1 = c1 ? 1.0 : 0.0;
      bool resid = c1;
      if (!c1) { norm2 = f[1]; resid = f[1] > K.tol_rot; }
      if (resid) { cont = iter < K.max_iter; iter++; }
    }
    {
      const bool fin = active && !cont;
      bool bad = false;
      if (fin && jl) {
        if (x < lbe) bad = true;
        if (x > ube) bad = true;
        q_out[idx * 14 + lj] = wrap ? wrap_pi_near(x) : x;
      }
      const unsigned long long badmask = __builtin_amdgcn_ballot_w64(bad);
      if (fin && l == 0) {
        const bool rbad = ((badmask >> (lane & ~15)) & 0xFFFFull) != 0ull;
        ok_out[idx] = (uint8_t)((!rbad) && (norm1 < K.tol_pos) && (norm2 < K.tol_rot));
        if (iters_out) iters_out[idx] = (uint16_t)updates;
      }
      if (fin) active = false;
    }
    if (__builtin_amdgcn_ballot_w64(cont) == 0ull) continue;
#include "ccmp_row16_step.inc"
  }
}


// ------------------------------------------------------------------------------------------------------------------------
// The extend step in analytic mode: jy_ProjectedStateSpace::discreteGeodesic (src/base/jy_ProjectedStateSpace.cpp:32-96) as a
// TRAVERSAL KERNEL on the latency kernel's layout — sixteen lanes (one DPP row) per edge, four edges per wavefront, one wavefront
// per block, persistent wavefronts that take edges from a ticket word; the rows of a wavefront run independently, driven by
// ballots.  Per edge exactly the order of ccmp_geo_edge_body.inc and oracle/ccmp_oracle.c: orc_discrete_geodesic_ex with
// interpolate = true (the host truncates the list at the first state its StateValidityChecker rejects): `from` as row 0,
// isSatisfied(to) with check_target (one function evaluation), the entry test, then per state the interpolation (lane l < 14:
// joint l), the projection (the Newton round of project_row16_kernel, ccmp_row16_eval.inc / ccmp_row16_step.inc: the same bits),
// jointValid, step and newDist as serial sums over the row's LDS record, the four break tests, the list-full rule, the round
// budget (ok = 2 between two states), carry_in / carry_out.  An edge that has ended does no further work: its row takes the next
// ticket between two Newton rounds.
constexpr int gX = qRec, gPrev = qRec + 14, gTo = qRec + 28, gRec = qRec + 42; // + the projected state, previous, the target; odd stride

template <bool DIAG>
__global__ __launch_bounds__(64, 2) void geodesic_row16_kernel(const ccmp_consts K_arg, const double delta, const double lambda,
                                                               const double *__restrict__ from, const double *__restrict__ to,
                                                               unsigned long long E, int max_states, double *__restrict__ states,
                                                               int32_t *__restrict__ n_states, uint8_t *__restrict__ ok_out,
                                                               int32_t *__restrict__ newton_iters, const double *__restrict__ carry_in,
                                                               double *__restrict__ carry_out, int round_budget, int check_target,
                                                               unsigned long long *queue)
{
#include "ccmp_row16_geo_body.inc"
}

// geodesic_row16_scene_kernel — the same traversal with the StateValidityChecker's proxy pre-filter on the device
// (ccmp_geodesic_scene_batch): the reference's loop with interpolate == false, where svc->isValid(scratch) is "the scene's clearance
// of scratch > margin" (ccmp_clearance.h on the row's sixteen lanes, between the projection and the step test).  A refused state
// ends the edge with blocked = 1; the list holds the states before it.
template <bool DIAG>
__global__ __launch_bounds__(64, 2) void geodesic_row16_scene_kernel(const ccmp_consts K_arg, const double delta, const double lambda,
                                                                     const double *__restrict__ from, const double *__restrict__ to,
                                                                     unsigned long long E, int max_states, double *__restrict__ states,
                                                                     int32_t *__restrict__ n_states, uint8_t *__restrict__ ok_out,
                                                                     int32_t *__restrict__ newton_iters, const double *__restrict__ carry_in,
                                                                     double *__restrict__ carry_out, int round_budget, int check_target,
                                                                     unsigned long long *queue, const scene_dev *__restrict__ scene,
                                                                     const double margin, uint8_t *__restrict__ blocked_out,
                                                                     double *__restrict__ clearance_out)
{
#define CCMP_ROW16_SCENE
#include "ccmp_row16_geo_body.inc"
#undef CCMP_ROW16_SCENE
}

// ------------------------------------------------------------------------------------------------------------------------
// resident_row16_kernel — the resident service kernel (ccmp_resident.h: what it is for, the mailbox, what keeps it from hanging
// anything) for a problem in analytic mode.  One persistent 128-thread block like resident_service_kernel (ccmp_kernels_resident.hip),
// polling the same request header on the same stream, but on this unit's latency layout: two wavefronts, EIGHT rows of sixteen lanes.
//   kResProject                 one state on row 0 of wavefront 0: project_row16_kernel's sequence with source 0 and no wrap (the same
//                               text: ccmp_row16_eval.inc / ccmp_row16_step.inc, the same flags: the same bits)
//   kResFunction / IsSatisfied  one evaluation (ccmp_row16_eval.inc), as the traversal's isSatisfied(to)
//   kResJointValid              the bounds test of project_row16_kernel
//   kResGeodesicMulti           1..8 edges of discreteGeodesic / checkMotion, each on its own row through the text of
//                               geodesic_row16_kernel (ccmp_row16_geo_body.inc, included without its prologue).  The ticket word is an
//                               LDS word; from / to / carry_in are staged from the mailbox into LDS once and verified
//                               (ccmp_resident_proto.h); state rows and per-edge results go to the mailbox as the body writes them.
//                               The two wavefronts run the body independently — it has no barrier — and meet at block barriers
//                               before and after the request only.
// Every loop is bounded: the idle poll by idle_ticks, the read-it-again loop by kResRereads (then the request is answered with
// kResErrTorn), a projection by max_iter, a traversal by max_states and the reference's own break tests.
__device__ __forceinline__ unsigned long long res_load(const unsigned long long *p)
{
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void res_store(unsigned long long *p, unsigned long long v)
{
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned long long res_lane_word(unsigned long long v, int src_lane) // wave-uniform broadcast of one lane's word
{
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(v & 0xffffffffull), src_lane);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(v >> 32), src_lane);
  return ((unsigned long long)hi << 32) | lo;
}

template <bool DIAG>
__global__ __launch_bounds__(128, 1) void resident_row16_kernel(unsigned long long *box, unsigned long long last_tag,
                                                               unsigned long long idle_ticks /* of the 100 MHz wall clock */)
{
  __shared__ double ktab[kConstsDoubles + 1];
  __shared__ double lds[8 * gRec];                                   // one record per row
  __shared__ unsigned long long s_multi[ccmp_res::kMultiMaxWords];   // a several-edge request as read from the mailbox
  __shared__ double edge_from[8 * 14], edge_to[8 * 14], edge_carry[8 * 2];
  __shared__ double s_x[14];                                         // the state of a single-state command
  __shared__ unsigned long long s_tag, s_ticket;
  __shared__ int s_cmd, s_edges, s_bad;
  __shared__ unsigned int s_consts;
  __shared__ ccmp_res::MultiParams s_mp;
  const int tid = threadIdx.x;
  const int lane = tid & 63, l = lane & 15; // (lane: within the wavefront — what the row16 texts' ballots and shuffles index)
  const unsigned long long *consts = box + kResConstsOff / 8;
  const unsigned long long *req = box + kResReqOff / 8;
  const unsigned long long *mreq = box + kResMultiReqOff / 8;
  unsigned long long *resp = box + kResRespOff / 8;
  unsigned long long *mresp = box + kResMultiRespOff / 8;
  unsigned long long *state = box + kResStateOff / 8;
  const ccmp_consts &K = *reinterpret_cast<const ccmp_consts *>(ktab);
  double *const rec = lds + (tid >> 4) * gRec;
  unsigned int my_consts = ~0u; // nothing loaded yet: the first request brings its constants
  if (tid == 0) res_store(state, (unsigned long long)kResRunning);
  unsigned long long idle_since = wall_clock64();

  for (;;) {
    // ---- wait for a request: the header's five lines, 40 words in one load by wavefront 0 (resident_service_kernel's poll) -------
    if (tid < 64) {
      unsigned long long w = 0;
      if (tid < kResReqWords) w = res_load(req + tid);
      const int col = tid & 7;
      unsigned long long h = 0;
      if (col < 7) { const int r = 7 * col + 1; h = (w << r) | (w >> (64 - r)); }
      h ^= __shfl_xor(h, 1);
      h ^= __shfl_xor(h, 2);
      h ^= __shfl_xor(h, 4); // every lane of a line holds the line's checksum
      const bool torn = col == 7 && tid < kResReqWords && (unsigned int)(w >> 32) != (unsigned int)(h ^ (h >> 32));
      const bool clean = __builtin_amdgcn_ballot_w64(torn) == 0ull;
      const unsigned int ta = (unsigned int)res_lane_word(w, 7), tb = (unsigned int)res_lane_word(w, 15), tc = (unsigned int)res_lane_word(w, 23),
                         td = (unsigned int)res_lane_word(w, 31), te = (unsigned int)res_lane_word(w, 39);
      const bool fresh = clean && ta == tb && tb == tc && tc == td && td == te && te != (unsigned int)last_tag;
      if (fresh) {
        if (col < 7 && tid < 16) s_x[7 * (tid >> 3) + col] = __longlong_as_double((long long)w); // lines A, B: the state
        if (tid == 0) {
          const unsigned long long head = res_lane_word(w, 32);
          s_cmd = (int)(head & 0xffffffffull);
          s_consts = (unsigned int)(head >> 32);
          s_edges = (int)(unsigned int)(res_lane_word(w, 37) & 0xffffffffull); // kResGeodesicMulti: how many edges' lines to read
          s_tag = (unsigned long long)te;
        }
        last_tag = te;
      } else if (tid == 0) {
        s_cmd = (wall_clock64() - idle_since > idle_ticks) ? kResStop : kResNone; // nobody has asked for a while: leave by itself
      }
    }
    __syncthreads();
    const int cmd = s_cmd;
    if (cmd == kResNone) {
      __syncthreads(); // (s_cmd is rewritten at the top)
      continue;
    }
    if (cmd == kResStop) break;
    if (tid >= 64) last_tag = s_tag;
    // ---- the problem in force: its constants are reloaded when the host says they changed ----------------------------------------
    if (s_consts != my_consts) {
      __syncthreads();
      for (int k = tid; k < kConstsDoubles; k += 128) ktab[k] = __longlong_as_double((long long)res_load(consts + k));
      my_consts = s_consts;
      __syncthreads();
    }
    unsigned long long flags = 0ull;
    if (cmd == kResGeodesicMulti) {
      // ---- the edges' lines: staged into LDS, then verified (ccmp_res::line_ok on one thread per line, multi_unpack on thread 0 —
      // the two functions ccmp_res::multi_accept is made of); lines that do not agree are read again, kResRereads times at most
      const int hdr_edges = s_edges < 1 ? 1 : (s_edges > ccmp_res::kMultiMaxEdges ? ccmp_res::kMultiMaxEdges : s_edges);
      const int lines = ccmp_res::multi_lines(hdr_edges);
      bool accepted = false;
      for (int attempt = 0; attempt < kResRereads && !accepted; attempt++) {
        for (int w = tid; w < 8 * lines; w += 128) s_multi[w] = res_load(mreq + w);
        if (tid == 0) s_bad = 0;
        __syncthreads();
        if (tid < lines && !ccmp_res::line_ok((unsigned int)s_tag, s_multi + 8 * tid)) s_bad = 1;
        if (tid == 127) {
          ccmp_res::MultiParams m;
          const bool good = ccmp_res::multi_unpack(s_multi, &m);
          s_mp = m;
          // (the bounds of everything the traversal indexes: rows of the states area, words of the per-edge response)
          if (!good || m.E != s_edges || m.max_states < 1 || m.max_states > kResMaxStates) s_bad = 1;
        }
        __syncthreads();
        accepted = s_bad == 0;
        __syncthreads(); // (s_bad and s_multi are rewritten by the next attempt)
      }
      if (!accepted) flags = kResErrTorn;
      else {
        const int n_edges = s_mp.E;
        if (tid < 14 * n_edges) {
          const int e = tid / 14, i = tid - 14 * e;
          edge_from[tid] = __longlong_as_double((long long)s_multi[ccmp_res::multi_from_word(e, i)]);
          edge_to[tid] = __longlong_as_double((long long)s_multi[ccmp_res::multi_to_word(e, i)]);
        }
        if (tid < 2 * n_edges) edge_carry[tid] = __longlong_as_double((long long)s_multi[ccmp_res::multi_carry_word(tid >> 1, tid & 1)]);
        if (tid == 0) s_ticket = 0ull;
        __syncthreads();
        {
          // geodesic_row16_kernel's arguments, pointed at LDS (inputs, the ticket word) and at the mailbox (outputs)
          const unsigned long long E = (unsigned long long)n_edges;
          const int max_states = s_mp.max_states, round_budget = s_mp.round_budget, check_target = s_mp.check_target;
          const double delta = __longlong_as_double((long long)s_mp.delta_bits), lambda = __longlong_as_double((long long)s_mp.lambda_bits);
          const double *from = edge_from, *to = edge_to, *carry_in = s_mp.has_carry ? edge_carry : nullptr;
          double *states = reinterpret_cast<double *>(box + kResMultiStatesOff / 8);
          int32_t *n_states = reinterpret_cast<int32_t *>(mresp + kResMultiRespN), *newton_iters = reinterpret_cast<int32_t *>(mresp + kResMultiRespIts);
          uint8_t *ok_out = reinterpret_cast<uint8_t *>(mresp + kResMultiRespOk);
          double *carry_out = reinterpret_cast<double *>(mresp + kResMultiRespCarry);
          unsigned long long *queue = &s_ticket;
#define CCMP_ROW16_NO_PROLOGUE
#include "ccmp_row16_geo_body.inc"
#undef CCMP_ROW16_NO_PROLOGUE
        }
      }
    } else if (cmd == kResProject || cmd == kResFunction || cmd == kResIsSatisfied || cmd == kResJointValid) {
      if (tid < 64) { // wavefront 0; its row 0 carries the state, rows 1..3 stay without one (as rows of project_row16_kernel past the batch)
        // joint role and chain role: as project_row16_kernel
        const bool jl = l < 14;
        const int lj = jl ? l : 13;
        const int aj = lj >= 7 ? 1 : 0, ij = lj - 7 * aj;
        double ax[3], ap[6];
#pragma unroll
        for (int k = 0; k < 3; k++) ax[k] = K.axis[aj][ij][k];
#pragma unroll
        for (int k = 0; k < 6; k++) ap[k] = K.aprod[aj][ij][k];
        const double lbe = K.lbe[ij], ube = K.ube[ij];
        const double sgn = aj ? -1.0 : 1.0;
        const int ac = (l / 3) & 1, rc = l % 3;
        double cee[3], cRt[9];
#pragma unroll
        for (int k = 0; k < 3; k++) cee[k] = K.ee[ac][k];
#pragma unroll
        for (int k = 0; k < 9; k++) cRt[k] = K.R_tool[ac][k];
        const double cd = K.base_R[ac][4 * rc], cbp = K.base_p[ac][rc];
        const bool row0 = lane < 16;
        double x = row0 ? s_x[lj] : 0.0;
        int iter = 0, updates = 0;
        double norm1 = 0.0, norm2 = 0.0;
        bool ok = false;
        if (cmd == kResJointValid) { // ConstraintFunction.h:43-55
          const bool bad = row0 && jl && (x < lbe || x > ube);
          ok = (__builtin_amdgcn_ballot_w64(bad) & 0xFFFFull) == 0ull;
        } else if (cmd == kResProject) { // KinematicChainConstraint::project (ConstraintFunction.h:57-82): project_row16_kernel's sequence
          bool active = row0;
          for (;;) {
            if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
#include "ccmp_row16_eval.inc"
            bool cont = false;
            if (active) { // ConstraintFunction.h:68, quirks included
              const bool c1 = f[0] > K.tol_pos;
              norm1 = c1 ? 1.0 : 0.0;
              bool resid = c1;
              if (!c1) { norm2 = f[1]; resid = f[1] > K.tol_rot; }
              if (resid) { cont = iter < K.max_iter; iter++; }
            }
            {
              const bool fin = active && !cont;
              bool bad = false;
              if (fin && jl) {
                if (x < lbe) bad = true;
                if (x > ube) bad = true;
                res_store(resp + kResRespQ + lj, (unsigned long long)__double_as_longlong(x));
              }
              const unsigned long long badmask = __builtin_amdgcn_ballot_w64(bad);
              if (fin) {
                ok = ((badmask & 0xFFFFull) == 0ull) && (norm1 < K.tol_pos) && (norm2 < K.tol_rot);
                active = false;
              }
            }
            if (__builtin_amdgcn_ballot_w64(cont) == 0ull) continue;
#include "ccmp_row16_step.inc"
          }
        } else { // function(x): one evaluation; KinematicChainConstraint::isSatisfied's test on it (ConstraintFunction.h:114-120)
#include "ccmp_row16_eval.inc"
          ok = (f[0] - f[0] == 0.0) && (f[1] - f[1] == 0.0) && f[0] <= K.tol_pos && f[1] <= K.tol_rot;
          if (tid < 2) res_store(resp + kResRespF + tid, (unsigned long long)__double_as_longlong(tid ? f[1] : f[0]));
        }
        if (tid == 0) flags = (unsigned long long)(ok ? 1u : 0u) | ((unsigned long long)(unsigned int)updates << 32);
      }
    } else {
      flags = kResErrTorn; // a command this kernel does not serve (the host never sends one): answered, refused
    }
    if (tid == 0) res_store(resp + kResRespFlags, flags);
    // every wavefront's result words are on their way before the tag is: system fence, block barrier, then the tag
    __threadfence_system();
    __syncthreads();
    if (tid == 0) {
      __hip_atomic_store(resp + kResRespDone, s_tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      idle_since = wall_clock64();
    }
    __syncthreads();
  }
  if (tid == 0) {
    __threadfence_system();
    __hip_atomic_store(state, (unsigned long long)kResExited, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

} // namespace

namespace ccmp_launch {

// One call of the analytic mode on one stream: the lane-pair kernel with pair_blocks wavefronts (0: none) and behind it, or
// alone, the latency kernel with latency_blocks wavefronts (0: none).  With both, a wavefront of the lane-pair kernel whose
// tickets are used up and that holds at most dump_below samples hands them over through `pool` (kPoolEntry doubles per
// sample; the fill count is read on the device: surplus wavefronts of the latency kernel exit at once).  queue: kFastQueues
// ticket words of the lane-pair kernel, the pool's fill count, the ticket word of the latency kernel.
hipError_t project_analytic(const ProjectCall &c, int pair_blocks, int dump_below, int latency_blocks, double *pool,
                            unsigned long long *queue, hipStream_t st)
{
  if (pair_blocks <= 0 && latency_blocks <= 0) return hipErrorInvalidValue;
  hipError_t e = clear_words(queue, (kFastQueues + 2) * 2, st); // a kernel, so that a stream capture replays it
  if (e != hipSuccess) return e;
  const ccmp_consts *K = c.K;
  unsigned long long *count = queue + kFastQueues, *lat_tickets = queue + kFastQueues + 1;
  const bool both = pair_blocks > 0 && latency_blocks > 0;
  if (pair_blocks > 0) {
#define CCMP_LAUNCH_PAIR(STOCK, TWIN)                                                                                                  \
  hipLaunchKernelGGL((project_pair_kernel<STOCK, TWIN>), dim3(pair_blocks), dim3(64), 0, st, *K, c.mode | (c.mode << 4), c.q_in, c.q_out, c.ok, \
                     c.iters, c.q_ambient, (unsigned long long)c.B, queue, c.seed, c.first, both ? pool : nullptr, count, dump_below)
    if (K->twin_arms) CCMP_LAUNCH_PAIR(true, true);
    else if (K->stock) CCMP_LAUNCH_PAIR(true, false);
    else CCMP_LAUNCH_PAIR(false, false);
#undef CCMP_LAUNCH_PAIR
  }
  if (latency_blocks > 0) {
    // srcmode: low nibble = where the samples come from (2: the pool), high nibble = the call's mode (a sample of a fused
    // sampleUniform is wrapped by whichever kernel finishes it)
    const int srcmode = (both ? 2 : c.mode) | (c.mode << 4);
    if (K->base_diag == 3)
      hipLaunchKernelGGL((project_row16_kernel<true>), dim3(latency_blocks), dim3(64), 0, st, *K, srcmode, c.q_in, c.q_out, c.ok, c.iters,
                         c.q_ambient, (unsigned long long)c.B, lat_tickets, c.seed, c.first, pool, count);
    else
      hipLaunchKernelGGL((project_row16_kernel<false>), dim3(latency_blocks), dim3(64), 0, st, *K, srcmode, c.q_in, c.q_out, c.ok, c.iters,
                         c.q_ambient, (unsigned long long)c.B, lat_tickets, c.seed, c.first, pool, count);
  }
  return hipGetLastError();
}

// The extend step in analytic mode, one call on one stream: the ticket word cleared (a kernel, so that a stream capture replays it),
// then geodesic_row16_kernel with `blocks` wavefronts (four edges each at a time).
hipError_t geodesic_analytic(const GeoCall &g, int blocks, unsigned long long *queue, hipStream_t st)
{
  if (blocks <= 0) return hipErrorInvalidValue;
  hipError_t e = clear_words(queue, 2, st);
  if (e != hipSuccess) return e;
#define CCMP_LAUNCH_GEO_ROW16(DIAG)                                                                                                       \
  hipLaunchKernelGGL((geodesic_row16_kernel<DIAG>), dim3(blocks), dim3(64), 0, st, *g.K, g.delta, g.lambda, g.from, g.to, (unsigned long long)g.E, \
                     g.max_states, g.states, g.n_states, g.ok, g.newton_iters, g.carry_in, g.carry_out, g.round_budget, g.check_target, queue)
  if (g.K->base_diag == 3) CCMP_LAUNCH_GEO_ROW16(true);
  else CCMP_LAUNCH_GEO_ROW16(false);
#undef CCMP_LAUNCH_GEO_ROW16
  return hipGetLastError();
}

// The same with a proxy scene: geodesic_row16_scene_kernel.
hipError_t geodesic_analytic_scene(const GeoCall &g, const GeoScene &s, int blocks, unsigned long long *queue, hipStream_t st)
{
  if (blocks <= 0) return hipErrorInvalidValue;
  hipError_t e = clear_words(queue, 2, st);
  if (e != hipSuccess) return e;
#define CCMP_LAUNCH_GEO_ROW16_SCENE(DIAG)                                                                                                       \
  hipLaunchKernelGGL((geodesic_row16_scene_kernel<DIAG>), dim3(blocks), dim3(64), 0, st, *g.K, g.delta, g.lambda, g.from, g.to, (unsigned long long)g.E, \
                     g.max_states, g.states, g.n_states, g.ok, g.newton_iters, g.carry_in, g.carry_out, g.round_budget, g.check_target, queue,     \
                     s.scene, s.margin, s.blocked, s.clearance)
  if (g.K->base_diag == 3) CCMP_LAUNCH_GEO_ROW16_SCENE(true);
  else CCMP_LAUNCH_GEO_ROW16_SCENE(false);
#undef CCMP_LAUNCH_GEO_ROW16_SCENE
  return hipGetLastError();
}

// The resident service kernel for a problem in analytic mode (ccmp_resident.cpp starts it on the service's own stream).
hipError_t resident_row16(int diag, void *box_dev, unsigned long long last_tag, unsigned long long idle_ticks, hipStream_t st)
{
  if (diag)
    hipLaunchKernelGGL(resident_row16_kernel<true>, dim3(1), dim3(128), 0, st, (unsigned long long *)box_dev, last_tag, idle_ticks);
  else
    hipLaunchKernelGGL(resident_row16_kernel<false>, dim3(1), dim3(128), 0, st, (unsigned long long *)box_dev, last_tag, idle_ticks);
  return hipGetLastError();
}

}  // namespace ccmp_launch
