// ccmp_kernels_ik_vet.hip — the collision gate of growTree's sampleCalibGoal on the device (csrc/ccmp_ik_vet.h holds the rule,
// csrc/ccmp_scene_math.h the arm clearance's arithmetic, each one text for host and device): ik_vet_kernel, the arm clearance of every
// candidate record (and of ccmp_arm_clearance_batch's rows), sixteen lanes per candidate; ik_assemble_kernel, one thread per
// (target, slot); ik_pick_kernel, one thread per target.  Between the last two the
// slots' full clearances come from ccmp_clearance_batch on the same stream.  Built with the IK unit's flags; no scratch (_SCRATCH_RULES).
#include <hip/hip_runtime.h>

#include "ccmp_fd_common.h"
#include "ccmp_ik_vet.h"
#include "ccmp_launch.h"
#include "ccmp_scene_math.h"

using namespace ccmp;

namespace {

constexpr int kRow = 16, kRows = 64 / kRow; // lanes per candidate, candidates per wavefront (one wavefront per block)
constexpr int kThreads = 256;               // of the two per-thread kernels

// Row `row` of the wavefront works on row n = 4 blockIdx.x + row of arm (arm0 + blockIdx.y): the arm is uniform over the block, so its
// constants and its pair list stay scalar.  per > 0: the rows are the candidate records of a pose-IK call, n = ts per + r -> record
// c = (2 ts + arm) per + r, and a record that did not converge or was skipped does no work and gets -inf; per == 0: the rows are the
// caller's own, c = n.  The work split of ccmp_clearance.h: state_clearance<16> with one arm's chain, on the text of ccmp_scene_math.h —
//   1  lanes 0..6: the rotation of joint `tid` (scene_joint_rot), into the space the centres take later;
//   2  lanes 0..2: row tid of the arm's chain (scene_chain_row), the eight frames into LDS;
//   3  lane s, s + 16, ...: the world centre of stored sphere s (scene_place) unless it moves on the other arm;
//   4  lane i, i + 16, ...: entry i of the arm's pair list (scene_pair_clearance); the minimum over the row by four exchanges.
// The rows of a wavefront never wait for each other or for another wavefront: LDS accesses of one wavefront complete in order, so a
// compiler barrier stands where a block would need __syncthreads.  Every loop is bounded by the scene's sizes.  2.3 KB of LDS per row.
__global__ __launch_bounds__(64) void ik_vet_kernel(const ccmp_consts K, const scene_dev *__restrict__ S, const scene_arm_dev *__restrict__ A,
                                                    const double *__restrict__ q7, const int32_t *__restrict__ rounds, unsigned long long n_rows, int per,
                                                    int arm0, double margin, double *__restrict__ clear, uint8_t *__restrict__ free_out)
{
  __shared__ double lds[kRows][kSceneArmFrames + kSceneCentres];
  const int arm = arm0 + (int)blockIdx.y;
  const int lane = (int)threadIdx.x, row = lane / kRow, tid = lane % kRow;
  const unsigned long long n = (unsigned long long)blockIdx.x * kRows + (unsigned long long)row;
  const bool mine = n < n_rows;
  unsigned long long c = 0;
  if (mine) c = per > 0 ? ((n / (unsigned long long)per) * 2ull + (unsigned long long)arm) * (unsigned long long)per + n % (unsigned long long)per : n;
  const bool work = mine && (rounds == nullptr || rounds[c] >= 0);
  double *fr = lds[row], *cen = fr + kSceneArmFrames, *rj = cen; // rj [7][9]: dead once the frames exist
  double best = __builtin_inf();
  bool finite = true;
  if (work) {
    const double *x = q7 + c * 7;
#pragma unroll
    for (int i = 0; i < 7; i++) finite = finite && scene_finite(x[i]);
    if (tid < 7) scene_joint_rot(K, arm, tid, x[tid], rj + 9 * tid);
    asm volatile("" ::: "memory");
    if (tid < 3) scene_chain_row(K, arm, tid, rj, fr);
    asm volatile("" ::: "memory");
    const int ns = S->n_spheres, np = A->n_pairs[arm];
    for (int s = tid; s < ns; s += kRow) {
      const int slot = S->slot[s], m = scene_moving_arm(slot);
      if (m >= 0 && m != arm) continue; // moving on the other arm: in none of this arm's pairs
      const double cs[3] = {S->c[s][0], S->c[s][1], S->c[s][2]};
      double w[3];
      scene_place(K, slot, cs, fr, w);
      cen[3 * s] = w[0]; cen[3 * s + 1] = w[1]; cen[3 * s + 2] = w[2];
    }
    asm volatile("" ::: "memory");
    for (int i = tid; i < np; i += kRow) {
      const double clr = scene_pair_clearance(S, cen, (int)A->pair[arm][i]);
      if (clr < best) best = clr;
    }
  }
#pragma unroll
  for (int m = kRow / 2; m >= 1; m >>= 1) { // minimum over the row: every lane of the wavefront takes part, an idle row exchanges +inf
    const double v = shfl_f64(best, lane ^ m);
    if (v < best) best = v;
  }
  if (mine && tid == 0) {
    const double out = !work ? -__builtin_inf() : (finite ? best : __builtin_nan(""));
    clear[c] = out;
    if (free_out) free_out[c] = (uint8_t)(out > margin);
  }
}

__global__ __launch_bounds__(kThreads) void ik_assemble_kernel(const double *__restrict__ rec_q, const int32_t *__restrict__ rec_rounds,
                                                               const double *__restrict__ rec_d2, const double *__restrict__ cand_clear,
                                                               unsigned long long slots, int R, double margin, double *__restrict__ slot_q,
                                                               uint8_t *__restrict__ slot_has)
{
  const unsigned long long ts = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (ts >= slots) return;
  slot_has[ts] = ik_vet_assemble(rec_q, rec_rounds, rec_d2, cand_clear, (size_t)ts, R, margin, slot_q + ts * 14) ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void ik_pick_kernel(const double *__restrict__ slot_q, const uint8_t *__restrict__ slot_has,
                                                           const double *__restrict__ slot_clear, unsigned long long T, int S, double margin,
                                                           double *__restrict__ q_out, uint8_t *__restrict__ ok, int32_t *__restrict__ which,
                                                           double *__restrict__ clearance, double *__restrict__ slot_out)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  ik_vet_pick(slot_q, slot_has, slot_clear, (size_t)t, S, margin, q_out + t * 14, ok + t, which + t, clearance ? clearance + t : nullptr, slot_out);
}

}  // namespace

namespace ccmp_launch {

hipError_t ik_vet(const ccmp_consts *K, const ccmp::scene_dev *scene, const ccmp::scene_arm_dev *arms, const double *q7, const int32_t *rounds, size_t n_rows,
                  int per, int arm0, int n_arms, double margin, double *clear, uint8_t *free_out, hipStream_t st)
{
  const dim3 grid((unsigned int)((n_rows + kRows - 1) / kRows), (unsigned int)n_arms);
  hipLaunchKernelGGL(ik_vet_kernel, grid, dim3(64), 0, st, *K, scene, arms, q7, rounds, (unsigned long long)n_rows, per, arm0, margin, clear, free_out);
  return hipGetLastError();
}

hipError_t ik_assemble(const double *rec_q, const int32_t *rec_rounds, const double *rec_d2, const double *cand_clear, size_t slots, int R, double margin,
                       double *slot_q, uint8_t *slot_has, hipStream_t st)
{
  hipLaunchKernelGGL(ik_assemble_kernel, dim3((unsigned int)((slots + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, rec_q, rec_rounds, rec_d2, cand_clear,
                     (unsigned long long)slots, R, margin, slot_q, slot_has);
  return hipGetLastError();
}

hipError_t ik_pick(const double *slot_q, const uint8_t *slot_has, const double *slot_clear, size_t T, int S, double margin, double *q_out, uint8_t *ok,
                   int32_t *which, double *clearance, double *slot_out, hipStream_t st)
{
  hipLaunchKernelGGL(ik_pick_kernel, dim3((unsigned int)((T + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, slot_q, slot_has, slot_clear,
                     (unsigned long long)T, S, margin, q_out, ok, which, clearance, slot_out);
  return hipGetLastError();
}

}  // namespace ccmp_launch
