// ccmp_kernels_ik.hip — growTree's sampleCalibGoal step on the device (csrc/ccmp_ik.h holds the solver and the rule, one text for host and
// device): ik_solve_kernel, one candidate (target, seed slot, arm, start configuration) per lane, and ik_select_kernel, one thread per
// target over the candidates' records.  Built with the k-NN unit's flags and without machine LICM (build.py); no scratch (_SCRATCH_RULES),
// no LDS.
#include <hip/hip_runtime.h>

#include "ccmp_ik.h"
#include "ccmp_launch.h"

namespace {

// two wavefronts per SIMD: the register budget ik_solve_kernel is allocated for (it takes 190 of 256)
#define CCMP_IK_OCCUPANCY __attribute__((amdgpu_waves_per_eu(2, 2)))
constexpr int kThreads = 64; // one wavefront per block: a block leaves as soon as its slowest candidate has

// Lane n of arm blockIdx.y (the arm is uniform over a block, so its constants stay scalar): slot ts = n / (1 + R) = t S + s, candidate
// r = n % (1 + R).  The round loop is uniform over the wavefront — it runs while any lane is still solving, at most max_rounds steps and
// one last test; a lane that has converged, was skipped or lies beyond the call idles through the others' rounds.
template <bool STOCK>
__global__ __launch_bounds__(kThreads) CCMP_IK_OCCUPANCY void ik_solve_kernel(const ccmp_consts K, const ccmp::ik_arms arms, const ccmp::ik_params P, const double *__restrict__ poses,
                                                            const double *__restrict__ seeds, unsigned long long slots, int S, unsigned long long rng_seed,
                                                            unsigned long long first_index, double *__restrict__ rec_q, int32_t *__restrict__ rec_rounds,
                                                            double *__restrict__ rec_d2)
{
  const int arm = (int)blockIdx.y;
  const unsigned long long C = 1ull + (unsigned long long)P.restarts;
  const unsigned long long n = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  const bool mine = n < slots * C;
  const unsigned long long ts = mine ? n / C : 0ull;
  const int r = (int)(n - ts * C);
  const unsigned long long t = ts / (unsigned long long)S;
  double q[7];
  bool finite = true;
  const double *row = seeds + ts * 14, *pose = poses + t * 8;
  {
    double seed7[7]; // read again behind the loop: it need not live across it
#pragma unroll
    for (int i = 0; i < 7; i++) {
      seed7[i] = row[7 * arm + i];
      finite = finite && ccmp::ik_finite(row[i]) && ccmp::ik_finite(row[7 + i]);
    }
    ccmp::ik_start(K, P, rng_seed, first_index * (unsigned long long)S + ts, arm, r, seed7, q);
  }
  bool active = mine && finite;
  int rounds = finite ? ccmp::kIkNotConverged : ccmp::kIkSkipped;
  for (int it = 0; it <= P.max_rounds; it++) {
    if (active && ccmp::ik_round<STOCK>(K, arm, P, pose, arms.R[arm], arms.p[arm], q, it < P.max_rounds)) {
      rounds = it;
      active = false;
    }
    if (__builtin_amdgcn_ballot_w64(active) == 0ull) break;
  }
  if (!mine) return;
  const unsigned long long c = (ts * 2ull + (unsigned long long)arm) * C + (unsigned long long)r;
#pragma unroll
  for (int i = 0; i < 7; i++) rec_q[c * 7 + i] = finite ? q[i] : __builtin_nan("");
  rec_rounds[c] = rounds;
  double seed7[7];
#pragma unroll
  for (int i = 0; i < 7; i++) seed7[i] = row[7 * arm + i];
  rec_d2[c] = finite ? ccmp::ik_seed_d2(q, seed7) : __builtin_nan("");
}

__global__ __launch_bounds__(kThreads) void ik_select_kernel(const double *__restrict__ rec_q, const int32_t *__restrict__ rec_rounds, const double *__restrict__ rec_d2,
                                                             unsigned long long T, int S, int R, double *__restrict__ q_out, uint8_t *__restrict__ ok,
                                                             int32_t *__restrict__ which)
{
  const unsigned long long t = (unsigned long long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  ccmp::ik_select(rec_q, rec_rounds, rec_d2, (size_t)t, S, R, q_out + t * 14, ok + t, which + t);
}

// ccmp_roadmap_grow: the neighbours' joint rows as seed slots in rank order; an empty slot (-1) is a NaN seed, which the solver skips
__global__ __launch_bounds__(256) void ik_gather_seeds_kernel(const double *__restrict__ joints, const int32_t *__restrict__ nbr_idx, unsigned long long slots,
                                                              double *__restrict__ seeds)
{
  const unsigned long long w = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (w >= slots * 14) return;
  const int32_t j = nbr_idx[w / 14];
  seeds[w] = j < 0 ? __builtin_nan("") : joints[(size_t)j * 14 + w % 14];
}

// ccmp_roadmap_grow: one thread per edge e = q k + r (ccmp_launch.h: ik_grow_prepare)
__global__ __launch_bounds__(256) void ik_grow_prepare_kernel(const double *__restrict__ joints, const int32_t *__restrict__ nbr_idx, const uint8_t *__restrict__ ik_ok,
                                                              const double *__restrict__ q_new, unsigned long long Q, int k, int32_t *__restrict__ masked,
                                                              double *__restrict__ q_trav)
{
  const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= Q * (unsigned long long)k) return;
  const unsigned long long q = e / (unsigned long long)k;
  const bool have = ik_ok[q] != 0;
  int32_t j = nbr_idx[e];
  if (!have) j = -1;
  if (j >= 0) {
    bool finite = true;
    for (int c = 0; c < 14; c++) finite = finite && ccmp::ik_finite(joints[(size_t)j * 14 + c]);
    if (!finite) j = -1;
  }
  masked[e] = j;
  if (e == q * (unsigned long long)k)
    for (int c = 0; c < 14; c++) q_trav[q * 14 + c] = have ? q_new[q * 14 + c] : 0.0;
}

}  // namespace

namespace ccmp_launch {

hipError_t ik_solve(const IkCall &c, hipStream_t st)
{
  const unsigned long long slots = (unsigned long long)c.T * (unsigned long long)c.S;
  const unsigned long long lanes = slots * (unsigned long long)(1 + c.P->restarts);
  const dim3 grid((unsigned int)((lanes + kThreads - 1) / kThreads), 2);
  if (c.K->stock)
    hipLaunchKernelGGL(ik_solve_kernel<true>, grid, dim3(kThreads), 0, st, *c.K, *c.arms, *c.P, c.poses, c.seeds, slots, c.S, c.rng_seed, c.first_index, c.rec_q,
                       c.rec_rounds, c.rec_d2);
  else
    hipLaunchKernelGGL(ik_solve_kernel<false>, grid, dim3(kThreads), 0, st, *c.K, *c.arms, *c.P, c.poses, c.seeds, slots, c.S, c.rng_seed, c.first_index, c.rec_q,
                       c.rec_rounds, c.rec_d2);
  return hipGetLastError();
}

hipError_t ik_select(const IkCall &c, double *q_out, uint8_t *ok, int32_t *which, hipStream_t st)
{
  hipLaunchKernelGGL(ik_select_kernel, dim3((unsigned int)((c.T + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, c.rec_q, c.rec_rounds, c.rec_d2,
                     (unsigned long long)c.T, c.S, c.P->restarts, q_out, ok, which);
  return hipGetLastError();
}

hipError_t ik_gather_seeds(const double *joints, const int32_t *nbr_idx, size_t slots, double *seeds, hipStream_t st)
{
  hipLaunchKernelGGL(ik_gather_seeds_kernel, dim3((unsigned int)((slots * 14 + 255) / 256)), dim3(256), 0, st, joints, nbr_idx, (unsigned long long)slots, seeds);
  return hipGetLastError();
}

hipError_t ik_grow_prepare(const double *joints, const int32_t *nbr_idx, const uint8_t *ik_ok, const double *q_new, size_t Q, int k, int32_t *masked,
                           double *q_trav, hipStream_t st)
{
  hipLaunchKernelGGL(ik_grow_prepare_kernel, dim3((unsigned int)((Q * (size_t)k + 255) / 256)), dim3(256), 0, st, joints, nbr_idx, ik_ok, q_new,
                     (unsigned long long)Q, k, masked, q_trav);
  return hipGetLastError();
}

}  // namespace ccmp_launch
