// ccmp_kernels_plan.hip — the planner's loop on the roadmap store (ccmp_plan_*; the rule: csrc/ccmp_plan.h): the kernels that keep the
// loop's decisions and its state block (ccmp_plan_state) on the device between the launches of the units it calls.  Every kernel is ONE
// block; none loops beyond a bound that is a kernel argument or a constant, none waits for another.
//   plan_front_kernel      nearest_pose of the state block into the W `from` rows of the proposal
//   plan_tally_kernel      a growth step's (or a ladder's) outputs into the counters: one block of 256 lanes strides over the W rows and
//                          the W k slots, each lane adds its counts with one integer atomic per counter; lane 0 advances next_index
//   plan_check_kernel      one wavefront.  Lane 0 runs ccmp::plan_check — the gate, the carry rule over the <= 8 froms of each side IN THE
//                          LIST'S ORDER (a serial fold: the order is the rule's), the two thresholds, the state update — and copies
//                          pose[c] into nearest_pose; then lanes 0 .. 10 write one IK target and its seed row each: the goal pose, the nine
//                          ladder poses (ccmp::pose_interpolate of ccmp_object.h at 0.1 i) and the start pose, or a NaN row where the
//                          branch did not fire.  Every vertex index is range-checked against the store's size before it addresses a row.
//   plan_prefix_kernel     the ladder's prefix mask from valid[9] and ik_ok[9] (ccmp::plan_prefix) and the 16-byte summary the host reads:
//                          {prefix length, goal vertex solved, start vertex solved, the check ran}
//   plan_push_kernel       a committed new_index onto starts or goals under the cap (ccmp::plan_push)
//   plan_connected_kernel  the solution test of EVERY planner on the store, a template over the state type (ccmp_plan_state, ccmp_rrtc_state):
//                          one wavefront, lane l = pair (l / G, l % G) of the <= 8 x 8 pairs: the label compare, a ballot, and the lowest set
//                          bit is the first connected pair in start-major order — no race decides it
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
#include "ccmp_launch.h"
#include "ccmp_object.h"
#include "ccmp_plan.h"

namespace {

using ccmp_launch::GraphStore;
using ccmp_launch::PlanCheck;
constexpr int kWave = 64;
constexpr int kTallyThreads = 256;

__global__ __launch_bounds__(kTallyThreads) void plan_front_kernel(const ccmp_plan_state *__restrict__ state, double *__restrict__ from, unsigned int W)
{
  for (unsigned int i = threadIdx.x; i < W * 8u; i += kTallyThreads) from[i] = state->nearest_pose[i & 7u];
}

__global__ __launch_bounds__(kTallyThreads) void plan_tally_kernel(ccmp_plan_state *state, const int32_t *__restrict__ which, const uint8_t *__restrict__ ik_ok,
                                                                   const int32_t *__restrict__ new_index, const int32_t *__restrict__ mid_index,
                                                                   const int32_t *__restrict__ grow_state, unsigned int W, unsigned int k, int ladder)
{
  int valid = 0, solved = 0, kept = 0, mids = 0, unsettled = 0;
  for (unsigned int i = threadIdx.x; i < W; i += kTallyThreads) {
    if (which && which[i] >= 0) valid++;
    if (ik_ok && ik_ok[i]) solved++;
    if (new_index[i] >= 0) kept++;
    if (grow_state && grow_state[i] == CCMP_GROW_UNSETTLED) unsettled++;
  }
  if (mid_index)
    for (unsigned int i = threadIdx.x; i < W * k; i += kTallyThreads)
      if (mid_index[i] >= 0) mids++;
  ccmp_plan_counters *c = &state->counters;
  if (ladder) {
    if (kept) atomicAdd(&c->ladder_vertices, kept);
    return;
  }
  if (valid) atomicAdd(&c->valid_proposals, valid);
  if (solved) atomicAdd(&c->ik_successes, solved);
  if (kept) atomicAdd(&c->vertices_kept, kept);
  if (mids) atomicAdd(&c->mid_stones, mids);
  if (unsettled) atomicAdd(&c->unsettled, unsettled);
  if (threadIdx.x == 0) {
    atomicAdd(&c->proposals, (int)W);
    state->next_index += (uint64_t)W;
  }
}

__global__ __launch_bounds__(kWave) void plan_check_kernel(const GraphStore s, ccmp_plan_state *state, const PlanCheck c)
{
  __shared__ int32_t trig[4];
  __shared__ int32_t side[4]; // goal IK tried, start IK tried, the start side's seed vertex
  const int lane = threadIdx.x;
  const unsigned long long N = s.N;
  if (lane == 0) {
    ccmp::plan_check(state, N, c.a_idx, c.a_dist, c.a_from, c.b_idx, c.b_dist, c.b_from, trig);
    side[0] = trig[1] && state->n_goals < CCMP_PLAN_MAX_GOALS;
    side[1] = trig[2] && state->n_starts < CCMP_PLAN_MAX_STARTS;
    side[2] = state->sprevious;
    if (trig[1] && trig[3] >= 0 && (unsigned long long)trig[3] < N)
      for (int i = 0; i < 8; i++) state->nearest_pose[i] = s.poses[(size_t)trig[3] * 8 + i];
    for (int i = 0; i < 4; i++) c.trig[i] = trig[i];
  }
  __syncthreads();
  if (lane >= ccmp::kPlanTargets) return;
  const bool goal_row = lane == ccmp::kPlanGoalRow, start_row = lane == ccmp::kPlanStartRow;
  const int32_t v = start_row ? side[2] : trig[3];
  bool on = goal_row ? side[0] != 0 : start_row ? side[1] != 0 : trig[1] != 0;
  on = on && v >= 0 && (unsigned long long)v < N;
  double *t = c.targets + lane * 8, *sd = c.seeds + lane * 14;
  const double nan = __builtin_nan("");
  if (!on) {
#pragma unroll
    for (int i = 0; i < 7; i++) t[i] = nan;
    t[7] = 0.0;
#pragma unroll
    for (int i = 0; i < 14; i++) sd[i] = nan;
    return;
  }
  if (goal_row || start_row) {
#pragma unroll
    for (int i = 0; i < 7; i++) t[i] = goal_row ? c.goal[i] : c.start[i];
    t[7] = 0.0;
  } else {
    ccmp::pose_interpolate(s.poses + (size_t)v * 8, c.goal, 0.1 * (double)lane, t); // lane = the ladder's i = 1 .. 9
  }
#pragma unroll
  for (int i = 0; i < 14; i++) sd[i] = s.joints[(size_t)v * 14 + i];
}

__global__ __launch_bounds__(kWave) void plan_prefix_kernel(const ccmp_plan_state *__restrict__ state, const int32_t *__restrict__ trig,
                                                            const uint8_t *__restrict__ valid, const uint8_t *__restrict__ ik_ok, uint8_t *__restrict__ vertex_ok,
                                                            int32_t *__restrict__ summary)
{
  if (threadIdx.x != 0) return;
  const int n = trig[1] ? ccmp::plan_prefix(valid, ik_ok + ccmp::kPlanLadderRow, vertex_ok) : 0;
  if (!trig[1])
    for (int i = 0; i < CCMP_PLAN_LADDER; i++) vertex_ok[i] = 0;
  summary[0] = n;
  summary[1] = trig[1] && state->n_goals < CCMP_PLAN_MAX_GOALS && ik_ok[ccmp::kPlanGoalRow];
  summary[2] = trig[2] && state->n_starts < CCMP_PLAN_MAX_STARTS && ik_ok[ccmp::kPlanStartRow];
  summary[3] = trig[0];
}

__global__ __launch_bounds__(kWave) void plan_push_kernel(ccmp_plan_state *state, int which, const int32_t *__restrict__ new_index)
{
  if (threadIdx.x == 0) ccmp::plan_push(state, which, new_index[0]);
}

template <class S> __global__ __launch_bounds__(kWave) void plan_connected_kernel(const GraphStore s, S *state, int bump_cycle)
{
  const int lane = threadIdx.x;
  const int n_s = ccmp::planner_clamp(state->n_starts), G = ccmp::planner_clamp(state->n_goals);
  const bool solved = state->status == CCMP_PLAN_SOLVED;
  bool hit = false;
  if (!solved && G > 0 && lane < n_s * G) hit = ccmp::pair_connected(state, lane / G, lane % G, s.labels, s.N);
  const unsigned long long mask = __ballot(hit);
  if (lane != 0) return;
  if (bump_cycle) state->cycle += 1;
  if (mask) {
    const int first = __ffsll((long long)mask) - 1;
    ccmp::solved(state, first / G, first % G);
  }
}

template <class S> hipError_t launch_connected(const GraphStore &s, S *state, int bump_cycle, hipStream_t st)
{
  hipLaunchKernelGGL(plan_connected_kernel<S>, dim3(1), dim3(kWave), 0, st, s, state, bump_cycle);
  return hipGetLastError();
}

}  // namespace

namespace ccmp_launch {

hipError_t plan_front(const ccmp_plan_state *state, double *from, size_t W, hipStream_t st)
{
  hipLaunchKernelGGL(plan_front_kernel, dim3(1), dim3(kTallyThreads), 0, st, state, from, (unsigned int)W);
  return hipGetLastError();
}

hipError_t plan_tally(ccmp_plan_state *state, const int32_t *which, const uint8_t *ik_ok, const int32_t *new_index, const int32_t *mid_index,
                      const int32_t *grow_state, size_t W, int k, int ladder, hipStream_t st)
{
  hipLaunchKernelGGL(plan_tally_kernel, dim3(1), dim3(kTallyThreads), 0, st, state, which, ik_ok, new_index, mid_index, grow_state, (unsigned int)W,
                     (unsigned int)k, ladder);
  return hipGetLastError();
}

hipError_t plan_check(const GraphStore &s, ccmp_plan_state *state, const PlanCheck &c, hipStream_t st)
{
  hipLaunchKernelGGL(plan_check_kernel, dim3(1), dim3(kWave), 0, st, s, state, c);
  return hipGetLastError();
}

hipError_t plan_prefix(const ccmp_plan_state *state, const int32_t *trig, const uint8_t *valid, const uint8_t *ik_ok, uint8_t *vertex_ok, int32_t *summary,
                       hipStream_t st)
{
  hipLaunchKernelGGL(plan_prefix_kernel, dim3(1), dim3(kWave), 0, st, state, trig, valid, ik_ok, vertex_ok, summary);
  return hipGetLastError();
}

hipError_t plan_push(ccmp_plan_state *state, int which, const int32_t *new_index, hipStream_t st)
{
  hipLaunchKernelGGL(plan_push_kernel, dim3(1), dim3(kWave), 0, st, state, which, new_index);
  return hipGetLastError();
}

hipError_t plan_connected(const GraphStore &s, ccmp_plan_state *state, int bump_cycle, hipStream_t st) { return launch_connected(s, state, bump_cycle, st); }
hipError_t plan_connected(const GraphStore &s, ccmp_rrtc_state *state, int bump_cycle, hipStream_t st) { return launch_connected(s, state, bump_cycle, st); }

}  // namespace ccmp_launch
