/* ccmp_ctx.h — internals shared by the host translation units of libccmp (ccmp_api.cpp, ccmp_host_io.cpp, ccmp_comm.cpp); not part of
 * the public ABI. */
#ifndef CCMP_CTX_H
#define CCMP_CTX_H
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>

#include "../../include/ccmp.h"

namespace ccmp { struct ik_params; }

namespace ccmp_host {

/* text of the last HIP / RCCL failure on this thread (ccmp_last_hip_error) */
extern thread_local char g_hip_err[256];

inline int hip_fail(hipError_t e, const char *what)
{
  snprintf(g_hip_err, sizeof g_hip_err, "%s: %s", what, hipGetErrorString(e));
  return CCMP_EHIP;
}
#define HIP_TRY(...)                                                    \
  do {                                                                  \
    hipError_t e_ = (__VA_ARGS__);                                      \
    if (e_ != hipSuccess) return ccmp_host::hip_fail(e_, #__VA_ARGS__); \
  } while (0)

/* makes `dev` current for the lifetime of the guard and restores the previous device */
struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev)
  {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard()
  {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

}  // namespace ccmp_host

// Scheduling constants.  Every value below was chosen from an interleaved A/B on the device; the tables behind them live in
// DESIGN_experiments.md §11 (they were comments here until round 5), the regimes they delimit are what ccmp_ctx_describe() prints,
// and tools/policy_check.py re-times each boundary on whatever box it runs on.
constexpr size_t kDefaultSmallBatch = 10240;       // at or below: the latency kernel alone
constexpr size_t kSplitWideMax = 24576;            // split launch: up to here two latency blocks per CU for the front (fd_split*)
constexpr size_t kGeoGroupHighCut = 20480;         // bulk extend calls: the low cut of the order is 40 rounds below this many edges, 48 from here on ...
constexpr size_t kGeoGroupLateHandoverFrom = 32768; // bulk extend calls: the group kernel hands over below 50 % occupancy up to here, below 80 % from here on (profiles/r05_bulk_handover_sweep.log)
constexpr size_t kGeoGroupHigherCut = 65536;        // ... and 56 from here on (profiles/r05_low_cut_sweep.log: 65 536 edges -1.7 %, 131 072 -2.1 % against 48)
constexpr size_t kDefaultLatencyOrderMin = 2049;   // latency kernel alone: FP32 scout order as soon as the blocks take tickets (more samples than blocks)
constexpr size_t kDefaultLptMinBatch = 16384;      // throughput kernel: the scout's order pays from here on
constexpr size_t kOccupancyHandoverBelow = 53248;  // below: the throughput kernel hands over by occupancy, from here on at once
constexpr int kOccupancyHandoverValue = 10 + 70;   // "handover_threshold" encoding of that rule: 10 + per cent of the group slots (70 %)
constexpr size_t kNoHandoverFrom = 131072;         // ordered batches of this size or more end on their shortest samples: no hand-over
// fixed since round 6 (no option sets them any more)
constexpr int kDefaultFdHeadRounds = 5;            // from fd_head_min_batch samples on: every sample's first rounds in a launch of their own (0 = one launch; DESIGN_experiments.md §5.6, tools/head_rounds_model.py)
constexpr size_t kDefaultFdHeadMinBatch = 262144;  // ... from here on: the call must be bound by the chip's turnover of rounds, not by its longest sample's chain of them — a sample's first rounds end only with the whole head launch (131 584 samples: +16 %, 196 608: -1.7 %, 262 144: -1.7 %)
constexpr int kPoolLongRemaining = 24;             // two-class hand-over: samples with at least this many predicted iterations left go first
constexpr int kLatencyBlocksPerCu = 8;             // the projector's latency kernel (and the extend step's throughput flavour): blocks per CU
constexpr int kScoutBlocksPerCu = 2;               // scout_kernel: 256-lane blocks per CU at most (two wavefronts per SIMD; its lanes refill from their wavefront's slice)
constexpr int kScoutPairBlocksPerCu = 1;           // the scout's two-lanes-per-sample form while every sample gets its pair at once
constexpr size_t kScoutPairMaxEdges = 131072;      // extend step: the scout's two-lanes-per-edge form up to this many edges
constexpr int kGeoBlocksPerCu = 4;                 // the extend step's latency flavour: blocks per CU
constexpr int kGeoGroupHeavyPermille = 100;        // bulk extend calls: the front is the edges beyond the scout's cap if they carry this much of the work
constexpr int kGeoGroupFrontPerCu = 8;             // bulk extend calls: latency blocks of the front per CU ...
constexpr int kGeoGroupWavesPerCu = 8;             // ... and wavefronts of geodesic_group_kernel per CU

// One execution context (include/ccmp.h).  The tuning members are reached by name through the option table of ccmp_policy.cpp
// (ccmp_ctx_set_option / ccmp_ctx_get_option / ccmp_ctx_option_info), which also holds their ranges and one-line meanings; their
// initialisers here ARE the built-in defaults the table reports.
struct ccmp_ctx {
  int device = 0;
  int num_cus = 0;
  hipStream_t stream = nullptr;        // internal stream of the *_host entry points
  hipStream_t side = nullptr;          // side stream of split launches (highest priority: a hardware queue of its own)
  hipEvent_t fork = nullptr, join = nullptr;
  hipEvent_t gate = nullptr;           // head launch of a large projector batch: holds the head back until the side stream has reached the scout pass
  unsigned long long *queue = nullptr; // work-queue words: ccmp_launch.h (QueueWord)
  double *pool = nullptr;              // straggler hand-over records (throughput kernel -> latency kernel)
  size_t pool_cap = 0;                 // in records
  double *fd_state = nullptr;          // head -> resume launch of a large projector batch: one row per sample (ccmp_launch.h: kStagedRow doubles on stock twin arms, kPoolEntry otherwise)
  size_t fd_state_cap = 0;             // in doubles
  void *lpt_buf = nullptr;             // pred (u16 x B) | hist (u32 x 1024) | order (u32 x B) | flags (u8 x B, bulk checkMotion)
  size_t lpt_cap = 0;                  // in samples
  double *geo_pool = nullptr;          // bulk extend hand-over: kGeoPoolEntry doubles per edge
  size_t geo_pool_cap = 0;
  unsigned int *scan = nullptr;        // compaction block counts
  size_t scan_cap = 0;
  void *knn_ws = nullptr;              // k-NN: the partitions' lists (ccmp_launch.h: KnnShape)
  size_t knn_ws_cap = 0;               // in bytes
  void *retime_ws = nullptr;           // ccmp_path_timestamps: status-independent scratch, A bits [F] | ceiling [rows] | envelope [rows] (ccmp_retime.cpp)
  size_t retime_ws_cap = 0;            // in bytes
  double *connect_ws = nullptr;        // ccmp_connect_batch: the gathered endpoints, from [E][14] then to [E][14]
  size_t connect_ws_cap = 0;           // in edges
  void *ik_ws = nullptr;               // ccmp_pose_ik_batch: the candidates' records, q [C][7] | d2 [C] | rounds [C] (ccmp_launch.h: IkCall)
  size_t ik_ws_cap = 0;                // in candidates
  void *ik_vet_ws = nullptr;           // ccmp_pose_ik_vetted_batch: cand_clear [C] | slot_clear [T S] | slot_q [T S][14] | slot_has [T S] (ccmp_ik.cpp: ik_vetted_launches)
  size_t ik_vet_ws_cap = 0;            // in bytes
  void *stage = nullptr;               // device staging of the *_host conveniences
  size_t stage_cap = 0;
  void *pin = nullptr;                 // pinned, device-mapped host block for small *_host calls (single states of the reference signature)
  void *pin_dev = nullptr;             // the same block as the kernels see it
  // completion word of single-state calls (last 64 bytes of the pinned block): the kernel publishes done_seq behind its results
  // and the host polls it instead of waiting for the stream's completion signal
  unsigned int done_seq = 0;
  bool done_armed = false;             // set by the launch path when the launch it made will publish done_seq
  bool want_done = false;              // set by the host entry point that is going to poll
  const unsigned int *order = nullptr; // experimental: externally supplied processing order
  double shard_launch_ms = -1.0;       // ccmp_*_sharded*: when this context's shard had its upload behind it (host clock, ms from entry) ...
  hipEvent_t ev_shard = nullptr;       // ... and the event recorded on its stream at that point
  // resident service kernel (opt-in, option "resident"; ccmp_resident.h)
  struct ccmp_resident *resident = nullptr;
  int resident_on = 0;
  long resident_served = 0;            // requests the service kernel has answered for this context (read-only option "resident_served")
  int resident_gave_up = 0;            // how often a start of the service kernel gave up (it did not get to run within 5 ms: that ONE call took the launch path; ccmp_resident.cpp)

  // ---- tuning (option table: ccmp_policy.cpp) ----------------------------------------------------------------------------
  int waves_per_cu = 0;                // persistent wavefronts of the throughput kernels per CU (0 = 12)
  int wave_kernel = 1;                 // "hand_over": 0 throughput kernel only, 1 + latency kernel for stragglers, 2 latency kernel only
  size_t small_batch = kDefaultSmallBatch;
  int flat_kernel = 1;
  int stock_kernels = 1;
  int lpt = 1;
  size_t lpt_min_batch = kDefaultLptMinBatch;
  size_t latency_order_min = kDefaultLatencyOrderMin;
  int dump_threshold = -1;             // "handover_threshold"
  int fd_split = 1;
  size_t fd_split_min = 0, fd_split_max = 90112;
  int fd_split_pred = -1, fd_split_front = -1, fd_split_group_cut = -1;
  long long fd_split_samples = -1;
  int fd_head_rounds = kDefaultFdHeadRounds;
  size_t fd_head_min_batch = kDefaultFdHeadMinBatch;
  size_t analytic_small_batch = 8192;  // analytic mode: at or below, the sixteen-lanes-per-sample latency kernel alone
  int analytic_waves_per_cu = 12;      // ... persistent wavefronts of the lane-pair kernel per CU (142 registers, 13 KB of LDS: three per SIMD)
  int analytic_handover = 8;           // ... one of them hands over to the latency kernel once its tickets are gone and it holds at most this many samples (0: never)
  int scout_pairs = 1;
  int geodesic_flavour = 0, geodesic_order = 2;
  size_t geodesic_order_min = 2049, geodesic_scout_min = 2049; // (4096 / 6144 until round 5: the scout's order pays as soon as the blocks take tickets — tools/policy_check.py)
  int geodesic_scout_rounds = 64;
  double geodesic_long_steps = 12.0;
  int geodesic_group = 1;
  size_t geodesic_group_min = 13312;  // (16384 until round 5: tools/policy_check.py found the bulk form 10-12 % ahead at 15872 edges; crossover at 13312, profiles/r05_bulk_crossover.log)
  int geodesic_group_pred = -1, geodesic_group_low_cut = -1, geodesic_group_permille = 0, geodesic_group_handover_pct = -1;
  size_t clearance_per_state_max = 8192;
  int host_zero_copy = 2;
  int resident_idle_ms = 10;           // the resident service kernel leaves by itself after this long without a request
  int fail_after_fork = 0;             // debug build only (include/ccmp_debug.h): 1 / 2 = the split launches report a failure in front of / behind their side-stream part
  int debug_fail_calls = 0;            // debug build only: the next so many compute entry points return CCMP_EHIP before anything is launched
};

namespace ccmp_host {
/* the pinned, device-mapped block of the small *_host calls: its last 64 bytes hold the completion word */
constexpr size_t kPinBytes = 64 * 1024;
constexpr size_t kPinData = kPinBytes - 64;
/* single-state calls from the host entry points: the kernel publishes ctx->done_seq in the pinned block behind its result and
 * HostIO::finish polls that word (nullptr: this launch does not publish) */
inline unsigned int *arm_done_word(ccmp_ctx *ctx, size_t B)
{
  if (!ctx->want_done || B != 1 || !ctx->pin_dev) return nullptr;
  ctx->done_seq++;
  ctx->done_armed = true;
  return (unsigned int *)((char *)ctx->pin_dev + kPinData);
}
/* a workspace of the context (or of an object on it) at `n` units / `bytes` before anything that uses it is in flight: stops a resident
 * service kernel first (hipFree waits for the whole device), frees and reallocates; a no-op while *cap >= n (ccmp_api.cpp) */
int grow_buffer(ccmp_ctx *ctx, void **buf, size_t *cap, size_t n, size_t bytes);
/* check_problem of ccmp_api.cpp; what a connect call checks before its first launch; its gather -> traversal -> fix chain on the
 * neighbours in nbr_idx (ctx->connect_ws holds Q * k edges by then) — shared by ccmp_connect_batch and ccmp_roadmap_connect */
int problem_ok(const ccmp_problem *p);
int connect_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, int max_states, double *states, int32_t *n_states,
                   uint8_t *ok, double *carry_out, int round_budget, int check_target);
int connect_edges(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *nodes, const double *queries, size_t Q, int k,
                  int check_target, int max_states, int round_budget, const int32_t *nbr_idx, double *states, int32_t *n_states, uint8_t *ok,
                  int32_t *newton_iters, uint8_t *blocked, double *carry_out, void *hip_stream);
/* pose-targeted IK (ccmp_ik.cpp), shared with ccmp_roadmap_grow: the checks of a call (problem, options, S, the candidate count) and the
 * options as the kernels take them; the candidate count; the context's record workspace at that size; the launches of a checked call */
int ik_checks(const ccmp_problem *p, const ccmp_ik_opts *opts, size_t T, int S, ccmp::ik_params *P);
size_t ik_candidates(size_t T, int S, const ccmp::ik_params &P);
int ik_reserve(ccmp_ctx *ctx, size_t candidates);
int ik_launches(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp::ik_params &P, const double *poses, const double *seeds, size_t T, int S, uint64_t rng_seed,
                uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds, hipStream_t st);
/* the vetted IK (csrc/ccmp_ik_vet.h), shared with ccmp_roadmap_grow_vetted: what a call checks of its scene and margin; both workspaces
 * at the call's size; the launches of a checked call — ik_solve, ik_vet, ik_assemble, ccmp_clearance_batch on the slots, ik_pick */
int ik_vet_checks(const ccmp_ctx *ctx, const ccmp_scene *scene, double margin);
int ik_vetted_reserve(ccmp_ctx *ctx, size_t T, int S, const ccmp::ik_params &P);
int ik_vetted_launches(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp::ik_params &P, const double *poses, const double *seeds, size_t T, int S,
                       uint64_t rng_seed, uint64_t first_index, const ccmp_scene *scene, double margin, double *q_out, uint8_t *ok, int32_t *which,
                       double *cand_q, int32_t *cand_rounds, double *cand_clear, double *slot_clear, double *clearance, hipStream_t st);
/* device staging of the *_host conveniences, grown on demand */
int ensure_stage(ccmp_ctx *ctx, size_t bytes);
/* the device-visible alias of a caller's host range if all of it is page-locked and mapped (hipHostMalloc,
 * hipHostRegister), else nullptr; the calling thread's current device is the one that will use it */
void *pinned_alias(const void *host, size_t bytes);
/* runs fn(g) for g = 0..n-1, each on its own short-lived thread when n > 1 (one planner process driving several GPUs: a
 * copy from or to pageable memory blocks its caller, so shards issued from ONE thread start one after the other);
 * returns the first non-zero result and leaves that thread's error text in this thread's g_hip_err */
int for_each_shard(int n, int (*fn)(int g, void *arg), void *arg);
}  // namespace ccmp_host

#endif /* CCMP_CTX_H */
