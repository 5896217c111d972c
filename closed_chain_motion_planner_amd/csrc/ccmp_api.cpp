// ccmp_api.cpp — host side of libccmp: execution context, scheduling, argument checking and kernel launches
// (problem set-up lives in ccmp_problem.cpp).
//
// There is deliberately no CPU implementation of the hot path in this library: project / function /
// isSatisfied batches run on the GPU or fail with CCMP_ENODEV / CCMP_EHIP.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <set>

#include "../../include/ccmp.h"
#include "ccmp_ctx.h"
#include "ccmp_host.h"
#include "ccmp_launch.h"
#include "ccmp_policy.h"
#include "ccmp_resident.h"
#include "ccmp_scene.h"

using namespace ccmp_host;
using namespace ccmp_launch; // the queue words, the call-wide argument structs

namespace ccmp_host {
thread_local char g_hip_err[256] = "";
}  // namespace ccmp_host

namespace {

// A launch sequence that puts part of a call on the context's side stream.  fork() orders the side stream behind what the
// caller's stream holds; step() launches and remembers the FIRST failure instead of returning (later steps are skipped);
// side_done() marks the end of the side stream's part; join() ALWAYS orders the caller's stream behind the side stream — also
// when a step failed: the kernels already queued there write the caller's buffers and the context's queue words — and returns
// the call's result.
struct ForkJoin {
  ccmp_ctx *ctx;
  hipStream_t st;
  hipError_t err = hipSuccess;
  const char *what = nullptr;
  bool forked = false, recorded = false;
  ForkJoin(ccmp_ctx *c, hipStream_t s) : ctx(c), st(s) {}
  void fail(hipError_t e, const char *w) { if (err == hipSuccess && e != hipSuccess) { err = e; what = w; } }
  bool step(hipError_t e, const char *w) { fail(e, w); return err == hipSuccess; } // (FJ_STEP: not evaluated behind a failure)
  void fork()
  {
    if (err != hipSuccess) return;
    if (!step(hipEventRecord(ctx->fork, st), "hipEventRecord(fork)")) return;
    if (step(hipStreamWaitEvent(ctx->side, ctx->fork, 0), "hipStreamWaitEvent(side, fork)")) forked = true;
  }
  void side_done()
  {
    if (!forked || recorded) return;
    const hipError_t e = hipEventRecord(ctx->join, ctx->side); // (also behind a failed step: what reached the side stream must be joined)
    if (e == hipSuccess) recorded = true;
    fail(e, "hipEventRecord(join)");
  }
  int join()
  {
    if (forked) {
      side_done();
      if (recorded) fail(hipStreamWaitEvent(st, ctx->join, 0), "hipStreamWaitEvent(st, join)");
      else (void)hipStreamSynchronize(ctx->side); // the join event could not be recorded: the only ordering left is the host's
    }
    return err == hipSuccess ? CCMP_OK : hip_fail(err, what);
  }
};

#define FJ_STEP(fj, ...)                                                 \
  do {                                                                   \
    if ((fj).err == hipSuccess) (fj).fail((__VA_ARGS__), #__VA_ARGS__);  \
  } while (0)

int check_problem(const ccmp_problem *p)
{
  if (!p) return CCMP_EINVAL;
  if (!(p->tol_pos > 0) || !(p->tol_rot > 0)) return CCMP_EINVAL;
  if (p->max_iter < 0 || p->max_iter > 65535) return CCMP_EINVAL;
  if (p->jacobian_mode != CCMP_JAC_FD && p->jacobian_mode != CCMP_JAC_ANALYTIC) return CCMP_EINVAL;
  return CCMP_OK;
}

} // namespace

extern "C" {

int ccmp_version(void) { return CCMP_VERSION; }
size_t ccmp_problem_sizeof(void) { return sizeof(ccmp_problem); }
const char *ccmp_last_hip_error(void) { return g_hip_err; }

const char *ccmp_strerror(int code)
{
  switch (code) {
    case CCMP_OK: return "ok";
    case CCMP_EINVAL: return "invalid argument";
    case CCMP_EHIP: return "HIP runtime error";
    case CCMP_EIO: return "cannot read file";
    case CCMP_EPARSE: return "YAML key missing or malformed";
    case CCMP_ENODEV: return "no usable HIP device";
    case CCMP_ENOMEM: return "out of memory";
    case CCMP_ECOMM: return "RCCL error or librccl not loadable";
    case CCMP_EOVERFLOW: return "more valid states than the gather blocks hold";
    default: return "unknown error";
  }
}

// ---- context ---------------------------------------------------------------------------------------
// the contexts that exist (ccmp_host::context_alive): +1 registers, -1 removes, 0 asks
static bool live_contexts(const ccmp_ctx *ctx, int op)
{
  static std::mutex mu;
  static std::set<const ccmp_ctx *> live;
  std::lock_guard<std::mutex> hold(mu);
  if (op > 0) live.insert(ctx);
  else if (op < 0) live.erase(ctx);
  return live.count(ctx) != 0;
}

int ccmp_ctx_create(int device, ccmp_ctx **out)
{
  if (!out) return CCMP_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    snprintf(g_hip_err, sizeof g_hip_err, "hipGetDeviceCount: no HIP device");
    return CCMP_ENODEV;
  }
  if (device < 0 || device >= ndev) return CCMP_ENODEV;
  DeviceGuard guard(device);
  if (!guard.ok) return CCMP_ENODEV;
  ccmp_ctx *ctx = new (std::nothrow) ccmp_ctx();
  if (!ctx) return CCMP_ENOMEM;
  ctx->device = device;
  hipDeviceProp_t prop;
  hipError_t e = hipGetDeviceProperties(&prop, device);
  if (e != hipSuccess) { delete ctx; return hip_fail(e, "hipGetDeviceProperties"); }
  ctx->num_cus = prop.multiProcessorCount;
  e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
  if (e != hipSuccess) { delete ctx; return hip_fail(e, "hipStreamCreate"); }
  e = hipMalloc((void **)&ctx->queue, kQueueWords * sizeof(unsigned long long));
  if (e != hipSuccess) { (void)hipStreamDestroy(ctx->stream); delete ctx; return hip_fail(e, "hipMalloc(queue)"); }
  // side stream of the analytic mode's split launches (latency kernel beside the throughput kernel) and the two events
  // that order it against the caller's stream
  // The side stream must not share a hardware queue with the stream the caller launches on: HIP spreads streams over a
  // handful of hardware queues, and two streams on one queue run their kernels one after the other — seen with a second
  // context in the process, whose side stream landed on the NULL stream's queue: the split launch's front ran alone, in
  // front of the throughput kernel, and a 16 384-sample call took 2.34 ms instead of 1.68 (kernel trace).  Streams of another
  // PRIORITY get queues of their own, so the side stream takes the highest one (callers' streams are normal priority unless
  // they ask otherwise) — which also suits what runs there: the longest samples.
  {
    int prio_least = 0, prio_greatest = 0;
    e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
    if (e == hipSuccess && prio_greatest != prio_least) e = hipStreamCreateWithPriority(&ctx->side, hipStreamNonBlocking, prio_greatest);
    else e = hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking);
  }
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->gate, hipEventDisableTiming);
  if (e != hipSuccess) { ccmp_ctx_destroy(ctx); return hip_fail(e, "side stream / events"); }
  live_contexts(ctx, +1);
  *out = ctx;
  return CCMP_OK;
}

void ccmp_ctx_destroy(ccmp_ctx *ctx)
{
  if (!ctx) return;
  live_contexts(ctx, -1);
  DeviceGuard guard(ctx->device);
  ccmp_host::resident_destroy(ctx); // first: hipFree below waits for the whole device, a resident kernel included
  (void)hipStreamSynchronize(ctx->stream);
  if (ctx->geo_pool) (void)hipFree(ctx->geo_pool);
  if (ctx->knn_ws) (void)hipFree(ctx->knn_ws);
  if (ctx->retime_ws) (void)hipFree(ctx->retime_ws);
  if (ctx->connect_ws) (void)hipFree(ctx->connect_ws);
  if (ctx->ik_ws) (void)hipFree(ctx->ik_ws);
  if (ctx->ik_vet_ws) (void)hipFree(ctx->ik_vet_ws);
  if (ctx->queue) (void)hipFree(ctx->queue);
  if (ctx->pool) (void)hipFree(ctx->pool);
  if (ctx->fd_state) (void)hipFree(ctx->fd_state);
  if (ctx->lpt_buf) (void)hipFree(ctx->lpt_buf);
  if (ctx->scan) (void)hipFree(ctx->scan);
  if (ctx->stage) (void)hipFree(ctx->stage);
  if (ctx->pin) (void)hipHostFree(ctx->pin);
  if (ctx->side) { (void)hipStreamSynchronize(ctx->side); (void)hipStreamDestroy(ctx->side); }
  if (ctx->fork) (void)hipEventDestroy(ctx->fork);
  if (ctx->join) (void)hipEventDestroy(ctx->join);
  if (ctx->gate) (void)hipEventDestroy(ctx->gate);
  if (ctx->ev_shard) (void)hipEventDestroy(ctx->ev_shard);
  (void)hipStreamDestroy(ctx->stream);
  delete ctx;
}

int ccmp_ctx_set_waves_per_cu(ccmp_ctx *ctx, int w)
{
  if (!ctx || w < 0 || w > 32) return CCMP_EINVAL;
  ctx->waves_per_cu = w;
  return CCMP_OK;
}
int ccmp_ctx_set_schedule(ccmp_ctx *ctx, int wave_kernel, size_t small_batch)
{
  if (!ctx || wave_kernel < 0 || wave_kernel > 2) return CCMP_EINVAL;
  ctx->wave_kernel = wave_kernel;
  ctx->small_batch = small_batch == CCMP_DEFAULT ? kDefaultSmallBatch : small_batch;
  return CCMP_OK;
}
int ccmp_ctx_set_option(ccmp_ctx *ctx, const char *name, long value)
{
  if (!ctx || !name) return CCMP_EINVAL;
  if (!strcmp(name, "resident")) return ccmp_host::resident_set(ctx, value); // starts / stops the service kernel (ccmp_resident.cpp)
  return ccmp_host::policy_set_option(ctx, name, value); // the option table: ccmp_policy.cpp
}
int ccmp_ctx_set_lpt(ccmp_ctx *ctx, int mode, size_t min_batch)
{
  if (!ctx || mode < 0 || mode > 2) return CCMP_EINVAL;
  ctx->lpt = mode;
  ctx->lpt_min_batch = min_batch == CCMP_DEFAULT ? kDefaultLptMinBatch : min_batch;
  return CCMP_OK;
}
#ifdef CCMP_DEBUG_HOOKS // include/ccmp_debug.h: lib/libccmp_debug.so only
int ccmp_ctx_debug_lpt_pred(ccmp_ctx *ctx, uint16_t *host_out, size_t B)
{
  if (!ctx || !host_out || !ctx->lpt_buf || B > ctx->lpt_cap) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  ccmp_host::quiesce(ctx);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host_out, ctx->lpt_buf, B * sizeof(uint16_t), hipMemcpyDeviceToHost));
  return CCMP_OK;
}
int ccmp_ctx_set_order_experimental(ccmp_ctx *ctx, const unsigned int *order_dev)
{
  if (!ctx) return CCMP_EINVAL;
  ctx->order = order_dev;
  return CCMP_OK;
}
int ccmp_debug_fail_calls(ccmp_ctx *ctx, int n)
{
  if (!ctx || n < 0) return CCMP_EINVAL;
  ctx->debug_fail_calls = n;
  return CCMP_OK;
}
#endif
int ccmp_ctx_device(const ccmp_ctx *ctx) { return ctx ? ctx->device : -1; }
int ccmp_ctx_num_cus(const ccmp_ctx *ctx) { return ctx ? ctx->num_cus : 0; }

#ifdef CCMP_DEBUG_HOOKS
#define CCMP_DEBUG_FAIL_POINT() if (ctx->debug_fail_calls > 0) { ctx->debug_fail_calls--; return CCMP_EHIP; }
#define CCMP_FAIL_AFTER_FORK(fj, where) if (ctx->fail_after_fork == (where)) (fj).fail(hipErrorLaunchFailure, "fail_after_fork (debug option)")
#else
#define CCMP_DEBUG_FAIL_POINT()
#define CCMP_FAIL_AFTER_FORK(fj, where)
#endif
#define CCMP_PROLOGUE()                                        \
  if (!ctx) return CCMP_EINVAL;                                \
  CCMP_DEBUG_FAIL_POINT()                                      \
  { int rc_ = check_problem(p); if (rc_ != CCMP_OK) return rc_; } \
  DeviceGuard guard(ctx->device);                              \
  if (!guard.ok) return CCMP_ENODEV;                           \
  hipStream_t st = (hipStream_t)hip_stream; \
  ccmp_consts K;                                               \
  ccmp_host::make_consts(*p, K);                               \
  if (!ctx->stock_kernels) K.stock = K.twin_arms = K.rot_x0 = 0

int ccmp_function_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, double *f, size_t B, void *hip_stream)
{
  CCMP_PROLOGUE();
  if (B == 0) return CCMP_OK;
  if (!q || !f) return CCMP_EINVAL;
  unsigned int *flag = arm_done_word(ctx, B);
  HIP_TRY(ccmp_launch::function(&K, q, f, B, flag, ctx->done_seq, st));
  return CCMP_OK;
}

// workspaces owned by the context: below n units (*cap) *buf is replaced by `bytes` new bytes.  They grow outside any stream
// capture (the first call at a size is never captured) and after a resident service kernel has left (hipFree waits for it)
extern "C++" {
namespace ccmp_host {
int grow_buffer(ccmp_ctx *ctx, void **buf, size_t *cap, size_t n, size_t bytes)
{
  if (*cap >= n) return CCMP_OK;
  ccmp_host::quiesce(ctx);
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *cap = 0;
  HIP_TRY(hipMalloc(buf, bytes));
  *cap = n;
  return CCMP_OK;
}
}  // namespace ccmp_host
}  // extern "C++"
static int grow(ccmp_ctx *ctx, void **buf, size_t *cap, size_t n, size_t bytes) { return ccmp_host::grow_buffer(ctx, buf, cap, n, bytes); }
static int ensure_pool(ccmp_ctx *ctx, size_t records) { return grow(ctx, (void **)&ctx->pool, &ctx->pool_cap, records, records * kPoolEntry * sizeof(double)); }
// head -> resume workspace: one row per sample — a staged record on stock twin arms (ccmp_launch.h: kStagedRow doubles, 1.26 KB: 331 MB at
// 262 144 samples), the hand-over's record otherwise (kPoolEntry).  false: the device has no room for it — the caller runs the call as
// the one-launch whole kernel, which needs none
static bool ensure_fd_state(ccmp_ctx *ctx, size_t B, int row_doubles)
{
  const size_t doubles = B * (size_t)row_doubles;
  if (ctx->fd_state_cap >= doubles) return true;
  ccmp_host::quiesce(ctx);
  if (ctx->fd_state) (void)hipFree(ctx->fd_state);
  ctx->fd_state = nullptr;
  ctx->fd_state_cap = 0;
  if (hipMalloc((void **)&ctx->fd_state, doubles * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError(); // out of memory is this function's answer, not the call's error
    ctx->fd_state = nullptr;
    return false;
  }
  ctx->fd_state_cap = doubles;
  return true;
}
static int ensure_lpt_buffers(ccmp_ctx *ctx, size_t B) // pred u16 | hist 1024 x u32 | order u32 | flags u8 (bulk checkMotion)
{
  return grow(ctx, &ctx->lpt_buf, &ctx->lpt_cap, B, ((B * 2 + 255) & ~(size_t)255) + 4096 + B * 4 + B);
}

// the scout's workspace inside ctx->lpt_buf: pred (u16 x cap) | hist (u32 x 1024) | order (u32 x cap) | flags (u8 x cap)
struct ScoutBuffers {
  uint16_t *pred;
  unsigned int *hist, *order;
  explicit ScoutBuffers(const ccmp_ctx *ctx)
  {
    char *base = (char *)ctx->lpt_buf;
    pred = (uint16_t *)base;
    hist = (unsigned int *)(base + ((ctx->lpt_cap * 2 + 255) & ~(size_t)255));
    order = (unsigned int *)((char *)hist + 4096);
  }
};

static int project_common(ccmp_ctx *ctx, const ccmp_problem *p, int mode, const double *q_in, double *q_out,
                          uint8_t *ok, uint16_t *iters, double *q_ambient, size_t B, uint64_t seed, uint64_t first,
                          void *hip_stream)
{
  CCMP_PROLOGUE();
  if (B == 0) return CCMP_OK;
  if (!q_out || !ok || (mode == 0 && !q_in)) return CCMP_EINVAL;
  if ((((uintptr_t)q_in) | ((uintptr_t)q_out)) & 15u) return CCMP_EINVAL; // rows are moved in 16-byte pieces
  const ProjectCall c{&K, mode, q_in, q_out, ok, iters, q_ambient, B, seed, first};
  const int scout_pair_blocks = ctx->scout_pairs ? ctx->num_cus * kScoutPairBlocksPerCu : 0;
  if (p->jacobian_mode != CCMP_JAC_FD) { // analytic mode: the plan is ccmp_policy.cpp's plan_analytic_batch
    const AnalyticPlan pl = ccmp_host::plan_analytic_batch(ctx, B);
    if (pl.pool_records > 0) {
      int rc = ensure_pool(ctx, pl.pool_records); // sized before anything of the call is in flight
      if (rc != CCMP_OK) return rc;
    }
    HIP_TRY(ccmp_launch::project_analytic(c, pl.pair_blocks, pl.dump, pl.latency_blocks, ctx->pool, ctx->queue + kQAnalytic, st));
    return CCMP_OK;
  }
  // Reference arithmetic.  sampleUniform on arms WITHOUT the stock structure (calibrated arms, tilted bases) is not fused: the
  // ambient sampler writes the states, the projector runs on them in place, enforceBounds wraps them — the same values through
  // 60 MB more traffic at C3 (0.03 ms beside a 20 ms kernel).  The fused general instantiation project_fd_kernel<1, false>
  // spilled 2.3 KB per lane (its sampler prologue and the general chain's pose arrays overlap) and was removed in round 6.
  if (mode == 1 && !(K.stock && K.twin_arms)) {
    double *amb = q_ambient ? q_ambient : q_out;
    HIP_TRY(ccmp_launch::ambient_uniform(&K, seed, first, amb, B, st));
    const int rc = project_common(ctx, p, 0, amb, q_out, ok, iters, nullptr, B, seed, first, hip_stream);
    if (rc != CCMP_OK) return rc;
    HIP_TRY(ccmp_launch::enforce_bounds(q_out, B, st));
    return CCMP_OK;
  }
  // the plan is ccmp_policy.cpp's plan_fd_batch (what ccmp_ctx_describe prints)
  FdPlan pl = ccmp_host::plan_fd_batch(ctx, B, ctx->order != nullptr);
  // every workspace of the call is sized before anything of it is in flight
  if (pl.scout || pl.latency_order) {
    int rc = ensure_lpt_buffers(ctx, B);
    if (rc != CCMP_OK) return rc;
  }
  if (pl.handover) {
    int rc = ensure_pool(ctx, (size_t)pl.group_blocks * 10);
    if (rc != CCMP_OK) return rc;
  }
  if (pl.head_rounds > 0 && !ensure_fd_state(ctx, B, K.stock && K.twin_arms ? ccmp_launch::kStagedRow : kPoolEntry)) pl.head_rounds = 0; // no room for the staged records: one launch, the same bits
  unsigned long long *const q_pool_count = ctx->queue + kQPool, *const q_latency = ctx->queue + kQLatency;
  if (!pl.latency_static) HIP_TRY(ccmp_launch::clear_words(ctx->queue, 16, st)); // the projector's eight queue words

  if (pl.group_blocks == 0) { // small batches and single states
    if (ctx->flat_kernel) {
      unsigned int *flag = arm_done_word(ctx, B);
      const unsigned int *lat_order = nullptr;
      // (Round 6 measured and dropped a head start — the first resident-blocks samples in index order on this stream while scout
      // and sort of the rest, and then the rest, ran on the side stream: 4 096 Wine_Bottle samples 0.656 -> 0.704 ms, stefan 0.977 ->
      // 1.163 ms over six seeds, bit-identical; the longest sample is as likely in the rest, where it then starts later than behind
      // the scout — profiles/r06_head_start_ab.log.)
      if (pl.latency_order) { // longest-predicted-first on the latency kernel alone
        const ScoutBuffers sb(ctx);
        HIP_TRY(ccmp_launch::scout_order(c, sb.pred, sb.hist, sb.order, ctx->queue + kQScout, ctx->num_cus * kScoutBlocksPerCu, scout_pair_blocks, nullptr, st));
        lat_order = sb.order;
      }
      HIP_TRY(ccmp_launch::project_flat(c, {.blocks = pl.latency_blocks, .queue = pl.latency_static ? nullptr : q_latency, .pool = ctx->pool,
                                            .pool_count = q_pool_count, .order = lat_order, .done_flag = flag, .done_seq = ctx->done_seq}, st));
    }
    else
      HIP_TRY(ccmp_launch::project_wave(c, false, pl.latency_blocks, q_latency, ctx->pool, q_pool_count, st));
    return CCMP_OK;
  }

  const unsigned int *order = ctx->order;
  const uint16_t *pred = nullptr;
  ForkJoin fj(ctx, st);
  // Head and resume (ccmp_kernels_fd.hip: FdPart): every sample's first rounds, ten samples of one age per wavefront in index order,
  // then the persistent kernel on the rows those left in ctx->fd_state.  The scout pass reads q_in alone and runs beside the head.  The
  // head's workgroups keep every wavefront slot of the chip taken until its last generation, and a kernel dispatched behind them waits
  // for wavefronts to retire one by one (the scout pass then ends 0.23 ms after the head; the sort's small kernels took 3 ms).  So the
  // scout pass must be dispatched FIRST: it goes to the side stream, and the head waits for an event that the side stream records in
  // front of the scout pass (`gate`) — one signal further away than the scout pass itself.  The scout takes two wavefronts per SIMD for
  // its 0.34 ms and leaves the head the rest; the sort runs once both are done, in front of the resume launch.  (The orders this one
  // was measured against — scout and sort in front, an ungated side stream, a side stream of lowest priority: DESIGN_experiments.md §5.6.)
  // A call IN PLACE (q_out on q_in, include/ccmp.h) keeps the scout in front: the head writes back the samples that end within its
  // rounds, and beside it the scout pass would read rows that are being overwritten — the order would still be a permutation and the
  // results the same bits, but the schedule would differ from run to run.
  if (pl.head_rounds > 0) {
    const int head_blocks = (int)((B + 9) / 10);
    const bool in_place = mode == 0 && q_in < q_out + B * 14 && q_out < q_in + B * 14;
    if (pl.scout) {
      const ScoutBuffers sb(ctx);
      const int scout_blocks = ctx->num_cus * kScoutBlocksPerCu;
      unsigned long long *const q_scout = ctx->queue + kQScout;
      order = sb.order;
      if (in_place) {
        HIP_TRY(ccmp_launch::scout_order(c, sb.pred, sb.hist, sb.order, q_scout, scout_blocks, scout_pair_blocks, nullptr, st));
        HIP_TRY(ccmp_launch::project_group(c, head_blocks, ctx->queue, nullptr, pl.dump_threshold, nullptr, nullptr, 0, 0, st, kFdHead, ctx->fd_state, pl.head_rounds));
      } else {
        HIP_TRY(ccmp_launch::scout_order(c, sb.pred, sb.hist, sb.order, q_scout, scout_blocks, scout_pair_blocks, nullptr, st, kScoutClear));
        fj.fork();
        FJ_STEP(fj, hipEventRecord(ctx->gate, ctx->side));
        FJ_STEP(fj, ccmp_launch::scout_order(c, sb.pred, sb.hist, sb.order, q_scout, scout_blocks, scout_pair_blocks, nullptr, ctx->side, kScoutPass));
        FJ_STEP(fj, hipStreamWaitEvent(st, ctx->gate, 0));
        FJ_STEP(fj, ccmp_launch::project_group(c, head_blocks, ctx->queue, nullptr, pl.dump_threshold, nullptr, nullptr, 0, 0, st, kFdHead, ctx->fd_state, pl.head_rounds));
        const int rc = fj.join();
        if (rc != CCMP_OK) return rc;
        HIP_TRY(ccmp_launch::scout_order(c, sb.pred, sb.hist, sb.order, q_scout, scout_blocks, scout_pair_blocks, nullptr, st, kScoutSort));
      }
    } else
      HIP_TRY(ccmp_launch::project_group(c, head_blocks, ctx->queue, nullptr, pl.dump_threshold, nullptr, nullptr, 0, 0, st, kFdHead, ctx->fd_state, pl.head_rounds));
    HIP_TRY(ccmp_launch::project_group(c, pl.group_blocks, ctx->queue, nullptr, pl.dump_threshold, order, nullptr, 0, 0, st, kFdResume, ctx->fd_state, pl.head_rounds));
    return CCMP_OK;
  }
  if (pl.scout) { // FP32 scout pass -> predicted iteration counts -> descending counting sort -> processing order
    const ScoutBuffers sb(ctx);
    // up to two 256-thread blocks per CU (kScoutBlocksPerCu): a wavefront owns a contiguous slice of the batch — 128 samples at
    // 262144 — and its lanes refill from it, so a second wavefront per SIMD no longer lengthens the launch by its unluckiest lane;
    // it halves the drain at the end of the slices (262144 samples: 0.362 ms at one block per CU, 0.336 at two, 0.387 at three)
    // (a split launch's cut of the order — fd_split_kernel's rule — is decided by the sort's own kernel: ccmp_launch.h, ccmp_split_req)
    const ccmp_split_req cut{ctx->queue, 1, pl.shape.pred, 0, 0, pl.shape.samples, 0};
    HIP_TRY(ccmp_launch::scout_order(c, sb.pred, sb.hist, sb.order, ctx->queue + kQScout, ctx->num_cus * kScoutBlocksPerCu, scout_pair_blocks, pl.split ? &cut : nullptr, st));
    order = sb.order;
    // hand-over in two classes (scout's prediction minus the iterations done): the pool is filled from both ends and the
    // latency kernel takes the long samples first
    if (pl.two_class_pool) pred = sb.pred;
    // Split launch (round 4).  A mid-size batch ends on the serial chain of its longest samples: they start first in the
    // throughput kernel, do ~22 iterations there at 26-62 us each, and only after the hand-over — a millisecond into the call —
    // go on at the latency kernel's pace.  With the split the front of the order runs on latency blocks on the side stream FROM
    // THE START, beside the throughput kernel, which takes the rest of the order with a few wavefronts per CU fewer and hands
    // over as before.  From the fork on a failure is reported only after the side stream has been joined back (ForkJoin).
    if (pl.split) {
      fj.fork();
      CCMP_FAIL_AFTER_FORK(fj, 1);
      FJ_STEP(fj, ccmp_launch::project_flat(c, {.blocks = pl.shape.blocks, .queue = ctx->queue + kQFront, .pool = ctx->pool, .pool_count = q_pool_count,
                                                .order = sb.order, .total = ctx->queue + kQFrontLen}, ctx->side));
      fj.side_done();
      CCMP_FAIL_AFTER_FORK(fj, 2);
    }
  }
  const size_t pool_records = pred ? (size_t)pl.group_blocks * 10 : 0;
  FJ_STEP(fj, ccmp_launch::project_group(c, pl.group_blocks, ctx->queue, pl.handover ? ctx->pool : nullptr, pl.dump_threshold, order, pred,
                                         kPoolLongRemaining, pool_records, st));
  if (pl.handover) { // the pool's fill count is read on the device: the latency kernel's surplus blocks exit at once
    if (ctx->flat_kernel)
      FJ_STEP(fj, ccmp_launch::project_flat(c, {.blocks = pl.latency_blocks, .queue = q_latency, .from_pool = true, .pool = ctx->pool,
                                                .pool_count = q_pool_count, .pool_records = pool_records}, st));
    else
      FJ_STEP(fj, ccmp_launch::project_wave(c, true, pl.latency_blocks, q_latency, ctx->pool, q_pool_count, st));
  }
  return fj.join(); // the call is complete on `st` when the front is
}

int ccmp_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q_in, double *q_out, uint8_t *ok,
                       uint16_t *iters, size_t B, void *hip_stream)
{
  return project_common(ctx, p, 0, q_in, q_out, ok, iters, nullptr, B, 0, 0, hip_stream);
}

int ccmp_sample_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index, double *q_out,
                              uint8_t *ok, uint16_t *iters, double *q_ambient, size_t B, void *hip_stream)
{
  return project_common(ctx, p, 1, nullptr, q_out, ok, iters, q_ambient, B, seed, first_index, hip_stream);
}

static int sample_ref_common(ccmp_ctx *ctx, const ccmp_problem *p, int kind, uint64_t seed, uint64_t first_index,
                             const double *ref, int ref_stride, double param, double *q_out, uint8_t *ok, uint16_t *iters,
                             double *q_ambient, size_t B, void *hip_stream)
{
  if (!ctx || !p) return CCMP_EINVAL;
  if (B == 0) return CCMP_OK;
  if (!ref || !q_out || !ok || (ref_stride != 0 && ref_stride != 14) || !(param >= 0)) return CCMP_EINVAL;
  {
    CCMP_PROLOGUE();
    HIP_TRY(ccmp_launch::ambient_ref(&K, kind, seed, first_index, ref, ref_stride, param, q_out, B, st));
    if (q_ambient) HIP_TRY(hipMemcpyAsync(q_ambient, q_out, B * 14 * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  int rc = ccmp_project_batch(ctx, p, q_out, q_out, ok, iters, B, hip_stream);
  if (rc != CCMP_OK) return rc;
  return ccmp_enforce_bounds_batch(ctx, q_out, B, hip_stream);
}

int ccmp_sample_near_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                                   const double *near, int near_stride, double distance, double *q_out, uint8_t *ok,
                                   uint16_t *iters, double *q_ambient, size_t B, void *hip_stream)
{
  return sample_ref_common(ctx, p, 0, seed, first_index, near, near_stride, distance, q_out, ok, iters, q_ambient, B, hip_stream);
}

int ccmp_sample_gaussian_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                                       const double *mean, int mean_stride, double std_dev, double *q_out, uint8_t *ok,
                                       uint16_t *iters, double *q_ambient, size_t B, void *hip_stream)
{
  return sample_ref_common(ctx, p, 1, seed, first_index, mean, mean_stride, std_dev, q_out, ok, iters, q_ambient, B, hip_stream);
}

int ccmp_compute_t_wo_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, int q_stride, double *t_wo, size_t B,
                            void *hip_stream)
{
  CCMP_PROLOGUE();
  if (B == 0) return CCMP_OK;
  if (!q || !t_wo || q_stride < 7) return CCMP_EINVAL;
  HIP_TRY(ccmp_launch::t_wo(&K, q, q_stride, t_wo, B, st));
  return CCMP_OK;
}

// the arguments of an extend-step call (E > 0) that every form of it checks
static int geodesic_args(const ccmp_problem *p, const double *from, const double *to, int max_states, double *states, int32_t *n_states,
                         uint8_t *ok, const double *carry_in, double *carry_out, int round_budget, int check_target)
{
  if (!from || !to || !states || !n_states || !ok || max_states < 1 || round_budget < 0) return CCMP_EINVAL;
  if (!(p->delta > 0) || !(p->lambda > 0)) return CCMP_EINVAL;
  if (carry_in && check_target) return CCMP_EINVAL;        // a continuation's target was tested by the call it continues
  if (round_budget > 0 && !carry_out) return CCMP_EINVAL;  // a suspended edge is useless without what its continuation needs
  // a resumable call needs room for one state besides `from`: with a one-entry list the first accepted state already reports
  // max_states + 1 with `from` as its last stored state, and a caller following the protocol would continue from `from` for ever
  if ((carry_in || carry_out || round_budget > 0) && max_states < 2) return CCMP_EINVAL;
  return CCMP_OK;
}

static int geodesic_common(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                           double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, const double *carry_in,
                           double *carry_out, int round_budget, int check_target, void *hip_stream)
{
  CCMP_PROLOGUE();
  if (E == 0) return CCMP_OK;
  { const int rc = geodesic_args(p, from, to, max_states, states, n_states, ok, carry_in, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; }
  const GeoCall g{&K, p->delta, p->lambda, from, to, E, max_states, states, n_states, ok, newton_iters, carry_in, carry_out, round_budget, check_target};
  if (p->jacobian_mode != CCMP_JAC_FD) {
    // Analytic mode: one launch of the traversal kernel on the analytic latency kernel's layout (ccmp_kernels_fast.hip:
    // geodesic_row16_kernel — four edges per wavefront, ticket queue, isSatisfied(to), the round budget and the carries inside);
    // no workspace, no host synchronisation, capturable.  ccmp_policy.cpp: plan_geodesic_analytic — what ccmp_ctx_describe prints.
    HIP_TRY(ccmp_launch::geodesic_analytic(g, ccmp_host::plan_geodesic_analytic(ctx, E), ctx->queue + kQGeoAnalytic, st));
    return CCMP_OK;
  }
  // what the call is going to launch is decided (ccmp_policy.cpp: plan_geodesic — what ccmp_ctx_describe prints) and every workspace
  // it needs is sized before anything of it is in flight
  const GeoPlan pl = ccmp_host::plan_geodesic(ctx, E, round_budget, carry_in != nullptr);
  unsigned long long *queue = nullptr;
  const unsigned int *order = nullptr;
  if (pl.ordered) {
    int rc = ensure_lpt_buffers(ctx, E);
    if (rc != CCMP_OK) return rc;
  }
  if (pl.bulk && pl.handover_pct > 0) {
    int rc = grow(ctx, (void **)&ctx->geo_pool, &ctx->geo_pool_cap, pl.group_waves * 10, pl.group_waves * 10 * kGeoPoolEntry * sizeof(double));
    if (rc != CCMP_OK) return rc;
  }
  if (pl.queued) {
    queue = ctx->queue + kQGeoTicket;
    HIP_TRY(ccmp_launch::clear_words(queue, 4, st)); // the ticket and the ordering pass's counters
    if (pl.ordered) {
      const ScoutBuffers sb(ctx);
      if (pl.scouted) {
        // FP32 scout of every edge (the traversal in single precision with the exact Jacobian, one edge per lane, rounds
        // capped) -> predicted Newton rounds -> descending counting sort: longest-predicted-first
        // (a bulk call's default cut of the order — apply_split's kind 2, ccmp_kernels_scout.hip — is decided, and the launch's block of queue words
        // cleared, by the sort's own kernel: ccmp_launch.h, ccmp_split_req)
        const ccmp_split_req cut{ctx->queue + kQBulk, 2, pl.low_cut, 64, kGeoGroupHeavyPermille, 0u, 8};
        HIP_TRY(ccmp_launch::geodesic_scout_order(g, ctx->geodesic_scout_rounds, sb.pred, sb.hist, sb.order, pl.scout_pairs,
                                                  pl.bulk && pl.default_cut ? &cut : nullptr, st));
      } else {
        HIP_TRY(ccmp_launch::geodesic_order(from, to, E, ctx->geodesic_long_steps * p->delta, (unsigned int *)(ctx->queue + kQGeoOrder), sb.order, st));
      }
      order = sb.order;
    }
  }
  // Bulk calls (round budget, thousands of edges, scout order): the SHORT edges run on the throughput layout — ten edges per
  // wavefront, geodesic_group_kernel, less than half the instructions per Newton round — and the front of the order on this
  // kernel's blocks on the side stream, both from the start.
  if (pl.bulk) {
    unsigned long long *gq = ctx->queue + kQBulk; // words: BulkWord
    const ScoutBuffers sb(ctx);
    const int pct = pl.handover_pct;
    if (!pl.default_cut) HIP_TRY(ccmp_launch::clear_words(gq, 16, st));
    // checkMotion: isSatisfied(to) of every edge up front (one lane per edge) for the group kernel; the front's blocks test their own
    uint8_t *target_ok = nullptr;
    if (check_target) {
      target_ok = (uint8_t *)sb.hist + 4096 + ctx->lpt_cap * 4;
      HIP_TRY(ccmp_launch::is_satisfied(&K, to, target_ok, E, nullptr, 0, st));
    }
    // the cut of the order: by default one of two, by what the batch looks like — at the scout's cap where the edges beyond it carry
    // a tenth of the predicted work (stefan, dumbbell), lower where they do not (Wine_Bottle) — decided by the sort's kernel above;
    // the options that fix it themselves get a launch of their own
    if (ctx->geodesic_group_permille > 0)
      HIP_TRY(ccmp_launch::geo_split(sb.hist, 8, ctx->geodesic_group_pred > 0 ? ctx->geodesic_group_pred : 64, ctx->geodesic_group_permille, gq, st));
    else if (ctx->geodesic_group_pred > 0)
      HIP_TRY(ccmp_launch::fd_split(sb.hist, ctx->geodesic_group_pred, 0xffffffffu, gq, st));
    // Fork.  From here on a failure no longer returns at once: whatever was queued on the side stream is joined back into the
    // caller's stream first (an early return left the side stream's kernels writing the caller's buffers unordered against
    // `st`), then the first error is reported.
    ForkJoin fj(ctx, st);
    fj.fork();
    CCMP_FAIL_AFTER_FORK(fj, 1);
    FJ_STEP(fj, ccmp_launch::geodesic(g, {.blocks = pl.front_blocks, .queue = gq + kBFront, .order = order, .total = gq + kBFrontLen}, ctx->side));
    fj.side_done();
    CCMP_FAIL_AFTER_FORK(fj, 2);
    FJ_STEP(fj, ccmp_launch::geodesic_group(g, (int)pl.group_waves, gq + kBTicket, order, pct > 0 ? ctx->geo_pool : nullptr, gq + kBPool, pct,
                                            target_ok, st));
    if (pct > 0) { // the handed-over edges: latency blocks behind the group kernel; the pool's fill count is read on the device
      GeoCall drain = g; // the pool's records: not the call's targets to test, order or carries to read
      drain.check_target = 0;
      drain.carry_in = nullptr;
      FJ_STEP(fj, ccmp_launch::geodesic(drain, {.blocks = pl.drain_blocks, .queue = gq + kBDrain, .order = nullptr, .pool = ctx->geo_pool,
                                                .pool_count = gq + kBPool}, st));
    }
    return fj.join();
  }
  HIP_TRY((pl.latency_flavour ? ccmp_launch::geodesic_lat : ccmp_launch::geodesic)(g, {.blocks = (int)pl.blocks, .queue = queue, .order = order}, st));
  return CCMP_OK;
}

int ccmp_geodesic_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                        double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, void *hip_stream)
{
  return geodesic_common(ctx, p, from, to, E, max_states, states, n_states, ok, newton_iters, nullptr, nullptr, 0, 0, hip_stream);
}

int ccmp_check_motion_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                            double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, void *hip_stream)
{
  return geodesic_common(ctx, p, from, to, E, max_states, states, n_states, ok, newton_iters, nullptr, nullptr, 0, 1, hip_stream);
}

int ccmp_geodesic_batch_ex(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                           double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, const double *carry_in,
                           double *carry_out, int round_budget, int check_target, void *hip_stream)
{
  return geodesic_common(ctx, p, from, to, E, max_states, states, n_states, ok, newton_iters, carry_in, carry_out, round_budget,
                         check_target, hip_stream);
}

// The extend step with the StateValidityChecker's proxy pre-filter on the device: one launch of the scene variant of the mode's
// traversal kernel (FD: geodesic_scene_kernel, the latency build's persistent blocks on a ticket; analytic: geodesic_row16_scene_kernel).
// Never the bulk form, never the resident service.  ccmp_policy.cpp: plan_geodesic_scene — what ccmp_ctx_describe prints.
int ccmp_geodesic_scene_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *from, const double *to,
                              size_t E, int max_states, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                              double *clearance, const double *carry_in, double *carry_out, int round_budget, int check_target, void *hip_stream)
{
  CCMP_PROLOGUE();
  if (!scene || scene->device != ctx->device || std::isnan(margin)) return CCMP_EINVAL;
  if (E == 0) return CCMP_OK;
  { const int rc = geodesic_args(p, from, to, max_states, states, n_states, ok, carry_in, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; }
  const GeoCall g{&K, p->delta, p->lambda, from, to, E, max_states, states, n_states, ok, newton_iters, carry_in, carry_out, round_budget, check_target};
  const ccmp_launch::GeoScene sg{scene->dev, margin, blocked, clearance};
  const int blocks = ccmp_host::plan_geodesic_scene(ctx, E, p->jacobian_mode != CCMP_JAC_FD);
  if (p->jacobian_mode != CCMP_JAC_FD) HIP_TRY(ccmp_launch::geodesic_analytic_scene(g, sg, blocks, ctx->queue + kQGeoAnalytic, st));
  else HIP_TRY(ccmp_launch::geodesic_scene(g, sg, blocks, ctx->queue + kQGeoTicket, st));
  return CCMP_OK;
}

// ---- the connection step -------------------------------------------------------------------------------
// what every form of a k-NN call checks (Q > 0 behind it)
static int knn_args(const double *nodes, size_t N, const double *queries, size_t Q, int k, int mode, const int32_t *nbr_idx)
{
  if (k < 1 || k > CCMP_KNN_MAX_K || mode < CCMP_KNN_ALL || mode > CCMP_KNN_EARLIER) return CCMP_EINVAL;
  if (N >= ((size_t)1 << 31) || Q >= ((size_t)1 << 31)) return CCMP_EINVAL; // indices are int32; one merge block per query
  if (Q > 0 && (!queries || !nbr_idx || (N > 0 && !nodes))) return CCMP_EINVAL;
  return CCMP_OK;
}

// the launches of a k-NN call whose arguments are checked and whose workspace has its size (ccmp_policy.cpp: plan_knn)
static int knn_launches(ccmp_ctx *ctx, const KnnCall &c, const KnnShape &s, hipStream_t st)
{
  HIP_TRY(ccmp_launch::knn(c, s, ctx->knn_ws, st));
  return CCMP_OK;
}

int ccmp_knn_batch(ccmp_ctx *ctx, const double *nodes, size_t N, const double *queries, size_t Q, int k, int mode, size_t self_base,
                   int32_t *nbr_idx, double *nbr_dist, void *hip_stream)
{
  if (!ctx) return CCMP_EINVAL;
  CCMP_DEBUG_FAIL_POINT()
  { const int rc = knn_args(nodes, N, queries, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (Q == 0) return CCMP_OK;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  const KnnShape s = ccmp_host::plan_knn(ctx, Q, N, k);
  { const int rc = grow(ctx, &ctx->knn_ws, &ctx->knn_ws_cap, s.workspace_bytes, s.workspace_bytes); if (rc != CCMP_OK) return rc; }
  return knn_launches(ctx, KnnCall{nodes, N, queries, Q, k, mode, self_base, nbr_idx, nbr_dist}, s, (hipStream_t)hip_stream);
}

// What a connect call (ccmp_connect_batch, ccmp_roadmap_connect) checks besides its k-NN arguments, before anything is launched: the
// problem, the scene, and the traversal's own arguments (geodesic_args on the workspace's endpoints, which are never NULL).
extern "C++" {
namespace ccmp_host {
int problem_ok(const ccmp_problem *p) { return check_problem(p); }
int connect_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, int max_states, double *states, int32_t *n_states,
                   uint8_t *ok, double *carry_out, int round_budget, int check_target)
{
  { const int rc = check_problem(p); if (rc != CCMP_OK) return rc; }
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
  static const double endpoint = 0.0; // stands for the gathered endpoints
  return geodesic_args(p, &endpoint, &endpoint, max_states, states, n_states, ok, nullptr, carry_out, round_budget, check_target);
}

// The edges of a connect call whose neighbours are in nbr_idx (on the stream, behind the k-NN): gather into ctx->connect_ws (grown by
// the caller to E edges before its first launch), the traversal the caller would have run on the gathered pairs (geodesic_common, or
// the scene variant's entry point, both unchanged), then the empty slots' values.
int connect_edges(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *nodes, const double *queries, size_t Q, int k,
                  int check_target, int max_states, int round_budget, const int32_t *nbr_idx, double *states, int32_t *n_states, uint8_t *ok,
                  int32_t *newton_iters, uint8_t *blocked, double *carry_out, void *hip_stream)
{
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t E = Q * (size_t)k;
  double *from = ctx->connect_ws, *to = ctx->connect_ws + E * 14;
  HIP_TRY(ccmp_launch::connect_gather(nodes, queries, nbr_idx, E, k, from, to, st));
  int rc;
  if (scene)
    rc = ccmp_geodesic_scene_batch(ctx, p, scene, margin, from, to, E, max_states, states, n_states, ok, newton_iters, blocked, nullptr, nullptr,
                                   carry_out, round_budget, check_target, hip_stream);
  else {
    rc = geodesic_common(ctx, p, from, to, E, max_states, states, n_states, ok, newton_iters, nullptr, carry_out, round_budget, check_target, hip_stream);
    if (rc == CCMP_OK && blocked) HIP_TRY(hipMemsetAsync(blocked, 0, E, st)); // no scene refuses anything
  }
  if (rc != CCMP_OK) return rc;
  HIP_TRY(ccmp_launch::connect_fix(nbr_idx, E, n_states, ok, newton_iters, blocked, carry_out, st));
  return CCMP_OK;
}
}  // namespace ccmp_host
}  // extern "C++"

// k-NN, then ccmp_host::connect_edges.  One stream, no host synchronisation; both workspaces of its own have their size
// before the first launch.
int ccmp_connect_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *nodes, size_t N,
                       const double *queries, size_t Q, int k, int mode, size_t self_base, int check_target, int max_states, int round_budget,
                       int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                       double *carry_out, void *hip_stream)
{
  if (!ctx) return CCMP_EINVAL;
  CCMP_DEBUG_FAIL_POINT()
  { const int rc = check_problem(p); if (rc != CCMP_OK) return rc; }
  { const int rc = knn_args(nodes, N, queries, Q, k, mode, nbr_idx); if (rc != CCMP_OK) return rc; }
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
  if (Q == 0) return CCMP_OK;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t E = Q * (size_t)k;
  const KnnShape s = ccmp_host::plan_knn(ctx, Q, N, k);
  { const int rc = grow(ctx, &ctx->knn_ws, &ctx->knn_ws_cap, s.workspace_bytes, s.workspace_bytes); if (rc != CCMP_OK) return rc; }
  { const int rc = grow(ctx, (void **)&ctx->connect_ws, &ctx->connect_ws_cap, E, E * 28 * sizeof(double)); if (rc != CCMP_OK) return rc; }
  { const int rc = geodesic_args(p, ctx->connect_ws, ctx->connect_ws + E * 14, max_states, states, n_states, ok, nullptr, carry_out, round_budget, check_target); if (rc != CCMP_OK) return rc; }
  { const int rc = knn_launches(ctx, KnnCall{nodes, N, queries, Q, k, mode, self_base, nbr_idx, nbr_dist}, s, st); if (rc != CCMP_OK) return rc; }
  return ccmp_host::connect_edges(ctx, p, scene, margin, nodes, queries, Q, k, check_target, max_states, round_budget, nbr_idx, states, n_states, ok,
                                  newton_iters, blocked, carry_out, hip_stream);
}

int ccmp_is_satisfied_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, uint8_t *ok, size_t B, void *hip_stream)
{
  CCMP_PROLOGUE();
  if (B == 0) return CCMP_OK;
  if (!q || !ok) return CCMP_EINVAL;
  unsigned int *flag = arm_done_word(ctx, B);
  HIP_TRY(ccmp_launch::is_satisfied(&K, q, ok, B, flag, ctx->done_seq, st));
  return CCMP_OK;
}

int ccmp_joint_valid_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, uint8_t *ok, size_t B, void *hip_stream)
{
  CCMP_PROLOGUE();
  if (B == 0) return CCMP_OK;
  if (!q || !ok) return CCMP_EINVAL;
  unsigned int *flag = arm_done_word(ctx, B);
  HIP_TRY(ccmp_launch::joint_valid(&K, q, ok, B, flag, ctx->done_seq, st));
  return CCMP_OK;
}

int ccmp_ambient_uniform_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index, double *q_out,
                               size_t B, void *hip_stream)
{
  CCMP_PROLOGUE();
  if (B == 0) return CCMP_OK;
  if (!q_out) return CCMP_EINVAL;
  HIP_TRY(ccmp_launch::ambient_uniform(&K, seed, first_index, q_out, B, st));
  return CCMP_OK;
}

int ccmp_enforce_bounds_batch(ccmp_ctx *ctx, double *q, size_t B, void *hip_stream)
{
  if (!ctx) return CCMP_EINVAL;
  if (B == 0) return CCMP_OK;
  if (!q) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(ccmp_launch::enforce_bounds(q, B, st));
  return CCMP_OK;
}

int ccmp_compact_valid(ccmp_ctx *ctx, const double *q, const uint8_t *ok, size_t B, double *q_valid, uint64_t *count_dev,
                       void *hip_stream)
{
  return ccmp_compact_valid_capped(ctx, q, ok, B, q_valid, B, count_dev, hip_stream);
}

int ccmp_compact_valid_capped(ccmp_ctx *ctx, const double *q, const uint8_t *ok, size_t B, double *q_valid, size_t capacity,
                              uint64_t *count_dev, void *hip_stream)
{
  if (!ctx || !count_dev) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (B == 0) {
    HIP_TRY(ccmp_launch::clear_words(count_dev, 2, st));
    return CCMP_OK;
  }
  if (!q || !ok || !q_valid) return CCMP_EINVAL;
  const size_t nblocks = (B + 255) / 256;
  {
    int rc = grow(ctx, (void **)&ctx->scan, &ctx->scan_cap, nblocks, nblocks * sizeof(unsigned int)); // callers that capture graphs call once un-captured first
    if (rc != CCMP_OK) return rc;
  }
  HIP_TRY(ccmp_launch::compact(q, ok, B, q_valid, capacity, ctx->scan, (unsigned long long *)count_dev, st));
  return CCMP_OK;
}

#ifdef CCMP_DEBUG_HOOKS
int ccmp_detmath_probe(ccmp_ctx *ctx, const double *x_dev, const double *y_dev, double *out_dev, size_t n, void *hip_stream)
{
  if (!ctx || !x_dev || !y_dev || !out_dev) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (n == 0) return CCMP_OK;
  HIP_TRY(ccmp_launch::detmath_probe(x_dev, y_dev, out_dev, n, st));
  return CCMP_OK;
}

int ccmp_detmath_div_probe(ccmp_ctx *ctx, const double *n_dev, const double *d_dev, double *out_dev, size_t count, void *hip_stream)
{
  if (!ctx || !n_dev || !d_dev || !out_dev) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (count == 0) return CCMP_OK;
  HIP_TRY(ccmp_launch::div_probe(n_dev, d_dev, out_dev, count, st));
  return CCMP_OK;
}

int ccmp_detmath_round_facts_probe(ccmp_ctx *ctx, const double *m_dev, const double *y_dev, const unsigned char *store_dev, double *out_dev, size_t n,
                                   void *hip_stream)
{
  if (!ctx || !m_dev || !y_dev || !store_dev || !out_dev || n == 0 || n % 64 != 0) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_TRY(ccmp_launch::round_facts_probe(m_dev, y_dev, store_dev, out_dev, n, st));
  return CCMP_OK;
}

// what the scout's order, histogram and the context's queue words hold behind the last call (ScoutBuffers; ccmp_launch.h: QueueWord)
int ccmp_ctx_debug_lpt_order(ccmp_ctx *ctx, unsigned int *order_host, size_t n, unsigned int *hist_host, unsigned long long *queue_host, size_t queue_words)
{
  if (!ctx || !order_host || !hist_host || !queue_host || !ctx->lpt_buf || n > ctx->lpt_cap || queue_words != (size_t)kQueueWords) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  ccmp_host::quiesce(ctx);
  HIP_TRY(hipDeviceSynchronize());
  const ScoutBuffers sb(ctx);
  HIP_TRY(hipMemcpy(order_host, sb.order, n * sizeof(unsigned int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hist_host, sb.hist, 1024 * sizeof(unsigned int), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(queue_host, ctx->queue, kQueueWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return CCMP_OK;
}

// the rows between the head and the resume launch as the last call that ran both ON STOCK TWIN ARMS left them (ccmp_launch.h: kStagedRow)
int ccmp_ctx_debug_fd_state(ccmp_ctx *ctx, double *rows_host, size_t n, int *row_doubles_out)
{
  if (!ctx || !row_doubles_out) return CCMP_EINVAL;
  *row_doubles_out = ccmp_launch::kStagedRow;
  if (!rows_host) return CCMP_OK;
  if (!ctx->fd_state || n * (size_t)ccmp_launch::kStagedRow > ctx->fd_state_cap) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  ccmp_host::quiesce(ctx);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(rows_host, ctx->fd_state, n * ccmp_launch::kStagedRow * sizeof(double), hipMemcpyDeviceToHost));
  return CCMP_OK;
}

// every index a split rule forms stays inside the 1024 bins (the kernels clamp p_high / p_max / kind 1's p_low from above only)
static bool split_args_ok(int kind, int p_low, int p_high, int permille, int clear)
{
  if (kind == 0) return true;
  if (kind != 1 && kind != 2) return false;
  if (p_low < 0 || p_high < 0 || permille < 0 || permille > 1000 || clear < 0 || clear > 16) return false;
  return kind == 1 || p_low <= 1023;
}

int ccmp_debug_sort_probe(ccmp_ctx *ctx, const uint16_t *keys_dev, size_t n, int nbins, int hist_blocks, int clear_first, unsigned int *order_dev,
                          unsigned int *hist_dev, unsigned long long *queue_dev, int kind, int p_low, int p_high, int permille, unsigned int limit,
                          int clear, void *hip_stream)
{
  if (!ctx || !keys_dev || !order_dev || !hist_dev || n == 0 || n > (1u << 24) || nbins < 1 || nbins > 1024 || hist_blocks < 1 || hist_blocks > 1024)
    return CCMP_EINVAL;
  if (!split_args_ok(kind, p_low, p_high, permille, clear) || (kind != 0 && !queue_dev)) return CCMP_EINVAL;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (ccmp_launch::sort_needs_clear(n)) {
    // the three-kernel form scans nbins bins only: a key beyond them would be scattered from an unscanned cursor, past the end of order
    uint16_t *keys = (uint16_t *)malloc(n * sizeof(uint16_t));
    if (!keys) return CCMP_ENOMEM;
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(keys, keys_dev, n * sizeof(uint16_t), hipMemcpyDeviceToHost);
    bool inside = true;
    for (size_t i = 0; e == hipSuccess && i < n; i++) inside = inside && (keys[i] < 1024 ? keys[i] : 1023) < nbins;
    free(keys);
    HIP_TRY(e);
    if (!inside) return CCMP_EINVAL;
    if (clear_first) HIP_TRY(ccmp_launch::clear_words(hist_dev, 1024, st));
    else { // the histogram kernel ADDS: on anything but zeros the scan's bases would leave order too
      unsigned int h[1024];
      HIP_TRY(hipMemcpy(h, hist_dev, sizeof h, hipMemcpyDeviceToHost));
      for (int k = 0; k < 1024; k++)
        if (h[k]) return CCMP_EINVAL;
    }
  }
  const ccmp_split_req req{kind ? queue_dev : nullptr, kind, p_low, p_high, permille, limit, clear};
  HIP_TRY(ccmp_launch::sort_desc(keys_dev, n, nbins, hist_blocks, hist_dev, order_dev, req, st));
  return CCMP_OK;
}

int ccmp_debug_split_probe(ccmp_ctx *ctx, int kernel, const unsigned int *hist_dev, int p_min, int p_max, int permille, unsigned int limit,
                           unsigned long long *queue_dev, void *hip_stream)
{
  if (!ctx || !hist_dev || !queue_dev || p_min < 0) return CCMP_EINVAL;
  if (kernel == 2 && (p_min > 1023 || p_max < p_min || permille < 0 || permille > 1000)) return CCMP_EINVAL; // (P walks down to p_min: never below bin 0)
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return CCMP_ENODEV;
  hipStream_t st = (hipStream_t)hip_stream;
  if (kernel == 1) HIP_TRY(ccmp_launch::fd_split(hist_dev, p_min, limit, queue_dev, st));
  else if (kernel == 2) HIP_TRY(ccmp_launch::geo_split(hist_dev, p_min, p_max, permille, queue_dev, st));
  else return CCMP_EINVAL;
  return CCMP_OK;
}
#endif

} // extern "C"

namespace ccmp_host {
bool context_alive(const ccmp_ctx *ctx) { return ctx && live_contexts(ctx, 0); }
}  // namespace ccmp_host
