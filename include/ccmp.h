/* ccmp.h — C ABI of libccmp: batched closed-chain constraint projector for AMD MI355X (gfx950).
 *
 * This is the drop-in boundary for ONE hot path of jkw0701/closed_chain_motion_planner: the Newton
 * retraction KinematicChainConstraint::project() and its sample/extend callers.  The reference has
 * no FFI layer (the path sits behind OMPL's C++ virtuals); every entry point below therefore names
 * the reference C++ member it replaces (paths relative to the reference checkout).  The C++ adapter
 * that keeps the OMPL surface source-compatible is include/ccmp_ompl_adapter.hpp; the binding a
 * maintainer adds is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C, no exceptions cross the ABI; every function returns CCMP_OK (0) or a negative code
 *   - all pointers are caller-owned; *_batch calls take DEVICE pointers and are asynchronous on
 *     the caller's HIP stream (NULL = the HIP default stream, as in every HIP API); *_host calls
 *     take host pointers, run on the ctx's own stream and are synchronous; a *_batch call may be recorded into a HIP
 *     graph by stream capture and replayed (tests/test_gpu_usage_modes.py) — after one eager call at that size, which grows
 *     the context's workspaces
 *   - state layout everywhere: row-major double q[B][14]; first 7 = the alphabetically first arm
 *     name, next 7 = the second (std::map order, src/base/constraints/ConstrainedPlanningCommon.cpp:89-91)
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails with
 *     CCMP_ENODEV
 */
#ifndef CCMP_H
#define CCMP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CCMP_VERSION 600

enum {
  CCMP_OK = 0,
  CCMP_EINVAL = -1, /* bad argument (also: non-positive tolerance, ConstraintFunction.h:106-108) */
  CCMP_EHIP = -2,   /* a HIP runtime call failed; see ccmp_last_hip_error()                      */
  CCMP_EIO = -3,    /* cannot read the YAML file                                                 */
  CCMP_EPARSE = -4, /* YAML key missing or malformed                                             */
  CCMP_ENODEV = -5, /* no HIP device / device index out of range                                 */
  CCMP_ENOMEM = -6,
  CCMP_ECOMM = -7,    /* RCCL call failed or librccl.so could not be opened; see ccmp_last_hip_error()  */
  CCMP_EOVERFLOW = -8 /* more valid states than the gather blocks / the output buffer hold: retry larger */
};

enum { CCMP_JAC_FD = 0, CCMP_JAC_ANALYTIC = 1 };

/* Everything the kernels need besides q.  POD; matrices row-major.  Built by
 * ccmp_problem_from_yaml / ccmp_problem_init, or filled by hand. */
typedef struct ccmp_problem {
  double axis[2][7][3];   /* joint axes in the parent body frame; src/kinematics/panda_rbdl.cpp:117-122 */
  double offset[2][7][3]; /* joint origin relative to the parent joint origin; panda_rbdl.cpp:128-130   */
  double ee[2][3];        /* rot_ee*(0,0,0.107); panda_rbdl.cpp:124-126                                 */
  double R_tool[2][9];    /* rot_ee*Rz(-pi/4); panda_rbdl.cpp:31                                        */
  double base_R[2][9];    /* t_wb per arm; src/kinematics/grasping_point.cpp:11-20                      */
  double base_p[2][3];
  double init_R[9];       /* init_chain_; ConstraintFunction.h:39                                       */
  double init_p[3];
  double lb[7];           /* ConstraintFunction.h:27-28 == KinematicChain.h:75-100                      */
  double ub[7];
  double joint_eps;       /* 0.001; ConstraintFunction.h:45                                             */
  double tol_pos;         /* tolerance1_ = 1e-3; ConstrainedPlanningCommon.cpp:120                      */
  double tol_rot;         /* tolerance2_ = 5e-3; ConstrainedPlanningCommon.cpp:121                      */
  double step;            /* 0.30; ConstraintFunction.h:71                                              */
  double delta;           /* 0.25; ConstrainedPlanningCommon.cpp:118                                    */
  double lambda;          /* 2.0;  ConstrainedPlanningCommon.cpp:119                                    */
  double start_joint[14]; /* config/<obj>.yaml: start_joint                                             */
  double obj_start_R[9];  /* t_wo_start; grasping_point.cpp:38-43                                       */
  double obj_start_p[3];
  double obj_goal_R[9];   /* t_wo_goal; grasping_point.cpp:45-50                                        */
  double obj_goal_p[3];
  double t_o7_R[2][9];    /* t_o7 per arm; ConstrainedPlanningCommon.cpp:110-111                        */
  double t_o7_p[2][3];
  int32_t max_iter;       /* 250; ConstraintFunction.h:26 (setMaxIterations(1000) never reaches it)     */
  int32_t jacobian_mode;  /* CCMP_JAC_FD (reference arithmetic, default) or CCMP_JAC_ANALYTIC           */
  int32_t arm_index[2];   /* 0 panda_left, 1 panda_right, 2 panda_top; grasping_point.cpp:59-63         */
} ccmp_problem;

/* ---- problem set-up (host, once per planning problem) ------------------------------------------ */
/* replaces grasping_point::loadConfig (grasping_point.cpp:34-65) + ConstrainedProblem::_setEnvironment
 * + setConstrainedOptions (ConstrainedPlanningCommon.cpp:85-132): reads the reference's YAML
 * unchanged (keys start_joint, t_wo_{start,goal}_{pos,quat}, arm1/arm2.{name,index}). */
int ccmp_problem_from_yaml(const char *yaml_path, ccmp_problem *out);
/* the same from explicit values; obj_* may be NULL (identity pose) */
int ccmp_problem_init(ccmp_problem *out, const char *arm1_name, int arm1_index, const char *arm2_name,
                      int arm2_index, const double start_joint[14], const double obj_start_pos[3],
                      const double obj_start_quat_xyzw[4], const double obj_goal_pos[3],
                      const double obj_goal_quat_xyzw[4]);
/* KinematicChainConstraint::setArmModels (ConstraintFunction.h:122-126) on a problem that is already set up — the
 * reference calls it after loadConfig (ConstrainedPlanningCommon.cpp:126): arm selection and base frames change, init_chain_
 * and t_o7 are recomputed from the stored start_joint and object pose; tolerances, delta/lambda, calibration (kept per
 * slot), mode and object poses stay.  The arms are stored IN THE ORDER GIVEN (arm1 = the first seven joints), as the
 * reference's setArmModels does; std::map (alphabetical) order is what ConstrainedProblem::_setEnvironment hands it
 * (ConstrainedPlanningCommon.cpp:89-91) and what ccmp_problem_init / ccmp_problem_from_yaml establish here.  Base frames come
 * from the index through the table of src/kinematics/grasping_point.cpp:11-20; ccmp_set_base_frame overrides one. */
int ccmp_set_arms(ccmp_problem *p, const char *arm1_name, int arm1_index, const char *arm2_name, int arm2_index);
/* ArmModel::t_wb of the arm in `arm_slot` (0 / 1), row-major rotation + translation — the frame
 * KinematicChainConstraint::function multiplies with (ConstraintFunction.h:89-90; panda_model.h:15; filled at
 * ConstrainedPlanningCommon.cpp:98).  The adapter's setArmModels passes what the ArmModel carries, so an edit of
 * grasping_point.cpp:11-20 reaches the GPU without touching this library.  init_chain_ / t_o7 are recomputed.
 * CCMP_EINVAL unless R is a finite rotation (orthonormal to 1e-9, determinant > 0) and pos is finite. */
int ccmp_set_base_frame(ccmp_problem *p, int arm_slot, const double R[9], const double pos[3]);
/* KinematicChainConstraint::setInitialPosition (ConstraintFunction.h:31-40) and the t_o7 of
 * ConstrainedPlanningCommon.cpp:110-111 */
int ccmp_set_start(ccmp_problem *p, const double q0[14]);
/* KinematicChainConstraint::setTolerance (ConstraintFunction.h:104-112): CCMP_EINVAL where the
 * reference throws ompl::Exception */
int ccmp_set_tolerance(ccmp_problem *p, double tolerance1, double tolerance2);
/* PandaModel::initModel(dh) with calibration offsets (panda_rbdl.cpp:80-148; columns a,d,theta,alpha) */
int ccmp_set_calibration(ccmp_problem *p, int arm_slot, const double dh_offsets[7][4]);

/* ---- execution context -------------------------------------------------------------------------- */
/* A context owns one device, one internal stream (used by the *_host entry points) and the work queues and
 * workspaces of the projector kernels.  Launches made through ONE context must be ordered: issue them on one
 * stream, or synchronise between streams — two projector launches of the same context running at once would
 * share queue words.  The same holds for EVERY launch-making call of a context, not only ccmp_project_* /
 * ccmp_sample_*: ccmp_geodesic_* and ccmp_check_motion_* keep their ticket and order counters in the context's queue words
 * and take their FP32 scout's workspace (predictions, histogram, processing order) from the same context-owned buffer the
 * projector's scout and two-class hand-over use — a buffer that grows (is freed and reallocated) on the first call at a
 * larger size — and the *_host / *_sharded* entry points use the context's staging buffer.  Overlapping any two of them on
 * different streams of ONE context is a data race; use one context per stream.  Calls on one context from several
 * threads must be serialised by the caller (the
 * reference serialises its constraint calls with graphMutex_, src/planner/stefanBiPRM.cpp:280,383,449); use one
 * context per thread or per stream for concurrency.  The problem description is passed by value into every
 * launch: it may be changed between calls without synchronising. */
typedef struct ccmp_ctx ccmp_ctx;
int ccmp_ctx_create(int device, ccmp_ctx **out);
void ccmp_ctx_destroy(ccmp_ctx *ctx);
/* persistent waves per CU for the projector kernels (0 = built-in default); = option "waves_per_cu" */
int ccmp_ctx_set_waves_per_cu(ccmp_ctx *ctx, int waves_per_cu);
/* projector scheduling (= options "hand_over", "small_batch"): hand_over 0 = throughput kernel (10 samples per wavefront) only,
 * 1 = that kernel until the sample queue drains, then the latency kernel on the samples still in flight (default), 2 = latency
 * kernel only; batches of at most small_batch samples always use the latency kernel (CCMP_DEFAULT = the built-in default of the
 * table below).  Results are bit-identical under every setting. */
#define CCMP_DEFAULT ((size_t)-1)
int ccmp_ctx_set_schedule(ccmp_ctx *ctx, int hand_over, size_t small_batch);
/* longest-predicted-first scheduling of large reference-arithmetic batches (= options "lpt", "lpt_min_batch"): mode 0 = index
 * order; 1 = an FP32 analytic-Jacobian scout pass predicts each sample's iteration count and the batch is processed longest
 * first, straggler hand-over kept below 131072 samples and dropped from there on (default); 2 = the same without hand-over at any size.
 * Used for batches of at least min_batch samples (CCMP_DEFAULT = the built-in default of the table below). */
int ccmp_ctx_set_lpt(ccmp_ctx *ctx, int mode, size_t min_batch);
/* Tuning options, by name.  NONE of them changes a result bit: they choose which kernels a call runs on and where the regimes
 * meet.  ccmp_ctx_set_option: CCMP_EINVAL for an unknown name or a value outside the range.  ccmp_ctx_get_option: the value in
 * force; with ctx == NULL the built-in default (no device needed); besides the table it answers "num_cus", "resident",
 * "resident_gave_up", "resident_served" and "side_stream_busy" (1 while the context's side stream still holds unfinished work).  ccmp_ctx_option_info enumerates the table
 * (index 0 .. until CCMP_EINVAL; any out-pointer may be NULL).  The table below is GENERATED from the library's
 * (tools/gen_option_docs.py) and compared with it by the CPU test suite, so a default stated here is the default in the code.
 * "resident" (0 / 1, default 0; not in the table: it starts and stops something) — see "resident service kernel" below. */
int ccmp_ctx_set_option(ccmp_ctx *ctx, const char *name, long value);
int ccmp_ctx_get_option(const ccmp_ctx *ctx, const char *name, long *value);
int ccmp_ctx_option_info(int index, const char **name, long *dflt, long *lo, long *hi, const char **doc);
/* BEGIN OPTION TABLE (generated from csrc/ccmp_policy.cpp: python tools/gen_option_docs.py --write)
 *   name                            default   range         meaning
 *   "hand_over"                     1         0..2          0 = throughput kernel (10 samples per wavefront) only, 1 = that kernel until its queue
 *                                                           drains, then the latency kernel on what is in flight, 2 = latency kernel only (=
 *                                                           ccmp_ctx_set_schedule)
 *   "small_batch"                   10240     0..max        batches of at most this many samples run on the latency kernel alone (=
 *                                                           ccmp_ctx_set_schedule)
 *   "waves_per_cu"                  0         0..32         persistent wavefronts of the throughput kernels per CU, 0 = 12 (=
 *                                                           ccmp_ctx_set_waves_per_cu)
 *   "lpt"                           1         0..2          0 = index order, 1 = FP32 scout + longest-predicted-first, hand-over kept below 131072
 *                                                           samples, 2 = the same without hand-over (= ccmp_ctx_set_lpt)
 *   "lpt_min_batch"                 16384     0..max        the scout's order from this many samples on (= ccmp_ctx_set_lpt)
 *   "latency_order_min"             2049      0..max        latency kernel alone: tickets through the scout's order from this many samples on
 *   "flat_kernel"                   1         0..1          latency work: 1 = one sample per 128-thread block, an iteration's evaluations in one
 *                                                           round, 0 = one wavefront per sample
 *   "stock_kernels"                 1         0..1          1 = kernels that skip the exact zeros of the uncalibrated Panda when both arms carry them
 *                                                           (same bits), 0 = always the general kernels
 *   "handover_threshold"            -1        -1..110       -1 = automatic; 0..10: a wavefront hands over once the queue is dry and at most this many
 *                                                           of its 10 groups are busy; 11..110: all hand over once the samples in flight fill less
 *                                                           than (value - 10) % of the group slots
 *   "fd_split"                      1         0..1          1 = split launch: above small_batch, the predicted-longest samples run on latency blocks
 *                                                           on a side stream beside the throughput kernel
 *   "fd_split_min"                  0         0..max        split launch from this many samples ...
 *   "fd_split_max"                  90112     0..max        ... up to this many
 *   "fd_split_pred"                 -1        -1..1023      predicted iterations from which a sample belongs to the front (-1: 40 up to 24576
 *                                                           samples, 56 above)
 *   "fd_split_front"                -1        -1..4096      latency blocks of the front (-1: two per CU up to 24576 samples, one above; 0 = no split)
 *   "fd_split_samples"              -1        -1..2147483647 samples of the front at most (-1: four per CU up to 24576 samples, three to four above;
 *                                                            0 = one per block)
 *   "fd_split_group_cut"            -1        -1..8         throughput wavefronts per CU left out for the front's blocks (-1: 3 up to 24576 samples,
 *                                                           2 above)
 *   "fd_head_rounds"                5         0..65535      throughput kernel alone (no split, no hand-over) from fd_head_min_batch samples on: the
 *                                                           first this many Newton rounds of every sample in a launch of their own, ten samples of
 *                                                           one age per wavefront, and the persistent kernel resumes them (0 = one launch)
 *   "fd_head_min_batch"             262144    0..max        ... from this many samples on
 *   "analytic_small_batch"          8192      0..max        analytic mode: at or below, the sixteen-lanes-per-sample latency kernel alone
 *   "analytic_waves_per_cu"         12        1..12         analytic mode: persistent wavefronts of the lane-pair kernel per CU
 *   "analytic_handover"             8         0..32         analytic mode: a wavefront of the lane-pair kernel whose tickets are gone hands over to
 *                                                           the latency kernel once it holds at most this many samples (0 = never: one launch)
 *   "scout_pairs"                   1         0..1          1 = two lanes per sample / edge, one arm each, where lanes are plentiful (stock twin
 *                                                           arms)
 *   "geodesic_flavour"              0         0..2          two builds, same bits: 0 = throughput build for calls with a round budget beyond the
 *                                                           latency build's blocks, latency build otherwise; 1 / 2 = always the throughput / latency
 *                                                           build
 *   "geodesic_order"                2         0..2          batches beyond the resident blocks: 0 = index order, 1 = far-apart edges first, 2 = FP32
 *                                                           scout order from geodesic_scout_min edges on
 *   "geodesic_order_min"            2049      0..max        no ordering pass below this many edges
 *   "geodesic_long_steps"           12        0..max        order 1: edges further apart than this many delta count as long
 *   "geodesic_scout_min"            2049      0..max        the scout from this many edges on
 *   "geodesic_scout_rounds"         64        1..1023       the scout stops an edge after this many Newton rounds
 *   "geodesic_group"                1         0..1          1 = bulk calls (round budget, scout order): short edges ten to a wavefront on the
 *                                                           throughput layout, the front of the order on latency blocks beside them
 *   "geodesic_group_min"            13312     0..max        ... from this many edges
 *   "geodesic_group_pred"           -1        -1..1023      ... cut of the order in predicted rounds (-1: the scout's cap where the edges beyond it
 *                                                           carry a tenth of the predicted work, else geodesic_group_low_cut)
 *   "geodesic_group_low_cut"        -1        -1..64        ... (-1: 40 below 20480 edges, 48 from there on, 56 from 65536)
 *   "geodesic_group_permille"       0         0..1000       ... > 0: instead, the largest cut whose front carries this share of the predicted work
 *   "geodesic_group_handover_pct"   -1        -1..100       ... with the queue dry, every wavefront gives its edges to latency blocks once those in
 *                                                           flight fill less than this share of the slots (0 = never; -1: 50 below 32768 edges, 80
 *                                                           from there on)
 *   "clearance_per_state_max"       8192      0..max        proxy clearance: one block per state up to this many states, 64-state tiles above
 *   "host_zero_copy"                2         0..2          *_host calls on page-locked caller buffers: 0 = staged, 1 = q_out written in place, 2 =
 *                                                           q_in read in place too
 *   "resident_idle_ms"              10        1..10000      the resident service kernel (option "resident") leaves by itself after this many
 *                                                           milliseconds without a request
 * END OPTION TABLE */
/* Resident service kernel (option "resident", 0 / 1, default 0): with it on, the calls the unchanged planner makes one at a time or
 * a handful at a time are served by ONE persistent 128-thread block that waits on a mailbox in pinned host memory, instead of a
 * kernel launch and a completion poll each: the same bits, no launch on the call path.  What is served:
 *   both modes      ccmp_project_host, ccmp_function_host, ccmp_is_satisfied_host, ccmp_joint_valid_host with B == 1 — the reference's
 *                   project(State*) / isSatisfied(State*), src/base/jy_ProjectedStateSpace.cpp:13,20,27,65;
 *   CCMP_JAC_FD     ccmp_geodesic_host / ccmp_geodesic_host_ex / ccmp_check_motion_host with E == 1, without carry_in, max_states <= 64 —
 *                   discreteGeodesic and checkMotion of one pair, src/planner/stefanBiPRM.cpp:315-318,397-398 (one state needs the
 *                   whole block in this mode: several edges would only run one after the other);
 *   CCMP_JAC_ANALYTIC  the same three entry points with 1 <= E <= 8 (growTree's five neighbours in one request: the edges traverse
 *                   side by side, one row of sixteen lanes each), WITH or without carry_in (continuation calls), max_states <= 64.
 * Everything else — larger E, longer lists, ccmp_geodesic_scene_host, every *_batch entry point — takes the launch path as before.
 * Each mode has its own kernel and one runs at a time: a call whose problem is of the other mode (or of the other instantiation
 * within a mode: stock / calibrated arms, diagonal / general base frames) stops the running kernel and starts the right one, which
 * costs ONE launch.  A planner that sets its mode once pays that once; one that alternates modes call by call pays it every time
 * and is better off without the option.  Started by the first served call, never under stream capture.
 * ccmp_ctx_get_option(ctx, "resident_served") is the number of requests the service has answered for this context (0 with
 * ctx == NULL; read-only, not in the table): a served call and one that fell back to the launch path give the same bits, and only
 * this count tells them apart.
 * What a kernel that stays on the device asks of the caller: the LIBRARY stops it before every hipFree / hipMalloc / device-wide
 * synchronise of its own and in ccmp_ctx_destroy (and takes the launch path while it is stopped), so every entry point of this
 * header can be mixed with resident calls; the APPLICATION's own hipDeviceSynchronize / hipFree waits until the service leaves by
 * itself, after "resident_idle_ms" (default 10) without a request — bounded, never for ever; the next call starts it again.  Its
 * stream has the lowest priority (a hardware queue of its own); should the kernel not get to run within 5 ms of a start — its queue
 * is shared with something that does not end soon, e.g. another context's service — THAT CALL takes the launch path, the kernel is
 * told to stop and abandoned (never waited for), and a later call starts the service again behind a back-off (10 ms, doubling up
 * to 1 s; "resident_gave_up" counts the occasions; setting "resident" to 1 again clears both).  Every wait is bounded, on both
 * sides: a request whose worst case exceeds 1.5 s goes to the launch path, CCMP_EHIP after 2 s without an answer (the service is
 * then not used again by the context); a several-edge request whose lines the kernel cannot read consistently within its bound is
 * answered with a refusal and that call takes the launch path. */
/* What the policy does with a call: writes ONE line into buf (NUL-terminated, truncated to cap) naming the kernels a call of
 * kind call_kind over n samples / edges runs on under the context's present settings, and the thresholds that delimit that
 * regime — computed by the same functions the launches use (csrc/ccmp_policy.cpp), so it cannot disagree with them.  ctx == NULL:
 * the built-in policy on a 256-CU device.  Returns the length of the whole line (snprintf's convention) or CCMP_EINVAL. */
enum {
  CCMP_CALL_PROJECT = 0,          /* ccmp_project_batch, reference arithmetic          */
  CCMP_CALL_SAMPLE_PROJECT = 1,   /* ccmp_sample_project_batch                         */
  CCMP_CALL_PROJECT_ANALYTIC = 2, /* ccmp_project_batch with CCMP_JAC_ANALYTIC         */
  CCMP_CALL_GEODESIC = 3,         /* ccmp_geodesic_batch / _ex without a round budget  */
  CCMP_CALL_GEODESIC_BUDGET = 4,  /* ccmp_geodesic_batch_ex with round_budget > 0      */
  CCMP_CALL_GEODESIC_ANALYTIC = 5, /* ccmp_geodesic_batch / _ex with CCMP_JAC_ANALYTIC */
  CCMP_CALL_GEODESIC_SCENE = 6,    /* ccmp_geodesic_scene_batch, both Jacobian modes    */
  CCMP_CALL_KNN = 7,               /* ccmp_knn_batch: n = the queries; 65536 nodes and k = 5 assumed (the shape follows Q, N and the CU count) */
  CCMP_CALL_CONNECT = 8,           /* ccmp_connect_batch: the k-NN part as above, then the CCMP_CALL_GEODESIC line for 5 n edges */
  /* (9 is not assigned: it stays an unknown kind) */
  CCMP_CALL_ROADMAP_KNN = 10,      /* ccmp_roadmap_knn with CCMP_METRIC_OBJECT: n = the queries; a store of 65536 nodes and k = 5 assumed */
  CCMP_CALL_ROADMAP_CONNECT = 11,  /* ccmp_roadmap_connect with CCMP_METRIC_OBJECT: the k-NN part as above, then the CCMP_CALL_GEODESIC line for 5 n edges */
  /* (12 is not assigned: it stays an unknown kind) */
  CCMP_CALL_POSE_IK = 13,          /* ccmp_pose_ik_batch: n = the targets; 5 seed slots and the default options (14 restarts) assumed */
  /* (14 is not assigned: it stays an unknown kind) */
  CCMP_CALL_OBJECT_PROPOSE = 15    /* ccmp_object_propose_batch: n = the grow indices; 2 attempts and a mesh of 1024 triangles assumed */
};
int ccmp_ctx_describe(const ccmp_ctx *ctx, int call_kind, size_t n, char *buf, size_t cap);
int ccmp_ctx_device(const ccmp_ctx *ctx);
int ccmp_ctx_num_cus(const ccmp_ctx *ctx);

/* ---- the hot path: device pointers, asynchronous on `hip_stream` -------------------------------- */
/* KinematicChainConstraint::function (ConstraintFunction.h:84-102): f[i] = (|dp|, angle) */
int ccmp_function_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, double *f, size_t B,
                        void *hip_stream);
/* KinematicChainConstraint::project (ConstraintFunction.h:57-82): q_out[i] = final iterate whether
 * or not ok[i]; ok[i] = the reference's return value; iters[i] (nullable) = Newton updates done.
 * q_in == q_out is allowed (in place, as the reference).  q_in and q_out must be 16-byte aligned (any row of a
 * hipMalloc'ed [B][14] array is): CCMP_EINVAL otherwise. */
int ccmp_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q_in, double *q_out,
                       uint8_t *ok, uint16_t *iters, size_t B, void *hip_stream);
/* KinematicChainConstraint::isSatisfied (ConstraintFunction.h:114-120) */
int ccmp_is_satisfied_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, uint8_t *ok,
                            size_t B, void *hip_stream);
/* KinematicChainConstraint::jointValid (ConstraintFunction.h:43-55) */
int ccmp_joint_valid_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, uint8_t *ok, size_t B,
                           void *hip_stream);
/* jy_ProjectedStateSampler::sampleUniform (src/base/jy_ProjectedStateSpace.cpp:10-15): ambient
 * uniform sample (counter-based: sample i, dim j uses splitmix64(seed ^ ((first_index+i)*14+j))) ->
 * project (result kept in ok[], the reference ignores it) -> enforceBounds (KinematicChain.h:118-130).
 * q_ambient (nullable) receives the un-projected samples. */
int ccmp_sample_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                              double *q_out, uint8_t *ok, uint16_t *iters, double *q_ambient, size_t B,
                              void *hip_stream);
/* jy_ProjectedStateSampler::sampleUniformNear (jy_ProjectedStateSpace.cpp:17-22): per dimension
 * uniform in [max(low, near-d), min(high, near+d)], then project, then enforceBounds.  `near` holds one
 * state per sample (near_stride 14) or one shared state (near_stride 0). */
int ccmp_sample_near_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                                   const double *near, int near_stride, double distance, double *q_out, uint8_t *ok,
                                   uint16_t *iters, double *q_ambient, size_t B, void *hip_stream);
/* jy_ProjectedStateSampler::sampleGaussian (jy_ProjectedStateSpace.cpp:24-29): mean + stdDev*N(0,1) per
 * dimension (Box-Muller on counter-based uniforms), clamped to the bounds, then project, then enforceBounds */
int ccmp_sample_gaussian_project_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                                       const double *mean, int mean_stride, double std_dev, double *q_out, uint8_t *ok,
                                       uint16_t *iters, double *q_ambient, size_t B, void *hip_stream);
/* IKTask::compute_t_wo (src/base/constraints/ik_task.cpp:10-14): object pose t_wb*FK(q)*t_o7^-1 from the
 * left arm's 7 joints (q + i*q_stride); t_wo[i] = rotation (9, row-major) then translation (3) */
int ccmp_compute_t_wo_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, int q_stride, double *t_wo, size_t B,
                            void *hip_stream);
/* jy_ProjectedStateSpace::discreteGeodesic (src/base/jy_ProjectedStateSpace.cpp:32-96), E edges at once:
 * states[e][0..n_states[e]) (capacity max_states each) = `from`, then every accepted state; ok[e] = the reference's
 * return value.  An edge whose list would need more than max_states entries stops there and reports n_states[e] =
 * max_states + 1 (ok[e] = 0): repeat it with a larger buffer before anything is concluded from it (the adapter and the
 * Python mirror do) — a creeping edge (observed: 952 accepted states, each a hair closer to the target) must not hold
 * a whole launch, and a cut list must never look complete.  Runs as the reference does with interpolate == true; for
 * interpolate == false the host truncates at the first state its StateValidityChecker rejects, or, for a
 * proxy scene's pre-filter, ccmp_geodesic_scene_batch applies it on the device.
 * With jacobian_mode = CCMP_JAC_ANALYTIC the traversal is one launch of a traversal kernel on the analytic projector's Newton round (four
 * edges per wavefront, no host synchronisation): the same lists, counts, flags and carries as the analytic mode's CPU restatement, bit for
 * bit, the round budget of ccmp_geodesic_batch_ex included; the resident service does not serve it. */
int ccmp_geodesic_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                        double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, void *hip_stream);
/* The same, resumable.  carry_out (nullable, [E][2]) receives what a continuation needs: the running length and the
 * bound lambda * dist(from, to).  An edge can stop short of its end in two ways, and either way a later call with
 * from[e] = its last stored state, the same to[e] and carry_in[e] = that carry_out[e] goes on where it stopped (its list
 * starts with that state again: drop it when joining the lists); first call + continuations give the states, flags and
 * Newton counts of ONE uninterrupted traversal, bit for bit:
 *   - its list is full: n_states[e] = max_states + 1, ok[e] = 0, last stored state = states[e][max_states - 1];
 *   - round_budget > 0 and the edge has spent that many Newton rounds (Jacobian evaluations) in this call: it stops between
 *     two states, ok[e] = 2, n_states[e] = the states stored so far (last stored state = states[e][n_states[e] - 1]).
 * A call thereby bounds the serial work it spends on any one edge — one edge in 16 384 near-neighbour edges creeps (952
 * states, 12 379 Newton rounds) and two dozen need more than 128 rounds; without a bound a launch lasts as long as its
 * longest edge.  round_budget = 0: no bound (ok is 0 / 1 only).  check_target as in ccmp_check_motion_batch (not together
 * with carry_in: the target was tested by the call being continued).  A resumable call (carry_in, carry_out or round_budget
 * given) needs max_states >= 2 — a one-entry list holds `from` only and its continuation would start from `from` again:
 * CCMP_EINVAL otherwise. */
int ccmp_geodesic_batch_ex(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                           double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, const double *carry_in,
                           double *carry_out, int round_budget, int check_target, void *hip_stream);
/* OMPL ConstrainedMotionValidator::checkMotion as the reference's planner calls it (src/planner/stefanBiPRM.cpp:397-398,
 * 463-464; jy_MotionValidator, jy_ProjectedStateSpace.h:57-69): isSatisfied(to) && discreteGeodesic(from, to) in ONE
 * launch — same outputs as ccmp_geodesic_batch, except that an edge whose target fails isSatisfied reports ok = 0 and
 * only `from` (n_states = 1) without being traversed */
int ccmp_check_motion_batch(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                            double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, void *hip_stream);
/* the ambient sampler alone (RealVectorStateSampler::sampleUniform over KinematicChain.h:75-100) */
int ccmp_ambient_uniform_batch(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                               double *q_out, size_t B, void *hip_stream);
/* KinematicChainSpace::enforceBounds (KinematicChain.h:118-130), in place */
int ccmp_enforce_bounds_batch(ccmp_ctx *ctx, double *q, size_t B, void *hip_stream);
/* stable compaction of the rows with ok != 0 (what the host tree consumes); *count_dev is a device
 * uint64 */
int ccmp_compact_valid(ccmp_ctx *ctx, const double *q, const uint8_t *ok, size_t B, double *q_valid,
                       uint64_t *count_dev, void *hip_stream);
/* the same into a buffer of `capacity` rows (fixed-size send buffers of the all-gather): valid rows past the capacity
 * are dropped, *count_dev still reports how many there were — a count above the capacity tells the consumer */
int ccmp_compact_valid_capped(ccmp_ctx *ctx, const double *q, const uint8_t *ok, size_t B, double *q_valid,
                              size_t capacity, uint64_t *count_dev, void *hip_stream);

/* ---- host-pointer conveniences (H2D, kernel, D2H; synchronous) ----------------------------------
 * ccmp_project_host recognises a caller's PAGE-LOCKED q_in / q_out (hipHostMalloc, hipHostRegister; a batch larger than 64 KB,
 * both 16-byte aligned): the kernels then write the projected rows straight into q_out instead of staging and downloading
 * them (option "host_zero_copy": 2 = that and q_in is read in place as well, default; 1 = q_in is uploaded by one copy first;
 * 0 = staged like pageable memory). */
int ccmp_project_host(ccmp_ctx *ctx, const ccmp_problem *p, const double *q_in, double *q_out, uint8_t *ok,
                      uint16_t *iters, size_t B);
int ccmp_function_host(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, double *f, size_t B);
int ccmp_is_satisfied_host(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, uint8_t *ok, size_t B);
int ccmp_joint_valid_host(ccmp_ctx *ctx, const ccmp_problem *p, const double *q, uint8_t *ok, size_t B);
int ccmp_sample_project_host(ccmp_ctx *ctx, const ccmp_problem *p, uint64_t seed, uint64_t first_index, double *q_out,
                             uint8_t *ok, uint16_t *iters, size_t B);
/* sampleUniformNear (kind 0, param = distance) / sampleGaussian (kind 1, param = stdDev) x B around ONE host reference
 * state (jy_ProjectedStateSpace.cpp:17-29): ambient draw, project, enforceBounds */
int ccmp_sample_ref_project_host(ccmp_ctx *ctx, const ccmp_problem *p, int kind, uint64_t seed, uint64_t first_index,
                                 const double ref[14], double param, double *q_out, uint8_t *ok, uint16_t *iters, size_t B);
/* states: [E][max_states][14], n_states: [E], ok: [E] (host buffers) */
int ccmp_geodesic_host(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                       double *states, int32_t *n_states, uint8_t *ok);
int ccmp_check_motion_host(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                           double *states, int32_t *n_states, uint8_t *ok);
int ccmp_geodesic_host_ex(ccmp_ctx *ctx, const ccmp_problem *p, const double *from, const double *to, size_t E, int max_states,
                          double *states, int32_t *n_states, uint8_t *ok, const double *carry_in, double *carry_out, int round_budget,
                          int check_target);

/* ---- one process, several GPUs (the reference's planner is a single process) ------------------------- */
/* Contiguous shards of the batch go to the n contexts (1 <= n <= 64, one per device; the same device may appear twice),
 * each shard is uploaded, projected and downloaded on its context's own stream, all concurrently; returns
 * when every shard is back.  No collective is needed: every GPU returns its shard straight to the host
 * tree.  Results are bit-identical to a single-GPU call.  (With the collective: ccmp_project_sharded below; the
 * one-process-per-GPU form lives above the ABI: closed_chain_motion_planner_amd/distributed.py.) */
int ccmp_project_sharded_host(ccmp_ctx *const *ctxs, int n, const ccmp_problem *p, const double *q_in, double *q_out,
                              uint8_t *ok, uint16_t *iters, size_t B);
/* sampleUniform x B across the contexts; sample i is a function of (seed, first_index + i) only */
int ccmp_sample_project_sharded_host(ccmp_ctx *const *ctxs, int n, const ccmp_problem *p, uint64_t seed, uint64_t first_index,
                                     double *q_out, uint8_t *ok, uint16_t *iters, size_t B);
/* Per context (n values each) of the last ccmp_*_sharded_host / ccmp_*_sharded call: launch_ms = milliseconds from the
 * call's entry to the moment the host had that shard's upload behind it and issued its kernels; start_ms = the same moment
 * on the GPU's timeline relative to ctxs[0]'s (an event on each context's stream; -1 for a context on another device than
 * ctxs[0], where no common timeline exists).  Every shard is driven by its own short-lived host thread, so both stay
 * within a fraction of a millisecond of each other for any number of GPUs; a serial upload would show as values growing
 * with the shard index (a pageable 29 MB shard: ~1.2 ms each). */
int ccmp_sharded_host_last_timing(ccmp_ctx *const *ctxs, int n, double *launch_ms, double *start_ms);

/* ---- one process, several GPUs, with the collective (ccmp_project_sharded) ------------------------- */
/* A communicator over the devices of n contexts (one context per device, 1 <= n <= 64): ncclCommInitAll in this
 * process — RCCL over xGMI inside a node; librccl.so is opened at run time, libccmp.so does not link against it. */
typedef struct ccmp_comm ccmp_comm;
int ccmp_comm_create(ccmp_ctx *const *ctxs, int n, ccmp_comm **out);
void ccmp_comm_destroy(ccmp_comm *comm);
/* per GPU (n values each), measured on that GPU's stream during the last ccmp_*_sharded call: milliseconds from the start
 * of its shard to the end of its projection + compaction, and from there to the completion of the all-gather (-1: no
 * call yet).  What a multi-GPU run is diagnosed by: stragglers show in kernel_ms, a slow collective in gather_ms. */
int ccmp_comm_last_timing(const ccmp_comm *comm, double *kernel_ms, double *gather_ms);
/* project(x) x B (host buffers), contiguous shards over the communicator's GPUs; every GPU compacts its VALID states
 * into a block of block_rows rows (+ one leading row that carries its count) and ONE ncclAllGather brings all blocks
 * to every GPU; GPU 0 hands them to the host: valid_out[0..*n_valid) (capacity valid_capacity rows) = the valid
 * states of all shards in global sample order, counts[g] (nullable, n entries) = valid states of shard g.  q_out / ok /
 * iters (all nullable) additionally receive the full per-sample results, each GPU returning its shard directly.
 * CCMP_EOVERFLOW if a shard holds more valid states than block_rows or the total exceeds valid_capacity (counts and
 * *n_valid are filled: retry with room).  Bit-identical to a single-GPU call. */
int ccmp_project_sharded(ccmp_comm *comm, const ccmp_problem *p, const double *q_in, size_t B, double *q_out, uint8_t *ok,
                         uint16_t *iters, size_t block_rows, double *valid_out, size_t valid_capacity, uint64_t *counts,
                         uint64_t *n_valid);
/* sampleUniform x B the same way; sample i is a function of (seed, first_index + i) only */
int ccmp_sample_project_sharded(ccmp_comm *comm, const ccmp_problem *p, uint64_t seed, uint64_t first_index, size_t B,
                                double *q_out, uint8_t *ok, uint16_t *iters, size_t block_rows, double *valid_out,
                                size_t valid_capacity, uint64_t *counts, uint64_t *n_valid);

/* ---- proxy-geometry clearance: a pre-filter in FRONT of the MoveIt validity test ----------------------------------- */
/* KinematicChainValidityChecker::isValid (src/kinematics/KinematicChain.cpp:94-123) sets both arms' joints, updates the
 * robot state and asks MoveIt's PlanningScene::checkCollision under an AllowedCollisionMatrix.  MoveIt, FCL and the
 * robot's URDF meshes stay on the host (out of scope to accelerate); what runs here is the cheap test a
 * planner puts in front of it ("per-arm collision pre-filter (capsule/sphere proxies) ahead of MoveIt
 * isValidImpl"): spheres rigidly attached to link frames of the two arms (or to the world), static oriented boxes (the
 * reference's "sub_table", KinematicChain.cpp:25-30), a 32 x 32 allowed-pair matrix between user-chosen groups (the
 * reference's acm_, KinematicChain.cpp:9,86-91), and for every state the smallest signed distance over all pairs that
 * are not allowed.  With proxies INSCRIBED in the real geometry a negative clearance proves a collision (the state can
 * be dropped without asking MoveIt); with CIRCUMSCRIBED proxies a positive clearance proves freedom.  The proxies are
 * the caller's: the reference ships no link geometry (robot_description comes from the ROS parameter server), so this
 * entry point cannot be — and is not — compared with MoveIt; it is bit-exact against oracle/ccmp_oracle.c:orc_clearance,
 * whose frames are the projector's own forward kinematics.
 *
 * Frames: CCMP_FRAME_WORLD, or CCMP_FRAME(arm, k) with arm 0 / 1 in state order and
 *   k = 0..6  the RBDL body of joint k (panda_link1..7): origin at the joint, axes parallel to the arm base at q = 0
 *             (panda_rbdl.cpp:117-147: the bodies are chained by pure translations)
 *   k = 7     the hand frame PandaModel::getTransform returns (panda_rbdl.cpp:24-42): 0.107 m beyond joint 6, turned -45 deg
 *   k = 8     the arm's base (panda_link0), t_wb of grasping_point.cpp:11-20 */
#define CCMP_FRAME_WORLD (-1)
#define CCMP_FRAME(arm, k) ((arm) * 9 + (k))
#define CCMP_MAX_SPHERES 64
#define CCMP_MAX_BOXES 8
typedef struct ccmp_sphere {
  int32_t frame; /* CCMP_FRAME_WORLD or CCMP_FRAME(arm, k) */
  int32_t group; /* 0..31: row / column of the allowed-pair matrix */
  double c[3];   /* centre in that frame, metres */
  double r;      /* radius, >= 0 */
} ccmp_sphere;
typedef struct ccmp_box { /* static, oriented, in the world frame */
  int32_t group;
  int32_t reserved;
  double c[3];    /* centre */
  double R[9];    /* row-major rotation, box axes -> world */
  double half[3]; /* half extents along the box axes */
} ccmp_box;
typedef struct ccmp_scene ccmp_scene;
/* allowed[g] bit h set = pairs between groups g and h are never tested (either direction counts; NULL = nothing allowed).
 * Never tested either: two proxies on the same frame, and two proxies that are both static (world or an arm's base).
 * Pairs are numbered sphere i < sphere j in the caller's order first, then (sphere i, box b).
 * Any finite centre and radius is accepted.  The 64-state tile kernel of ccmp_clearance_batch prunes pairs on their squared
 * distance, which is exact only while (running minimum + a pair's radii) < 2^22 m: the two roundings of that sum plus the
 * prune's nanometre stay below the nanometre there, so a pruned pair provably cannot become the minimum.  The host bounds that
 * sum from the arms' reach (base position, link offsets, tool), the largest sphere centre and radii and the boxes' centres
 * (ccmp_scene.cpp: clearance_magnitude_bound); a scene whose bound is not below 2^22 — a wall or a floor modelled as one huge
 * sphere — is served by the one-block-per-state kernel, which does not prune, whatever B and "clearance_per_state_max" say:
 * the same bits as the oracle, at that kernel's speed. */
int ccmp_scene_create(ccmp_ctx *ctx, const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes,
                      const uint32_t allowed[32], ccmp_scene **out);
void ccmp_scene_destroy(ccmp_scene *scene);
int ccmp_scene_num_pairs(const ccmp_scene *scene);
/* clearance[i] = min over tested pairs of (distance between centres - r_i - r_j), or (distance from the sphere centre to the
 * box, 0 inside) - r_i; +inf when nothing is tested; NaN for a state with a non-finite joint value.  pair[i] (nullable)
 * = i_sphere | (j << 8) of the first pair in the numbering above that attains it, j = 64 + box index for a box, -1 when
 * there is none.  free_out[i] (nullable) = (ok_in == NULL || ok_in[i]) && clearance[i] > margin — it can go straight into
 * ccmp_compact_valid behind a projection.  Device pointers, asynchronous on hip_stream. */
int ccmp_clearance_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, const double *q, const uint8_t *ok_in,
                         size_t B, double margin, double *clearance, int32_t *pair, uint8_t *free_out, void *hip_stream);
/* the same on host buffers (a single state: what a StateValidityChecker wrapper calls before MoveIt) */
int ccmp_clearance_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, const double *q, size_t B, double margin,
                        double *clearance, int32_t *pair, uint8_t *free_out);
/* The extend step with the proxy pre-filter on the device: jy_ProjectedStateSpace::discreteGeodesic with interpolate == false
 * (src/base/jy_ProjectedStateSpace.cpp:65-68, what growTree and checkMotion run) where svc->isValid(x) is
 * "ccmp_clearance_batch's clearance of x > margin" (the rule of its free_out).  Per edge the result equals, bit for bit and in
 * both Jacobian modes, the reference's loop with that validity test (the CPU checker oracle/ccmp_oracle.c: its resumable
 * discrete geodesic with a validity callback that asks its clearance): states, n_states, ok, newton_iters, carry_out.  Arguments, outputs, carries, the round budget (ok = 2) and check_target as
 * ccmp_geodesic_batch_ex; in addition:
 *   - where the test runs: after a successful projection (converged and jointValid), before the step test — the reference's
 *     order, so the clearances evaluated are exactly the oracle's valid() calls;
 *   - a refusal beats "list full": a refused state that finds the list full ends the edge with n_states = the states stored
 *     and blocked set, not max_states + 1;
 *   - never tested: row 0 (`from`, or the first state of a continuation) and the target under check_target (checkMotion does
 *     not call isValid(s2));
 *   - a refused edge ends as the reference's break: ok = (distance of the last accepted state to the target) <= delta, and its
 *     Newton count includes the refused state's projection;
 *   - blocked (nullable, uint8[E]) = 1 exactly when the traversal ended at a state the scene refused (the oracle's last valid()
 *     call returned 0).  A blocked edge is final: do not continue it;
 *   - clearance (nullable, double[E][max_states]): entry k = the clearance of listed state k, 1 <= k < min(n_states, max_states);
 *     entry 0 and entries past the list are not written.  Bit-identical to ccmp_clearance_batch of that state;
 *   - continuations keep their meaning: pass the same scene and margin, and first call + continuations give one uninterrupted
 *     traversal;
 *   - margin = -inf: the results of ccmp_geodesic_batch_ex, blocked all 0; margin = +inf: every edge that enters the loop stops
 *     at its first projected state with n_states = 1, blocked = 1 if that projection succeeded (0 if it failed).
 * CCMP_EINVAL besides ccmp_geodesic_batch_ex's cases: scene NULL, a scene of another device than ctx's, margin NaN.  One launch
 * (FD: geodesic_scene_kernel, one 128-thread block per edge; analytic: geodesic_row16_scene_kernel, sixteen lanes per edge), no
 * host synchronisation, capturable; never the bulk form of the FD extend step, never the resident service. */
int ccmp_geodesic_scene_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *from, const double *to,
                              size_t E, int max_states, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                              double *clearance, const double *carry_in, double *carry_out, int round_budget, int check_target, void *hip_stream);
/* the same on host buffers, synchronous */
int ccmp_geodesic_scene_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *from, const double *to,
                             size_t E, int max_states, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                             double *clearance, const double *carry_in, double *carry_out, int round_budget, int check_target);

/* ---- the connection step: k nearest neighbours, and neighbours + checkMotion in one call ------------------------------------------ */
/* The reference chooses the pairs it tries with connectionStrategy_(m): a KStrategy over tree_ with DEFAULT_NEAREST_NEIGHBORS = 5
 * (src/planner/stefanBiPRM.cpp:292,390,457; stefanBiPRM.h:35), followed by checkMotion(neighbour, new) per neighbour in addMilestone /
 * startgoalMilestone (:392-409, :458-475) or discreteGeodesic(neighbour, new) in growTree (:307-351).
 * Distance: RealVectorStateSpace::distance over the 14 joints exactly as oracle/ccmp_oracle.c: orc_distance states it — the chain
 * dist = fma(diff_i, diff_i, dist), i = 0..13, diff_i = a[i] - b[i], then the correctly rounded square root; not wrap-aware.  THE
 * JOINT TERM ONLY.  The metric the reference's tree actually ranks on is the SE3 distance between the vertices' object poses
 * (stefanBiPRM.h:194-201): CCMP_METRIC_OBJECT of the roadmap store below.
 * Ranking of the eligible nodes of a query: ascending by (distance as returned, i.e. after the square root; node index) — equal
 * distances go to the lower index, also where two different squared sums round to one distance.  Eligible: a node whose distance
 * to the query is not NaN (a NaN on either side: never a neighbour), and by mode
 *   CCMP_KNN_ALL       every node;
 *   CCMP_KNN_NOT_SELF  query q IS node self_base + q, which is left out;
 *   CCMP_KNN_EARLIER   only nodes j < self_base + q: a batch inserted in order, each node seeing the ones before it — the
 *                      sequential addMilestone order.
 * nbr_idx[q][r] / nbr_dist[q][r] (nullable), r = 0..k-1: the r-th neighbour; fewer than k eligible nodes leave the remaining slots
 * idx = -1, dist = +inf.  1 <= k <= CCMP_KNN_MAX_K, N < 2^31 (N == 0 is allowed: every slot empty), Q < 2^31; Q == 0 returns CCMP_OK and
 * touches nothing.  The result is a function of the arguments alone: the launch shape (csrc/ccmp_policy.cpp: plan_knn, from Q, N and
 * the CU count; no option) never changes it.  `nodes` is read per call and the host form uploads the nodes every time; a roadmap that
 * grows by one vertex per query belongs in the device-resident store below (ccmp_roadmap_*).  Device pointers, asynchronous on
 * hip_stream, capturable (after one eager call at that size); the resident service does not serve these calls. */
#define CCMP_KNN_MAX_K 16
enum { CCMP_KNN_ALL = 0, CCMP_KNN_NOT_SELF = 1, CCMP_KNN_EARLIER = 2 };
int ccmp_knn_batch(ccmp_ctx *ctx, const double *nodes, size_t N, const double *queries, size_t Q, int k, int mode, size_t self_base,
                   int32_t *nbr_idx, double *nbr_dist, void *hip_stream);
/* the same on host buffers, synchronous */
int ccmp_knn_host(ccmp_ctx *ctx, const double *nodes, size_t N, const double *queries, size_t Q, int k, int mode, size_t self_base,
                  int32_t *nbr_idx, double *nbr_dist);
/* Neighbours and their traversals in ONE call on one stream, without a host synchronisation: ccmp_knn_batch, then edge e = q * k + r
 * with from = nodes[nbr_idx[q][r]] and to = queries[q] — the reference's direction, checkMotion(n, m) / discreteGeodesic(n -> t) —
 * through the extend step exactly as ccmp_geodesic_batch_ex runs it (scene == NULL; blocked, if given, is all 0) or as
 * ccmp_geodesic_scene_batch runs it (scene, margin; no clearance output).  check_target = 1: addMilestone's checkMotion; 0: growTree's
 * discreteGeodesic.  states [Q*k][max_states][14], n_states / ok / newton_iters (nullable) / blocked (nullable) [Q*k], carry_out
 * [Q*k][2] (nullable unless round_budget > 0).  Every occupied slot reports, bit for bit, what that entry point reports for the pair;
 * an empty slot (idx = -1) costs no Newton work and reports ok = 0, n_states = 0, newton_iters = 0, blocked = 0, carry_out = {0, 0}
 * (its rows of `states` are unspecified).  A suspended (ok = 2) or full-list (n_states = max_states + 1) edge is continued through
 * ccmp_geodesic_batch_ex / ccmp_geodesic_scene_batch as documented there: from = its last stored state, to = queries[q], carry_in =
 * its carry_out.  CCMP_EINVAL: the k-NN's and ccmp_geodesic_batch_ex's cases, and with a scene ccmp_geodesic_scene_batch's. */
int ccmp_connect_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *nodes, size_t N,
                       const double *queries, size_t Q, int k, int mode, size_t self_base, int check_target, int max_states, int round_budget,
                       int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                       double *carry_out, void *hip_stream);
/* the same on host buffers, synchronous */
int ccmp_connect_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *nodes, size_t N,
                      const double *queries, size_t Q, int k, int mode, size_t self_base, int check_target, int max_states, int round_budget,
                      int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                      double *carry_out);

/* ---- the device-resident roadmap store, and the planner's own tree metric ------------------------------------------------------------ */
/* The reference's tree_ ranks on obj_space_->distance(components[1], components[1]) (stefanBiPRM.h:194-201; the joint-space line above it
 * is commented out): OMPL's SE3StateSpace::distance between the OBJECT POSES of two vertices, with the default weights 1 and 1,
 *     d(a, b) = |dp| + rot(a, b),   rot = 0 if |qa . qb| > 1 - 1e-9 (SO3StateSpace's MAX_QUATERNION_NORM_ERROR), else acos(|qa . qb|),
 * in the rounding model of the rest of the library (csrc/ccmp_pose.h: FMA chains over x, y, z and over qx, qy, qz, qw, the correctly
 * rounded square root, acos(dq) = atan2(sqrt(1 - dq^2), dq)); quaternions are not normalised, a NaN anywhere gives NaN.
 * A pose is 8 doubles: x y z qx qy qz qw pad; public pose arrays are [n][8]; the pad is written as 0 and never read.
 * The pose of a joint state (stefanBiPRM.cpp:338, utils.h:37-46) = ccmp_compute_t_wo_batch of the left arm, then Eigen's
 * Quaterniond(Matrix3d) (the trace / largest-diagonal branches of oracle/ccmp_oracle.c: R_to_quat, bit for bit).
 * The two functions below are pure host code: no device, never CCMP_ENODEV (the planner's single-pair distances,
 * stefanBiPRM.cpp:340-341,635). */
double ccmp_pose_distance(const double a[8], const double b[8]);
void ccmp_pose_from_t_wo(const double t_wo[12], double pose[8]);

/* The store: the joints [14] and the object pose [8] of every roadmap vertex, resident on the context's device, so that a planner that
 * appends one vertex and queries uploads one vertex.  Indices are positions: an append takes size .. size + Q - 1.  ONLY THE TAIL CAN BE
 * REMOVED (ccmp_roadmap_truncate: the reference's remove_vertex(t) of the vertex just appended, stefanBiPRM.cpp:353-359); interior
 * vertices cannot.  The size is host state of the handle: every call below takes effect, for later calls ON THE SAME STREAM, in call
 * order; calls on different streams are the caller's to order.  One store belongs to one context and to one thread at a time.
 *   create    capacity_hint = rows allocated up front (0: a small default).  Returns NULL on any failure (ctx NULL, no memory); a store
 *             needs a context, so where ccmp_ctx_create answers CCMP_ENODEV there is no store.  Every entry below answers a NULL store
 *             with CCMP_ENODEV on a machine without a HIP device and with CCMP_EINVAL otherwise.
 *   destroy   quiesces the context first, as scenes do; the context must outlive the store or be destroyed first with its service off.
 *   reserve   room for n vertices in all, now (synchronous: it waits for the device when it has to move the rows); after it, appends up to n
 *             never grow.
 *   append    joints [Q][14] and / or poses [Q][8], device pointers.  poses == NULL: derived on the device from the joints and `p`
 *             (pose_from_joints_kernel).  joints == NULL (poses given): growTree's pose-only vertex (stefanBiPRM.cpp:283-292) — its joint
 *             row is NaN, so no joint-metric query ever returns it, until ccmp_roadmap_set_joints fills it in.  Both NULL: CCMP_EINVAL.
 *             p may be NULL when poses are given.  *first_index (nullable) = the first new index.  Asynchronous on hip_stream and
 *             capturable WHILE THE CAPACITY HOLDS; an append beyond it grows the store: a new allocation of at least twice the size, a
 *             device-to-device copy and ONE synchronisation of hip_stream before the old block is freed — the only non-asynchronous case
 *             (never under capture: reserve first).
 *   set_joints  joints[14] (device pointer) into row `index` < size, asynchronous on hip_stream; the pose row is not touched.
 *             ccmp_roadmap_set_joints_host takes a host pointer (growTree hands over the result of its IK: ccmp_pose_ik_* / ccmp_roadmap_grow below) and is synchronous.
 *   truncate  size = n <= size; keeps the capacity.  CCMP_EINVAL for n below the edge floor of a store with edges (see the graph section below).
 *   read      rows first .. first + count - 1 into joints_out [count][14] / poses_out [count][8] (device pointers, either may be NULL).
 *   knn       the k nearest vertices of each query.  CCMP_METRIC_JOINT: queries [Q][14], the kernels of ccmp_knn_batch over the store's
 *             joint rows — bit-identical to ccmp_knn_batch on the same rows.  CCMP_METRIC_OBJECT: queries [Q][8] poses, the distance
 *             above (knn_pose_few_kernel / knn_pose_many_kernel; shape: csrc/ccmp_policy.cpp: plan_knn_pose, from Q, N and the CU count
 *             only).  Everything else as ccmp_knn_batch: modes and self_base, ranking by (distance, index), NaN never a neighbour,
 *             idx = -1 / dist = +inf in empty slots, 1 <= k <= CCMP_KNN_MAX_K, a result that no launch shape changes.
 *   connect   neighbours from the store by `metric`, then edge e = q * k + r from the store's JOINTS at nbr_idx[q][r] to query_joints[q]
 *             through the unchanged gather -> traversal -> fix chain of ccmp_connect_batch: outputs, empty slots and continuation rules
 *             as documented there.  CCMP_METRIC_OBJECT ranks on query_poses [Q][8], or with query_poses == NULL on the poses derived
 *             from query_joints.  A neighbour chosen by the object metric whose joint row is still NaN (a pose-only vertex) gives an
 *             edge from NaN joints: fill the joints in first.
 * The *_host forms take host pointers, are synchronous on the context's own stream and upload only what is new. */
enum { CCMP_METRIC_JOINT = 0, CCMP_METRIC_OBJECT = 1 };
typedef struct ccmp_roadmap ccmp_roadmap;
ccmp_roadmap *ccmp_roadmap_create(ccmp_ctx *ctx, size_t capacity_hint);
void ccmp_roadmap_destroy(ccmp_roadmap *rm);
size_t ccmp_roadmap_size(const ccmp_roadmap *rm);
int ccmp_roadmap_reserve(ccmp_roadmap *rm, size_t n);
int ccmp_roadmap_append(ccmp_roadmap *rm, const ccmp_problem *p, const double *joints, const double *poses, size_t Q, size_t *first_index,
                        void *hip_stream);
int ccmp_roadmap_set_joints(ccmp_roadmap *rm, size_t index, const double *joints, void *hip_stream);
int ccmp_roadmap_truncate(ccmp_roadmap *rm, size_t n);
int ccmp_roadmap_read(ccmp_roadmap *rm, size_t first, size_t count, double *joints_out, double *poses_out, void *hip_stream);
int ccmp_roadmap_knn(ccmp_roadmap *rm, int metric, const double *queries, size_t Q, int k, int mode, size_t self_base, int32_t *nbr_idx,
                     double *nbr_dist, void *hip_stream);
int ccmp_roadmap_connect(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, int metric, const double *query_joints,
                         const double *query_poses, size_t Q, int k, int mode, size_t self_base, int check_target, int max_states, int round_budget,
                         int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked,
                         double *carry_out, void *hip_stream);
int ccmp_roadmap_append_host(ccmp_roadmap *rm, const ccmp_problem *p, const double *joints, const double *poses, size_t Q, size_t *first_index);
int ccmp_roadmap_set_joints_host(ccmp_roadmap *rm, size_t index, const double *joints);
int ccmp_roadmap_read_host(ccmp_roadmap *rm, size_t first, size_t count, double *joints_out, double *poses_out);
int ccmp_roadmap_knn_host(ccmp_roadmap *rm, int metric, const double *queries, size_t Q, int k, int mode, size_t self_base, int32_t *nbr_idx,
                          double *nbr_dist);
int ccmp_roadmap_connect_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, int metric,
                              const double *query_joints, const double *query_poses, size_t Q, int k, int mode, size_t self_base, int check_target,
                              int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *states, int32_t *n_states, uint8_t *ok,
                              int32_t *newton_iters, uint8_t *blocked, double *carry_out);

/* ---- pose-targeted IK: growTree's sampleCalibGoal step ----------------------------------------------------------------------------- */
/* The reference's growTree creates a vertex that has only an object pose, ranks its neighbours on the object metric and calls
 * sampleCalibGoal(obj_state, neighbour joints, new joints) per neighbour until one succeeds (stefanBiPRM.cpp:283-302,
 * jy_ConstrainedValidStateSampler.h:147-189); the same call produces every start and goal state (stefanBiPRM.cpp:722,744,760).  Per arm
 * a the hand target is T_obj * t_o7[a] (ik_task.cpp:16-28); TRAC-IK solves from the neighbour's seven joints and, where that fails, from
 * 14 Gaussian configurations around mid-range (sigma 0.3, clamped to the limits: panda_tracik.cpp:62-78), keeping the converged one
 * closest to the seed; both arms must succeed; the first neighbour that succeeds wins.
 * WHAT IS AND IS NOT RESTATED: TRAC-IK (KDL + NLopt, time-bounded, two racing threads) is not reproducible and is not part of this
 * library.  These calls restate the RULE AROUND IT and put a deterministic damped-least-squares Newton solver of this project's own where
 * the reference calls CartToJnt, on the projector's own forward kinematics (csrc/ccmp_ik.h states target, error, test, step and rule in
 * full): a state they return satisfies the constraint by construction — both hands meet T_obj * t_o7 within eps per twist component.
 * The reference's IKValid and si_->isValid(result) (MoveIt) stay host calls on the returned state; the proxy pre-filter is one
 * ccmp_clearance_* call on it.
 *   target_poses [T][8]   object poses in the store's format (x y z qx qy qz qw pad); the quaternion is NOT normalised (utils.h:22)
 *   seeds [T][S][14]      S seed slots per target in the order to try them, 1 <= S <= CCMP_IK_MAX_SEEDS; a slot with a non-finite entry
 *                         is skipped
 *   rng_seed, first_index the restarts' stream: restart r = 1..R of (target t, slot s, arm a) starts from ccmp::ambient_gaussian at index
 *                         ((first_index + t) S + s) R + (r - 1), dimension 7 a + i, mean (lb_i + ub_i) / 2 — a call over T targets equals
 *                         T calls over one with the matching first_index
 *   q_out [T][14], ok [T], which [T]   the state, 1 / 0, and the slot that gave it; on failure a NaN row, ok = 0, which = -1
 *   cand_q [T][S][2][1 + R][7], cand_rounds [T][S][2][1 + R]   (nullable) every candidate's last iterate and the rounds it took, -1 = not
 *                         converged within max_rounds, -2 = its slot was skipped (the iterate is NaN)
 * Start configurations and every iterate are clamped into [lb + joint_eps, ub - joint_eps] (a value on the bound passes jointValid).
 * The result is a function of the arguments alone: no launch shape changes it, and ccmp_pose_ik_ref gives the same bits.
 * ccmp_pose_ik_batch: device pointers, asynchronous on hip_stream, capturable after one eager call at that size (the candidates'
 * records live in a workspace of the context).  ccmp_pose_ik_host: host pointers, synchronous on the context's stream.  Both answer a
 * NULL context with CCMP_ENODEV on a machine without a HIP device and with CCMP_EINVAL otherwise; every check runs before the first
 * launch.  ccmp_pose_ik_ref: THE SAME TEXT COMPILED FOR THE HOST on host pointers, one thread, no device, never CCMP_ENODEV — the
 * checker of the GPU tests and the CPU contender of tools/measure.py ik, as ccmp_pose_distance is for the metric.
 * CCMP_EINVAL: an invalid problem, options out of range, S out of range, T * S * 2 * (1 + restarts) >= 2^31, a NULL array with T > 0.
 * T == 0 returns CCMP_OK and touches nothing.  opts == NULL: the defaults. */
#define CCMP_IK_MAX_SEEDS 16
#define CCMP_IK_MAX_RESTARTS 31
#define CCMP_IK_MAX_ROUNDS 256
typedef struct ccmp_ik_opts {
  int32_t restarts;   /* 14   Gaussian restarts per (slot, arm) behind the seeded solve, 0..CCMP_IK_MAX_RESTARTS (jy_ConstrainedValidStateSampler.h:160) */
  int32_t max_rounds; /* 64   Newton steps per candidate at most, 1..CCMP_IK_MAX_ROUNDS */
  double eps;         /* 1e-5 per twist component, strictly below (TRAC-IK's default eps) */
  double lambda;      /* 0.05 damping */
  double err_clamp;   /* 0.5  the error vector's norm is clamped to this before a step */
  double sigma;       /* 0.3  standard deviation of the restarts (panda_tracik.cpp:70) */
} ccmp_ik_opts;
void ccmp_ik_opts_default(ccmp_ik_opts *opts);
int ccmp_pose_ik_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                       uint64_t rng_seed, uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds,
                       void *hip_stream);
int ccmp_pose_ik_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                      uint64_t rng_seed, uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds);
int ccmp_pose_ik_ref(const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S, uint64_t rng_seed,
                     uint64_t first_index, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds);
/* growTree's device part for Q poses in ONE call on one stream (stefanBiPRM.cpp:283-351), in this order: the object-metric k-NN of
 * query_poses [Q][8] on the store (k, mode, self_base as ccmp_roadmap_knn; k <= CCMP_IK_MAX_SEEDS); the neighbours' joint rows as seed
 * slots in rank order (an empty slot or a pose-only neighbour is a skipped slot); ccmp_pose_ik_batch on them; then edge e = q * k + r
 * from neighbour r to the new state through ccmp_roadmap_connect's own gather -> traversal -> fix chain, with its traversal arguments
 * and outputs unchanged in meaning (check_target = 0 is growTree's discreteGeodesic).  A target without a state makes all its slots
 * empty slots (ok = 0, n_states = 0, ...), as does a neighbour without joints: no NaN endpoint reaches a traversal kernel.
 * Additional outputs: q_new [Q][14], ik_ok [Q], ik_which [Q] (ccmp_pose_ik_batch's q_out, ok, which).  IT DOES NOT APPEND: the reference
 * adds the vertex only after an edge succeeded (stefanBiPRM.cpp:361) — the caller does, with ccmp_roadmap_append or set_joints. */
int ccmp_roadmap_grow(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts, const double *query_poses,
                      size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index, int check_target, int max_states,
                      int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok, int32_t *ik_which, double *states,
                      int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out, void *hip_stream);
int ccmp_roadmap_grow_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                           const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index,
                           int check_target, int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok,
                           int32_t *ik_which, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out);

/* ---- pose IK vetted against the proxy scene: IKValid and si_->isValid where the reference has them ---------------------------------- */
/* The reference gates every IK candidate with a collision test: sampleCalibGoal's _solveCalibIK / _randomsolveCalibIK are
 * ik_task_->solve(...) && IKvc_->IKValid(arm_idx, solution) (jy_ConstrainedValidStateSampler.h:192-199; IKValid is a collision test of
 * that one arm, KinematicChain.cpp:129-161, req.group_name = arm), and the function ends in si_->isValid(result) on the assembled
 * 14-joint state (:188).  Hence a seeded solution that collides loses to a restart that does not; among the restarts only collision-free
 * ones compete for "closest to the seed"; and growTree tries the next neighbour when the assembled state collides
 * (stefanBiPRM.cpp:294-302).  ccmp_pose_ik_* restate the rule WITHOUT the gate; these calls restate it WITH the gate, on the PROXY SCENE
 * (ccmp_scene_create) — this library's stand-in for MoveIt everywhere else, NOT MoveIt: si_->isValid(result) on the state they return
 * stays a host call.  csrc/ccmp_ik_vet.h states the rule in full:
 *   arm clearance   of arm a at seven joints: the smallest signed distance over the scene's tested pairs that contain no sphere moving on
 *                   the OTHER arm (a sphere moves on arm a on CCMP_FRAME(a, 0..7); world and base spheres are static); boxes included;
 *                   +inf for an empty set, NaN for a non-finite joint.  ccmp_clearance's arithmetic: bit-identical to ccmp_clearance_* on
 *                   the sub-scene made of the caller's spheres minus those moving on the other arm (whose seven joints are then free).
 *                   The scene's pairs are arm 0's, arm 1's and the cross pairs: full clearance = min(arm 0, arm 1, cross).
 *   admissible      a candidate that converged and whose arm clearance > margin (the rule of free_out)
 *   per arm         candidate 0 if admissible, else the admissible restart closest to the seed (ties to the lowest r), else failure
 *   slot            assembled when both arms succeed; it succeeds iff the full ccmp_clearance of its 14-joint row > margin (:188 — what
 *                   catches the cross pairs); the first slot that succeeds is the answer, else a NaN row, ok = 0, which = -1
 * HOW THIS DIFFERS FROM MoveIt's IKValid: the reference tests the arm against a robot state that still holds whatever the other arm was
 * last set to; here the arm is tested ALONE, and the pair of arms is tested on the assembled state.
 * margin = -inf gives ccmp_pose_ik_*'s answer bit for bit, margin = +inf fails every target; wherever the unvetted answer's own full
 * clearance is > margin the vetted answer is the same row, ok and which: vetting only ever adds solved targets.
 * ccmp_arm_clearance_*: IKValid(arm_index, sol) as a call of its own — q7 [B][7], clearance [B], free_out [B] (nullable) = clearance >
 * margin.  ccmp_pose_ik_vetted_*: ccmp_pose_ik_*'s arguments and outputs, plus (all nullable)
 *   cand_clear [T][S][2][1 + R]   the arm clearance of each converged candidate; -inf for one that did not converge or was skipped
 *   slot_clear [T][S]             the slot clearance; NaN where the slot was not assembled
 *   clearance [T]                 the chosen state's full clearance; NaN on failure
 * The *_batch forms take device pointers and are asynchronous on hip_stream (ccmp_pose_ik_vetted_batch: capturable after one eager call
 * at that size; candidate clearances and slot states live in a workspace of the context); the *_host forms take host pointers and are
 * synchronous on the context's stream; the *_ref forms are the same text compiled for the host, take the scene as the caller's arrays
 * (as ccmp_scene_create does), need no device and never answer CCMP_ENODEV.  Every check runs before the first launch.  CCMP_EINVAL:
 * what ccmp_pose_ik_* / ccmp_scene_create refuse, a NULL scene, a scene of another device, a NaN margin, arm outside 0..1.  A NULL context
 * is CCMP_ENODEV on a machine without a HIP device and CCMP_EINVAL otherwise. */
int ccmp_arm_clearance_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, int arm, const double *q7, size_t B, double margin,
                             double *clearance, uint8_t *free_out, void *hip_stream);
int ccmp_arm_clearance_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, int arm, const double *q7, size_t B, double margin,
                            double *clearance, uint8_t *free_out);
int ccmp_arm_clearance_ref(const ccmp_problem *p, const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes, const uint32_t allowed[32],
                           int arm, const double *q7, size_t B, double margin, double *clearance, uint8_t *free_out);
int ccmp_pose_ik_vetted_batch(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                              uint64_t rng_seed, uint64_t first_index, const ccmp_scene *scene, double margin, double *q_out, uint8_t *ok, int32_t *which,
                              double *cand_q, int32_t *cand_rounds, double *cand_clear, double *slot_clear, double *clearance, void *hip_stream);
int ccmp_pose_ik_vetted_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                             uint64_t rng_seed, uint64_t first_index, const ccmp_scene *scene, double margin, double *q_out, uint8_t *ok, int32_t *which,
                             double *cand_q, int32_t *cand_rounds, double *cand_clear, double *slot_clear, double *clearance);
int ccmp_pose_ik_vetted_ref(const ccmp_problem *p, const ccmp_ik_opts *opts, const double *target_poses, const double *seeds, size_t T, int S,
                            uint64_t rng_seed, uint64_t first_index, const ccmp_sphere *spheres, int n_spheres, const ccmp_box *boxes, int n_boxes,
                            const uint32_t allowed[32], double margin, double *q_out, uint8_t *ok, int32_t *which, double *cand_q, int32_t *cand_rounds,
                            double *cand_clear, double *slot_clear, double *clearance);
/* ccmp_roadmap_grow with the vetted IK in place of the plain one (growTree with IKValid inside sampleCalibGoal, stefanBiPRM.cpp:294-302),
 * plus ik_clearance [Q] (nullable): the new states' full clearances, NaN for a target without a state.  scene is REQUIRED and serves both
 * the IK and the traversals under the one margin; everything else — the gather, the empty-slot rule, the traversal chain — is
 * ccmp_roadmap_grow's.  CCMP_EINVAL additionally for a NULL scene or a NaN margin. */
int ccmp_roadmap_grow_vetted(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                             const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index, int check_target,
                             int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok, int32_t *ik_which,
                             double *ik_clearance, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out,
                             void *hip_stream);
int ccmp_roadmap_grow_vetted_host(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_ik_opts *opts,
                                  const double *query_poses, size_t Q, int k, int mode, size_t self_base, uint64_t rng_seed, uint64_t first_index,
                                  int check_target, int max_states, int round_budget, int32_t *nbr_idx, double *nbr_dist, double *q_new, uint8_t *ik_ok,
                                  int32_t *ik_which, double *ik_clearance, double *states, int32_t *n_states, uint8_t *ok, int32_t *newton_iters,
                                  uint8_t *blocked, double *carry_out);

/* ---- the head of growTree: object-pose proposal and the mesh-against-workspace test ------------------------------------------------ */
/* What the reference does before it grows (stefanBiPRM.cpp:255-276): interpolate the object pose 30 % from the nearest vertex towards the
 * goal, draw an SE(3) Gaussian sample around that (sigma 0.2, two attempts), ask stefan_checker_->isValid, and only then call
 * growTree(obj_state_); checkForSolution (:733-752) walks nine interpolated poses 0.1 i towards the goal and stops at the first pose the
 * checker refuses; stefanFCL::isFeasible (stefanFCL.h:115-138) tests the object's triangle mesh, moved by the pose, against six static
 * workspace boxes and answers "no" at the first that collides.  These calls close the loop (nearest pose, goal pose) -> vetted candidate
 * poses -> ccmp_roadmap_grow.
 * WHAT IS AND IS NOT RESTATED (csrc/ccmp_object.h states every term order): OMPL's SE3StateSpace::interpolate and its compound
 * sampleGaussian are restated from their published definitions in the rounding model of the rest of the library.  OMPL's random numbers
 * are not: the six unit deviates of a draw are Box-Muller on counter-based uniforms as the library's joint-space Gaussian sampler forms
 * them, counters rng_seed ^ (index 12 + 2 j) and rng_seed ^ (index 12 + 2 j + 1).  Nor is OMPL's uniform fall-back for wide rotations:
 * a sigma with 2 sigma / sqrt(3) > 1.44 is CCMP_EINVAL.  FCL's BVH and GJK code is not restated either: the mesh test is an exact
 * 13-axis separating-axis test of a triangle against an oriented box (unnormalised axes, no division, no square root; separated only by
 * a strict >, so touching is a hit; a degenerate triangle answers as the segment or point it is).  It answers the same geometric question
 * as FCL and is not comparable with it beyond that, as the proxy scene is not comparable with MoveIt.
 * MESHES ARE THE CALLER'S: triangles as numbers, [M][9] = x0 y0 z0 x1 y1 z1 x2 y2 z2 in the object frame, 1 <= M <=
 * CCMP_OBJECT_MAX_TRIANGLES.  The library hard-codes no workspace: 1 <= n_boxes <= CCMP_MAX_BOXES boxes of type ccmp_box, whose group is
 * ignored (half extents, not fcl::Box's side lengths).  Non-finite input: CCMP_EINVAL.
 * The pose rule: R from the quaternion by Eigen's toRotationMatrix arithmetic, not normalised (utils.h:22); world vertex = R v + p;
 * hit_mask bit b set iff any triangle hits box b with its half extents enlarged by inflate (finite, >= 0); valid = (hit_mask == 0).  A pose
 * with a non-finite component gives valid = 0, hit_mask = 0: nothing was tested.  A broad phase (the mesh's bounding sphere, computed at
 * creation with a slack that rounding cannot eat, against each box) skips boxes a pose cannot reach; it never changes an answer.
 *   create / destroy   the object lives on the context's device, remembers its context and follows the life-cycle rules of scenes: destroy
 *                      quiesces the context first; the context must outlive the object or be destroyed first with its service off.  Argument
 *                      checks come first; a NULL context then answers CCMP_ENODEV on a machine without a HIP device, CCMP_EINVAL otherwise.
 *   valid_batch        poses [T][8] -> valid [T] (uint8), hit_mask [T] (uint32, nullable).  One 256-lane block per pose.  With hit_mask
 *                      the mask is complete; without it a block leaves after the first 256 triangles among which one hit (the reference's
 *                      early return) — valid is the same either way.  Device pointers, asynchronous on hip_stream, capturable.
 *   propose_batch      grow index g, attempt a = 0 .. attempts - 1 (1 <= attempts <= CCMP_OBJECT_MAX_ATTEMPTS): the candidate is the
 *                      interpolation from from_poses[g] towards to_poses[g] (to_stride 8) or to_poses[0] (to_stride 0) at t, then the
 *                      Gaussian draw of index (first_index + g) attempts + a around it with sigma, its position clamped into [lo, hi];
 *                      sigma == 0 makes the candidate the interpolated pose itself.  pose_out [G][8] = the first valid candidate and
 *                      which [G] = its attempt, or a NaN row (pad 0) and -1.  cand_pose [G][attempts][8] and cand_valid [G][attempts]
 *                      (both nullable): every attempt, and all of them then run.  A total order over attempts: no launch shape changes the
 *                      result, and a call over G indices equals G calls over one with the matching first_index.
 *   *_host             the same calls on host buffers, synchronous on the context's stream.
 *   *_ref              THE SAME TEXT COMPILED FOR THE HOST: raw triangles and boxes instead of a handle, one thread, no device, never
 *                      CCMP_ENODEV.  The valid form takes broad_phase (0 switches it off: the answers must not change).
 * The device and host forms answer a NULL context with CCMP_ENODEV on a machine without a HIP device and with CCMP_EINVAL otherwise;
 * every check runs before the first launch.  CCMP_EINVAL: M or n_boxes out of range, non-finite mesh, box, inflate, t or sigma, a
 * negative inflate or sigma, the rotation limit above, lo > hi or NaN bounds, attempts out of range, to_stride not 0 or 8, T or G >= 2^31,
 * an object of another device than the context's, a NULL array with T or G > 0.  T == 0 / G == 0 returns CCMP_OK and touches nothing.
 * Where a result is NaN (a candidate of a non-finite pose, the row of a grow index without a valid attempt) it is some NaN: its sign and
 * payload are not specified.
 * ccmp_pose_interpolate is pure host code beside ccmp_pose_distance and gives the same bits as the kernels. */
#define CCMP_OBJECT_MAX_TRIANGLES 16384
#define CCMP_OBJECT_MAX_ATTEMPTS 16
typedef struct ccmp_object ccmp_object;
void ccmp_pose_interpolate(const double a[8], const double b[8], double t, double out[8]);
int ccmp_object_create(ccmp_ctx *ctx, const double *tri, int M, const ccmp_box *boxes, int n_boxes, ccmp_object **out);
void ccmp_object_destroy(ccmp_object *obj);
int ccmp_object_num_triangles(const ccmp_object *obj);
int ccmp_object_valid_batch(ccmp_ctx *ctx, const ccmp_object *obj, const double *poses, size_t T, double inflate, uint8_t *valid, uint32_t *hit_mask,
                            void *hip_stream);
int ccmp_object_valid_host(ccmp_ctx *ctx, const ccmp_object *obj, const double *poses, size_t T, double inflate, uint8_t *valid, uint32_t *hit_mask);
int ccmp_object_valid_ref(const double *tri, int M, const ccmp_box *boxes, int n_boxes, const double *poses, size_t T, double inflate, int broad_phase,
                          uint8_t *valid, uint32_t *hit_mask);
int ccmp_object_propose_batch(ccmp_ctx *ctx, const ccmp_object *obj, const double *from_poses, const double *to_poses, int to_stride, size_t G, double t,
                              double sigma, const double lo[3], const double hi[3], int attempts, uint64_t rng_seed, uint64_t first_index, double inflate,
                              double *pose_out, int32_t *which, double *cand_pose, uint8_t *cand_valid, void *hip_stream);
int ccmp_object_propose_host(ccmp_ctx *ctx, const ccmp_object *obj, const double *from_poses, const double *to_poses, int to_stride, size_t G, double t,
                             double sigma, const double lo[3], const double hi[3], int attempts, uint64_t rng_seed, uint64_t first_index, double inflate,
                             double *pose_out, int32_t *which, double *cand_pose, uint8_t *cand_valid);
int ccmp_object_propose_ref(const double *tri, int M, const ccmp_box *boxes, int n_boxes, const double *from_poses, const double *to_poses, int to_stride,
                            size_t G, double t, double sigma, const double lo[3], const double hi[3], int attempts, uint64_t rng_seed, uint64_t first_index,
                            double inflate, double *pose_out, int32_t *which, double *cand_pose, uint8_t *cand_valid);

/* ---- the roadmap graph on the device: edges, components and growTree's tail ------------------------------------------------------------ */
/* The store also keeps the graph: a device edge list uv [E][2] (int32) with weights w [E] (double), and one int32 LABEL per vertex,
 *     label[v] = the smallest vertex index in v's connected component
 * — a function of the edge set alone, fully compressed between calls; an append writes label[i] = i.  The handle keeps the edge count
 * and an EDGE FLOOR (1 + the largest endpoint of any edge) as host state: ccmp_roadmap_truncate(n) with n below the floor answers
 * CCMP_EINVAL (the reference only ever removes a vertex without an edge, stefanBiPRM.cpp:353-359, :375-378).
 *
 * ccmp_roadmap_commit is what follows the traversals in growTree (stefanBiPRM.cpp:303-372, milestonesToAdd :420-445), addMilestone and,
 * with CCMP_COMMIT_KEEP_ISOLATED, startgoalMilestone; the outputs of ccmp_roadmap_grow / ccmp_roadmap_connect go in unchanged.  For query
 * q and slot r < k (N = the store's size at entry) the slot is
 *     empty      nbr_idx < 0 (or >= N)
 *     unsettled  edge_ok == 2 or n_states > max_states: a continuation is still due
 *     reached    edge_ok == 1
 *     failed     otherwise
 * and, with L = the labels at call entry and root(l) = l is the label of one of roots[0 .. n_roots) (the planner's startM_):
 *     vertex_ok[q] == 0            -> TRAPPED, nothing committed
 *     any slot unsettled           -> UNSETTLED, nothing committed for q
 *     joined = {}, joined_start = false
 *     for r = 0 .. k-1:
 *       reached: edge (nbr, t), weight = joint distance; joined += L[nbr]; joined_start |= root(L[nbr])
 *       failed, a goal pose given, n_states > 1, and (root(L[nbr]) or (L[nbr] in joined and joined_start)):
 *           m = pose of states[q][r][n_states-1]
 *           if dist(m, goal) < dist(pose[nbr], goal)  (strict; a NaN never passes):
 *               mid-stone r = vertex (that state, m) + edge (nbr, mid)
 *     added = any slot reached;  t is kept iff added or KEEP_ISOLATED
 *     state = !added ? TRAPPED : joined_start ? SREACHED : GREACHED
 * (the second arm of the component test is the reference's: sameComponent_start(n) is asked inside the neighbour loop, after the earlier
 * successful edges of the same vertex have been united).  New indices are taken in a total order: for ascending q, t if kept, then its
 * mid-stones in r order; edges likewise: the reached edges of q in r order, then its mid-stone edges, each as (neighbour, new vertex).
 * The queries of one call do not see each other; with Q == 1 the rule is the reference's.  Weights are the joint distance of the k-NN
 * (FMA chain over the 14 differences, correctly rounded root); the pose of a state is what an append derives; distances are
 * ccmp_pose_distance.  csrc/ccmp_graph.h states all of it once, for the kernels and for the *_ref forms.
 *   commit      inputs (device pointers): nbr_idx [Q][k], edge_ok [Q k], n_states [Q k], states [Q k][max_states][14] (NULL: no
 *               mid-stones), new_joints [Q][14], new_poses [Q][8], vertex_ok [Q] (NULL: all 1).  Host arguments: p (may be NULL when states
 *               or goal_pose is), goal_pose[8] (NULL: no mid-stones), roots[n_roots] (0 <= n_roots <= CCMP_GRAPH_MAX_ROOTS, each < size),
 *               flags.  Outputs (device pointers): new_index [Q] (-1: not kept), mid_index [Q][k] (-1: none), grow_state [Q]; host:
 *               *vertices_added, *edges_added (nullable).  The worst case (Q (1 + k) rows, Q k edges) is reserved before the first launch;
 *               the call ends with one small read-back (the counts and the new edge floor): IT IS SYNCHRONOUS AT ITS END AND NOT CAPTURABLE.
 *   add_edges   explicit uv [E][2]; the weights (joint distance) are computed on the device.  An endpoint outside [0, size) or u == v:
 *               CCMP_EINVAL from the _host form (checked on the host); the device form skips such an edge and counts it in *rejected
 *               (nullable).  Synchronous at its end like commit.
 *   num_edges / read_edges (uv_out [count][2], w_out [count], either may be NULL) / read_labels (labels_out [count])   as read.
 *   closest     closestFromGoal's vertex scan (stefanBiPRM.cpp:675-684): for each of from_idx [F], 1 <= F <= CCMP_CLOSEST_MAX_FROM, the
 *               vertex with the smallest (ccmp_pose_distance(pose[i], target_pose), i) among those with label[i] == label[from]: idx [F],
 *               dist [F]; from_dist [F] = the distance of `from` itself.  A NaN distance is never a candidate (none at all: idx -1, dist
 *               +inf).  target_pose[8] is a device pointer in the device form.  Asynchronous and capturable.  A `from` outside [0, size):
 *               CCMP_EINVAL from the _host and _ref forms; the device form answers idx -1, dist +inf, from_dist NaN.
 *   *_ref       the same text on host arrays, one thread, no device, never CCMP_ENODEV.  commit_ref takes the store's raw arrays (joints
 *               [N][14], poses [N][8], labels [N]) and returns the appended rows (rows_joints [Q (1 + k)][14], rows_poses [..][8]) and edges
 *               (edges_uv [Q k][2], edges_w [Q k]), of which the first *vertices_added / *edges_added are written.
 *   ccmp_graph_labels_ref   plain host union-find: uv [E][2] over N vertices -> labels [N]; CCMP_EINVAL for an endpoint outside [0, N) or
 *               u == v, as add_edges_host.
 *   ccmp_joint_distance     the edge weight of two joint states; pure host code beside ccmp_pose_distance.
 * Conventions as the store's other entries: every check runs before the first launch; a NULL store answers CCMP_ENODEV without a device
 * and CCMP_EINVAL with one; zero counts return CCMP_OK and touch nothing.  The path search runs on the device too (the next section);
 * read_edges remains for callers that want the graph itself. */
#define CCMP_GRAPH_MAX_ROOTS 32
#define CCMP_CLOSEST_MAX_FROM 64
enum { CCMP_GROW_TRAPPED = 0, CCMP_GROW_SREACHED = 1, CCMP_GROW_GREACHED = 2, CCMP_GROW_UNSETTLED = 3 };
enum { CCMP_COMMIT_KEEP_ISOLATED = 1 };
double ccmp_joint_distance(const double a[14], const double b[14]);
int ccmp_graph_labels_ref(const int32_t *uv, size_t E, size_t N, int32_t *labels);
int ccmp_roadmap_commit(ccmp_roadmap *rm, const ccmp_problem *p, const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states,
                        const double *states, int max_states, const double *new_joints, const double *new_poses, const uint8_t *vertex_ok, size_t Q, int k,
                        const double *goal_pose, const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index,
                        int32_t *grow_state, size_t *vertices_added, size_t *edges_added, void *hip_stream);
int ccmp_roadmap_commit_host(ccmp_roadmap *rm, const ccmp_problem *p, const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states,
                             const double *states, int max_states, const double *new_joints, const double *new_poses, const uint8_t *vertex_ok, size_t Q,
                             int k, const double *goal_pose, const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index,
                             int32_t *grow_state, size_t *vertices_added, size_t *edges_added);
int ccmp_roadmap_commit_ref(const ccmp_problem *p, const double *store_joints, const double *store_poses, const int32_t *labels, size_t N,
                            const int32_t *nbr_idx, const uint8_t *edge_ok, const int32_t *n_states, const double *states, int max_states,
                            const double *new_joints, const double *new_poses, const uint8_t *vertex_ok, size_t Q, int k, const double *goal_pose,
                            const int32_t *roots, int n_roots, unsigned int flags, int32_t *new_index, int32_t *mid_index, int32_t *grow_state,
                            double *rows_joints, double *rows_poses, int32_t *edges_uv, double *edges_w, size_t *vertices_added, size_t *edges_added);
int ccmp_roadmap_add_edges(ccmp_roadmap *rm, const int32_t *uv, size_t E, size_t *rejected, void *hip_stream);
int ccmp_roadmap_add_edges_host(ccmp_roadmap *rm, const int32_t *uv, size_t E);
size_t ccmp_roadmap_num_edges(const ccmp_roadmap *rm);
int ccmp_roadmap_read_edges(ccmp_roadmap *rm, size_t first, size_t count, int32_t *uv_out, double *w_out, void *hip_stream);
int ccmp_roadmap_read_edges_host(ccmp_roadmap *rm, size_t first, size_t count, int32_t *uv_out, double *w_out);
int ccmp_roadmap_read_labels(ccmp_roadmap *rm, size_t first, size_t count, int32_t *labels_out, void *hip_stream);
int ccmp_roadmap_read_labels_host(ccmp_roadmap *rm, size_t first, size_t count, int32_t *labels_out);
int ccmp_roadmap_closest(ccmp_roadmap *rm, const int32_t *from_idx, size_t F, const double *target_pose, int32_t *idx, double *dist, double *from_dist,
                         void *hip_stream);
int ccmp_roadmap_closest_host(ccmp_roadmap *rm, const int32_t *from_idx, size_t F, const double *target_pose, int32_t *idx, double *dist,
                              double *from_dist);
int ccmp_roadmap_closest_ref(const double *store_poses, const int32_t *labels, size_t N, const int32_t *from_idx, size_t F, const double *target_pose,
                             int32_t *idx, double *dist, double *from_dist);

/* ---- shortest paths on the store's graph: the planner's solution step ------------------------------------------------------------ */
/* constructSolution, maybeConstructSolution and constructApproximateSolution (stefanBiPRM.cpp:161-239, :480-603) need the cheapest path
 * from a start vertex to a goal vertex as joint states.  One call answers 1 <= F <= CCMP_PATH_MAX_PAIRS pairs (src[f], dst[f]) on the
 * store's graph as it stands (undirected edges, the stored weights, parallel edges allowed) without taking it off the device.  The rule
 * (csrc/ccmp_path.h states it once, for the kernels and for the _ref form; fl(a + b) is one IEEE double addition), for one source s:
 *     candidate   over an edge {u, v} from u: c = fl(d[u] + w); it passes iff d[u] is finite, w >= 0 and c is finite — a NaN never passes
 *                 (an edge at a pose-only vertex has a NaN weight and is never traversed), nor does a sum that overflowed
 *     distance    d = the least fixed point of d[s] = +0.0, d[v] = min over the passing candidates into v; unreached: +inf.  The fixed
 *                 point is unique (fl(a + w) is non-decreasing in a and >= a), so the result is a function of the edge set alone, bit
 *                 for bit: Dijkstra, Bellman-Ford in any order and atomicMin arriving in any order reach the same values, with zero
 *                 weights and absorbed weights (fl(d + w) == d) included
 *     tight edge  u -> v: the candidate from u passes and equals d[v]
 *     hops        hops[v] = the breadth-first level of v from s in the directed graph of tight edges
 *     pred        pred[v] = the smallest u with a tight edge u -> v and hops[u] == hops[v] - 1 (-1 for s and for an unreached vertex):
 *                 acyclic by construction, where a rule on distances or indices would not be
 *     path        s -> t has hops[t] + 1 vertices (the walk of pred from t, written forwards); its cost d[t] is the left-to-right fl sum
 *                 of its weights.  s == t: length 1, cost +0.0.  t unreached: length 0, cost +inf.
 * THIS IS NOT boost's A*: the reference guides its search by the SE3 object distance (costHeuristic) while its weights are joint
 * distances; that heuristic is not admissible for these weights, so the reference's path need not be the cheapest.  This one is (its
 * cost is never above the reference's), and ties are broken by the rule above, not by heap order.
 *   shortest_paths   device pointers: src [F], dst [F]; outputs cost [F], path_len [F], path [F][max_len] (int32, the first path_len[f]
 *                    entries of row f), and, each nullable, path_joints [F][max_len][14], path_poses [F][max_len][8] (the store's rows at
 *                    those indices), dist_out [F][N] and pred_out [F][N] (N = the store's size).  A path longer than max_len reports its
 *                    length and leaves row f of path and of the rows untouched: call again with more room.  A src or dst outside
 *                    [0, size): length 0, cost NaN.  The per-pair arrays live in a workspace on the handle, grown before the first
 *                    launch (F N 20 bytes), allocated only when this call is used and freed with the store.  N and the edge count are
 *                    host state: the call is asynchronous on its stream, and capturable once the workspace holds F N (the first call
 *                    at a size grows it: never capture that one).
 *   _host            host pointers, synchronous on the context's stream; a src or dst outside [0, size) is CCMP_EINVAL, checked on the host.
 *   ccmp_graph_shortest_paths_ref   pure host code on uv [E][2], w [E] over N vertices, one thread, no device, never CCMP_ENODEV: distances
 *                    by HEAP DIJKSTRA (another algorithm than the kernel's rounds), hops and predecessors from the same rule text.
 *                    CCMP_EINVAL for an endpoint outside [0, N) or u == v (as add_edges_host) and for a src or dst outside [0, N).
 *   path_rounds_host   the relaxation and hop rounds ([F][2]) the store's last shortest_paths call took per pair; a diagnostic.
 * Conventions as above: every check runs before the first launch; a NULL store answers CCMP_ENODEV without a device and CCMP_EINVAL
 * with one; F == 0 returns CCMP_OK and touches nothing; F > CCMP_PATH_MAX_PAIRS, max_len < 1 or a NULL src, dst, cost, path_len or path
 * is CCMP_EINVAL.  The step behind it, PathGeometric::interpolate over the returned rows, is ccmp_path_densify below. */
#define CCMP_PATH_MAX_PAIRS 64
int ccmp_roadmap_shortest_paths(ccmp_roadmap *rm, const int32_t *src, const int32_t *dst, size_t F, int max_len, double *cost, int32_t *path_len,
                                int32_t *path, double *path_joints, double *path_poses, double *dist_out, int32_t *pred_out, void *hip_stream);
int ccmp_roadmap_shortest_paths_host(ccmp_roadmap *rm, const int32_t *src, const int32_t *dst, size_t F, int max_len, double *cost, int32_t *path_len,
                                     int32_t *path, double *path_joints, double *path_poses, double *dist_out, int32_t *pred_out);
int ccmp_graph_shortest_paths_ref(const int32_t *uv, const double *w, size_t E, size_t N, const int32_t *src, const int32_t *dst, size_t F, int max_len,
                                  double *cost, int32_t *path_len, int32_t *path, double *dist_out, int32_t *pred_out);
int ccmp_roadmap_path_rounds_host(ccmp_roadmap *rm, size_t F, int32_t *rounds);

/* ---- dense solution paths: PathGeometric::interpolate on the device --------------------------------------------------------------- */
/* ConstrainedProblem::solveOnce (ConstrainedPlanningCommon.cpp:207-222) runs PathGeometric::interpolate on the planner's solution and
 * prints the result as <obj>_path.txt.  One call takes F >= 0 paths as waypoint rows on the device — path_joints [F][max_len][14] and
 * path_len [F], the shapes ccmp_roadmap_shortest_paths writes — and returns them dense; the state lists never leave the device.  The
 * rule (csrc/ccmp_dense.h states it once, for the kernels and for the host forms); path f has L = path_len[f] waypoints w_0 .. w_{L-1}:
 *     segment list   G_i = the state list of ONE uninterrupted discreteGeodesic(w_i, w_{i+1}, interpolate = true)
 *                    (jy_ProjectedStateSpace.cpp:32-96): n_i >= 1 states, G_i[0] = w_i; seg_ok[i] its return value, seg_newton[i] its Newton
 *                    total.  The library cuts a traversal into extend calls of chunk_states list entries and round_budget Newton rounds
 *                    (ccmp_geodesic_batch_ex with carries) and continues every open segment until none is left: lists, flag and count
 *                    are those of one traversal, bit for bit, whatever the cut.  The problem's Jacobian mode decides the arithmetic.
 *     reference      flags = 0: w_0, G_0, w_1, G_1, .., w_{L-2}, G_{L-2}, w_{L-1} — sum (1 + n_i) + 1 rows, each w_i with i < L - 1 twice in a
 *     layout         row, as PathGeometric::interpolate followed by printAsMatrix writes them.  L == 1: one row.  L == 0: none.
 *     distinct       CCMP_DENSE_DISTINCT: G_0, G_1, .., G_{L-2}, w_{L-1} — sum n_i + 1 rows: the layout for executing the path.
 *     unreached      a segment with seg_ok = 0 contributes the rows it has and the next waypoint follows: the path has a jump there, as
 *                    the reference's own output has (Wine_Bottle_path.txt, segment 1).  Not an error.
 *     offsets        paths are packed one after another: path_first [F + 1] (path_first[F] = the row count), seg_first [F][max_len - 1] =
 *                    the first row of G_i, -1 for a slot without a segment (seg_ok and seg_newton are 0 there).
 *     arc            arc[path_first[f]] = +0.0, arc[r] = fl(arc[r-1] + ccmp_joint_distance(row[r-1], row[r])) within a path; length[f] = the
 *                    arc of the path's last row, +0.0 for an empty path.  A duplicated row adds exactly +0.0: both layouts carry the
 *                    same arcs at corresponding rows.
 *     clearance      only with a proxy scene: clearance[r] = ccmp_clearance_batch's value for row r; per path min_clear, min_row (the
 *     summary        first row attaining it; rows are numbered over the whole result) and first_blocked (the first row with clearance <
 *                    margin, -1: none).  A NaN never attains the minimum.  Empty path: +inf, -1, -1.  A pre-filter, as every proxy result.
 *   ccmp_path_densify   device pointers.  SYNCHRONOUS on its stream (it reads 5 bytes per open segment after every extend call to drive
 *                    the continuation, and path_len once, before any launch): not capturable.  It returns a handle, because the row
 *                    count is known only afterwards and no caller should pay for the traversal twice.  opts == NULL: the defaults.  With
 *                    max_calls extend calls spent and a segment still open: CCMP_EOVERFLOW, and no handle — a cut list never looks complete.
 *   _host            host pointers, on the context's stream.
 *   ccmp_dense_paths_info / _copy / _copy_host / _destroy   the result: F, max_len, the row count, the extend calls made; copies into
 *                    device (asynchronous on hip_stream) or host (synchronous) destinations, each nullable: rows_out [rows][14],
 *                    path_first [F + 1], seg_first / seg_ok / seg_newton [F][max_len - 1], arc [rows], length [F], clearance [rows],
 *                    min_clear / min_row / first_blocked [F] (the last four: CCMP_EINVAL if asked of a result made without a scene).
 *   ccmp_dense_layout_ref   the layout alone, pure host code, no device: from path_len and seg_states [F][max_len - 1] (the n_i; entries of
 *                    slots without a segment are not read) it writes path_first, seg_first (each nullable) and *rows.  CCMP_EINVAL for
 *                    a path_len outside [0, max_len], an n_i < 1, unknown flags, max_len < 1 or a NULL path_len, seg_states (where a
 *                    segment exists) or rows; CCMP_EOVERFLOW beyond 2^31 - 1 rows.
 *   ccmp_dense_arc_ref   the arc rule alone, pure host code: arc [rows] and length [F] (nullable) from rows and path_first.  CCMP_EINVAL for
 *                    a NULL path_first, a path_first that is negative or decreases, or NULL rows / arc where rows exist.
 * Conventions as above: every check runs before the first launch; a NULL context answers CCMP_ENODEV without a device and CCMP_EINVAL
 * with one; F == 0 gives an empty result (0 rows, path_first = {0}).  CCMP_EINVAL: chunk_states < 2, round_budget < 0, max_calls < 1,
 * unknown flags, max_len < 1, a path_len entry outside [0, max_len] (one that ccmp_roadmap_shortest_paths reported as "did not fit" lands
 * here), a scene of another device, a NaN margin with a scene, NULL path_joints, path_len or out. */
#define CCMP_DENSE_DISTINCT 1
typedef struct ccmp_dense_opts {
  int flags;        /* 0 or CCMP_DENSE_DISTINCT */
  int chunk_states; /* list entries per extend call, >= 2 */
  int round_budget; /* Newton rounds per segment and extend call, 0 = no bound */
  int max_calls;    /* extend calls at most */
} ccmp_dense_opts;
/* 0, 16, 128, 4096: the list length and round budget the extend step's bulk calls settled on */
void ccmp_dense_opts_default(ccmp_dense_opts *opts);
typedef struct ccmp_dense_paths ccmp_dense_paths;
int ccmp_path_densify(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                      size_t F, int max_len, const ccmp_dense_opts *opts, ccmp_dense_paths **out, void *hip_stream);
int ccmp_path_densify_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints,
                           const int32_t *path_len, size_t F, int max_len, const ccmp_dense_opts *opts, ccmp_dense_paths **out);
int ccmp_dense_paths_info(const ccmp_dense_paths *h, size_t *F, int *max_len, size_t *rows, int *calls);
int ccmp_dense_paths_copy(ccmp_dense_paths *h, double *rows_out, int32_t *path_first, int32_t *seg_first, uint8_t *seg_ok, int32_t *seg_newton, double *arc,
                          double *length, double *clearance, double *min_clear, int32_t *min_row, int32_t *first_blocked, void *hip_stream);
int ccmp_dense_paths_copy_host(ccmp_dense_paths *h, double *rows_out, int32_t *path_first, int32_t *seg_first, uint8_t *seg_ok, int32_t *seg_newton,
                               double *arc, double *length, double *clearance, double *min_clear, int32_t *min_row, int32_t *first_blocked);
void ccmp_dense_paths_destroy(ccmp_dense_paths *h);
int ccmp_dense_layout_ref(const int32_t *path_len, size_t F, int max_len, const int32_t *seg_states, int flags, int32_t *path_first, int32_t *seg_first,
                          size_t *rows);
int ccmp_dense_arc_ref(const double *rows, const int32_t *path_first, size_t F, double *arc, double *length);

/* ---- shortcut solution paths: the removal of interior vertices on the device ------------------------------------------------------- */
/* What comes out of ccmp_roadmap_shortest_paths is a roadmap path: it visits every milestone the tree happened to grow through.  OMPL
 * removes interior vertices by trying random pairs, one checkMotion at a time (PathSimplifier::reduceVertices); here every pair of a path
 * is tested in one batch and the cheapest path over the pairs that passed is taken — the optimum any sequence of vertex removals could
 * reach, deterministic, a function of the inputs alone, bit for bit.  The rule (csrc/ccmp_shortcut.h states it once, for the kernels, the
 * host forms and the _ref forms); path f has L = path_len[f] waypoints w_0 .. w_{L-1}, rows of path_joints [F][max_len][14]:
 *     candidate      a pair (i, j), 0 <= i, j < L, with j - i >= 2, j - i <= max_span (max_span == 0: every span) and both rows finite in all
 *                    14 coordinates; candidates are enumerated in (f, i, j) order.
 *     test           ONE uninterrupted checkMotion(w_i, w_j), forwards only: isSatisfied(w_j), then discreteGeodesic(w_i, w_j)
 *                    (ccmp_geodesic_batch_ex with check_target = 1 on the first call; with a proxy scene ccmp_geodesic_scene_batch and its
 *                    margin: the traversal breaks at the first refused state).  pair_ok[i][j] = its return value, pair_states[i][j] = its
 *                    list length, pair_newton[i][j] = its Newton total.  The library cuts traversals into extend calls of chunk_states
 *                    list entries and round_budget Newton rounds over tiles of at most tile_edges pairs and continues every open pair
 *                    until none is left: flag, count and total are those of one traversal, bit for bit, whatever the cut.  Only the last
 *                    stored state and the carry of an open pair are kept: no state lists.  Entries that are no candidates are 0.
 *     admitted edge  i -> j with j == i + 1 (the roadmap's own edge: never tested) or pair_ok[i][j] == 1.
 *     weight         w(i, j) = ccmp_joint_distance(w_i, w_j): what commit stores as motionCost.
 *     selection      the rule of ccmp_roadmap_shortest_paths on this DAG from source 0: d[0] = +0.0, d[j] = min over admitted i < j of
 *                    fl(d[i] + w(i, j)), a candidate passing iff d[i] is finite, w >= 0 and the sum is finite; hops[j] = the least
 *                    hops[i] + 1 over tight i; pred[j] = the smallest tight i with hops[i] == hops[j] - 1.  One forward sweep is exact.
 *     result         kept [F][max_len] = the walk of pred from L - 1 written forwards, -1 behind it; out_len [F] = its length; out_joints
 *                    [F][max_len][14] = the kept rows, bit for bit (rows behind out_len are untouched); cost_in [F] = the left-to-right fl
 *                    sum of the adjacent weights; cost_out [F] = d[L - 1].  L == 1: kept {0}, costs +0.0.  L == 0: nothing, costs +0.0.
 *                    d[L - 1] == +inf (an adjacent weight is NaN or infinite, e.g. a pose-only vertex): the path comes back unchanged —
 *                    identity kept — with cost_out = +inf.
 * The result does not depend on tile_edges, chunk_states, round_budget or launch shape.
 *   ccmp_path_shortcut   device pointers.  pair_ok (uint8), pair_states, pair_newton (int32), each [F][max_len][max_len], are nullable.
 *                    SYNCHRONOUS on its stream (it reads 5 bytes per open pair after every extend call, and path_len once, before any
 *                    launch): not capturable.  opts == NULL: the defaults.  max_calls extend calls spent on a tile with a pair still open:
 *                    CCMP_EOVERFLOW, every output untouched.  A shortcut leaves the edges the host validated: densify the result
 *                    (ccmp_path_densify) and put the dense rows to the host's validity test.
 *   _host            host pointers, on the context's stream.
 *   ccmp_shortcut_select   the selection alone on a caller's pair_ok (any edge test: the host's MoveIt verdicts, say): asynchronous on its
 *                    stream, capturable; path_len is read on the device, an entry outside [0, max_len] is taken as 0.  _host: host
 *                    pointers, synchronous; a path_len entry outside [0, max_len] is CCMP_EINVAL.
 *   ccmp_shortcut_select_ref   the same rule text on host pointers, one thread, no device, never CCMP_ENODEV.
 *   ccmp_shortcut_pairs_ref    the candidate enumeration, pure host code: triples [capacity][3] = (f, i, j) in order (nullable: count only)
 *                    and *count; CCMP_EOVERFLOW when capacity is too small (*count is still the number there is).
 * Conventions as the dense section's: every check runs before the first launch; a NULL context answers CCMP_ENODEV without a device and
 * CCMP_EINVAL with one; F == 0 returns CCMP_OK and touches nothing.  CCMP_EINVAL: a path_len entry outside [0, max_len], max_len < 1 or
 * > CCMP_SHORTCUT_MAX_LEN, max_span < 0, tile_edges < 1, chunk_states < 2, round_budget < 0, max_calls < 1, an output overlapping an input,
 * a NULL path_joints, path_len, out_joints, out_len, kept, cost_in or cost_out (select: pair_ok too), a scene of another device, a NaN
 * margin with a scene. */
#define CCMP_SHORTCUT_MAX_LEN 1024
typedef struct ccmp_shortcut_opts {
  int max_span;     /* candidates span at most this many waypoints, 0 = every span */
  int chunk_states; /* list entries per extend call, >= 2 */
  int round_budget; /* Newton rounds per pair and extend call, 0 = no bound */
  int max_calls;    /* extend calls at most, per tile */
  int tile_edges;   /* pairs per tile, >= 1 */
} ccmp_shortcut_opts;
/* 0, 16, 128, 4096, 65536 */
void ccmp_shortcut_opts_default(ccmp_shortcut_opts *opts);
int ccmp_path_shortcut(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                       size_t F, int max_len, const ccmp_shortcut_opts *opts, double *out_joints, int32_t *out_len, int32_t *kept, double *cost_in,
                       double *cost_out, uint8_t *pair_ok, int32_t *pair_states, int32_t *pair_newton, void *hip_stream);
int ccmp_path_shortcut_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints,
                            const int32_t *path_len, size_t F, int max_len, const ccmp_shortcut_opts *opts, double *out_joints, int32_t *out_len,
                            int32_t *kept, double *cost_in, double *cost_out, uint8_t *pair_ok, int32_t *pair_states, int32_t *pair_newton);
int ccmp_shortcut_select(ccmp_ctx *ctx, const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok,
                         double *out_joints, int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out, void *hip_stream);
int ccmp_shortcut_select_host(ccmp_ctx *ctx, const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok,
                              double *out_joints, int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out);
int ccmp_shortcut_select_ref(const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok, double *out_joints,
                             int32_t *out_len, int32_t *kept, double *cost_in, double *cost_out);
int ccmp_shortcut_pairs_ref(const double *path_joints, const int32_t *path_len, size_t F, int max_len, int max_span, int32_t *triples, size_t capacity,
                            size_t *count);

/* ---- smooth solution paths: B-spline passes on the manifold ----------------------------------------------------------------------- */
/* A roadmap path, shortcut or not, is a polygon with a corner at every kept vertex, and the corners are what the arms execute.  This is
 * the structure of OMPL's PathSimplifier::smoothBSpline — subdivide, then move every original vertex towards the middle of its two new
 * neighbours — with this project's midpoint, not OMPL's arithmetic.  A pass is data-parallel as written (only the original vertices move,
 * each reads only its two new neighbours, no pass moves a new neighbour), so every segment and every interior vertex of every path goes
 * into one batch per stage.  The rule (csrc/ccmp_smooth.h states it once, for the kernels, the host forms and the _ref forms); path f has
 * L = path_len[f] waypoints w_0 .. w_{L-1}, rows of path_joints [F][max_len][14]:
 *     closed list    of a pair (a, b): the distinct dense rows of the two-waypoint path [a, b] (the dense section): G = the list of ONE
 *                    uninterrupted discreteGeodesic(a, b, interpolate = true), then b; n >= 2 rows, arcs s_0 = +0.0,
 *                    s_k = fl(s_{k-1} + ccmp_joint_distance(row_{k-1}, row_k)).
 *     midpoint       mid(a, b): T = s_{n-1}, h = 0.5 T.  Not T > 0: mid = a (degenerate).  Otherwise k = the smallest k >= 1 with s_k >= h,
 *                    t = (h - s_{k-1}) / (s_k - s_{k-1}) (IEEE division, the denominator positive by construction), x =
 *                    WrapperStateSpace::interpolate(row_{k-1}, row_k, t) (the extend step's), (y, ok) = project(x); ok: mid = y
 *                    (projected); not ok: mid = row_{k-1} when (h - s_{k-1}) <= (s_k - h), else row_k (fallback).  The midpoint is the
 *                    blend at half the arc put back on the manifold and not the list state nearest to it: lists have one to seven states at
 *                    the planner's delta, so list-state midpoints coincide with waypoints after one pass.
 *     one pass       (L >= 3) m_i = mid(w_i, w_{i+1}) per segment; per interior i: t1 = mid(m_{i-1}, w_i), t2 = mid(w_i, m_i), c_i =
 *                    mid(t1, t2).  c_i is accepted iff checkMotion(m_{i-1}, c_i) and checkMotion(c_i, m_i) pass (each isSatisfied(target),
 *                    then one uninterrupted discreteGeodesic, forwards, as the shortcut section's test; with a proxy scene
 *                    ccmp_geodesic_scene_batch with the margin, and also clearance(m_{i-1}) >= margin and clearance(c_i) >= margin, a NaN
 *                    refusing) — otherwise it is refused — and then ccmp_joint_distance(w_i, c_i) > min_change — otherwise it is below
 *                    min_change.  The new path is w_0, m_0, w_1', m_1, .., m_{L-2}, w_{L-1}: 2L - 1 vertices, w_i' = c_i if accepted, else
 *                    w_i; u = the accepted vertices.
 *     loop           per path; stop [F] is the reason it ended, decided in this order: 4 a waypoint among the first L is not finite in all
 *                    14 coordinates (copied unchanged, nothing traversed); 0 L < 3 (copied); then, before every pass, 2 max_steps passes
 *                    have run, 3 the next pass would not fit (2L - 1 > out_max_len); after a pass 1 it moved nothing (u == 0; that pass's
 *                    subdivision is kept, as OMPL keeps it).  A path that has stopped takes no part in later passes: its result equals that
 *                    of the path run alone.
 *     result         out_joints [F][out_max_len][14] (rows behind out_len are untouched), out_len, passes, moved (the sum of u), stop [F]
 *                    int32; length_in, length_out [F] = the left-to-right fl sum of adjacent joint distances (a NaN row makes it NaN);
 *                    stats (nullable) [F][5] int32: midpoints projected, fallen back, degenerate, candidates refused (checkMotion or
 *                    clearance), candidates below min_change.
 * The result does not depend on launch shape, list length (chunk_states), round_budget or tile_edges.
 *   ccmp_path_smooth     device pointers.  SYNCHRONOUS on its stream and not capturable: it reads what the continuation loops of the dense
 *                    and shortcut sections read, path_len and F flags once, and F counts per pass.  opts == NULL: the defaults.  The
 *                    whole result is built in a workspace of the call and copied out only at the end: on any error (CCMP_EOVERFLOW when
 *                    max_calls extend calls are spent with a traversal still open among them) every output is untouched.
 *   _host            host pointers, on the context's stream.
 *   ccmp_smooth_mid_ref  the bracket and the blend of ONE pair, pure host code: rows [n][14] and arcs [n] of its closed list -> *k, *t, blend
 *                    [14] (before projection) and *fallback = the row a failed projection would take.  A degenerate list answers k = 0,
 *                    t = 0, blend = row 0, fallback = 0.  No projection, no device, never CCMP_ENODEV.  CCMP_EINVAL: n < 2, a NULL pointer.
 *   ccmp_smooth_len_after(L, passes)   the vertices of a path of L waypoints after that many passes (L < 3: L), saturating at INT32_MAX;
 *                    out_max_len = ccmp_smooth_len_after(max_len, max_steps) never stops a path on capacity.
 *   ccmp_smooth_last_counts   what the calling thread's last ccmp_path_smooth / _host did, for measurements (each pointer nullable): the
 *                    extend calls it made, the projector calls (one per midpoint step), and the bytes it read on the host (path_len and
 *                    the flags once, the continuation loops' 5 or 6 bytes per open traversal and extend call, F counts per pass).
 * Conventions as the dense and shortcut sections': every check runs before the first launch; a NULL context answers CCMP_ENODEV without a
 * device and CCMP_EINVAL with one; F == 0 returns CCMP_OK and touches nothing.  CCMP_EINVAL: max_steps < 0, a negative or NaN min_change
 * (+inf is allowed), max_len < 1, out_max_len < max_len, a path_len entry outside [0, max_len], chunk_states < 2, round_budget < 0,
 * max_calls < 1, tile_edges < 1, a scene of another device, a NaN margin with a scene, an output overlapping an input, a NULL path_joints,
 * path_len, out_joints, out_len, passes, moved, stop, length_in or length_out.  Order of use: shortcut -> smooth -> densify -> the host's
 * validity test over the dense rows. */
typedef struct ccmp_smooth_opts {
  int max_steps;     /* passes at most, >= 0 */
  double min_change; /* a vertex moves only by more than this */
  int chunk_states;  /* list entries per extend call, >= 2 */
  int round_budget;  /* Newton rounds per traversal and extend call, 0 = no bound */
  int max_calls;     /* extend calls at most, per midpoint step and per tile of the test step */
  int tile_edges;    /* checkMotion tests per tile, >= 1 */
} ccmp_smooth_opts;
/* 5, 0.005, 16, 128, 4096, 65536 */
void ccmp_smooth_opts_default(ccmp_smooth_opts *opts);
int ccmp_path_smooth(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const int32_t *path_len,
                     size_t F, int max_len, const ccmp_smooth_opts *opts, int out_max_len, double *out_joints, int32_t *out_len, int32_t *passes,
                     int32_t *moved, int32_t *stop, double *length_in, double *length_out, int32_t *stats, void *hip_stream);
int ccmp_path_smooth_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints,
                          const int32_t *path_len, size_t F, int max_len, const ccmp_smooth_opts *opts, int out_max_len, double *out_joints,
                          int32_t *out_len, int32_t *passes, int32_t *moved, int32_t *stop, double *length_in, double *length_out, int32_t *stats);
int ccmp_smooth_mid_ref(const double *rows, const double *arcs, int n, int *k, double *t, double *blend, int *fallback);
int ccmp_smooth_len_after(int L, int passes);
void ccmp_smooth_last_counts(long long *extend_calls, long long *project_calls, long long *bytes_read);

/* ---- executing a path: resample at even arc, then time stamps under joint limits --------------------------------------------------- */
/* The reference executes its path by giving every printed row the same time slice (scripts/execute_path.py:105-108, 2.5 s in all); dense
 * rows are not evenly spaced and nothing relates that time to what the joints can do.  Two steps close the gap; the rule of both is
 * csrc/ccmp_retime.h, stated once for the kernels, the host forms and the _ref forms, bit for bit against each other.
 *     resample       PathGeometric::interpolate(count) with this project's blend.  A dense path (either layout) has rows r_0 .. r_{R-1} and
 *                    arcs s, T = s_{R-1}.  status [F], tested in this order: CCMP_RETIME_EMPTY R == 0; _BROKEN a segment of the path has
 *                    seg_ok == 0 (the path has a jump); _NONFINITE a row is not finite in all 14 coordinates; _POINT not T > 0 (one row out:
 *                    r_0); _FULL N > max_rows; else _OK, N rows out.  N = count when count >= 2, else 1 + (int64)ceil(T / spacing) in IEEE
 *                    double (beyond INT32_MAX: _FULL).  Row 0 = r_0 and row N-1 = r_{R-1} (CCMP_SAMPLE_COPIED); for 0 < j < N-1:
 *                    h_j = fl(fl((double)j / (double)(N-1)) * T); not h_j > 0: r_0 (_DEGENERATE); else k = the smallest k >= 1 with
 *                    s_k >= h_j, t = (h_j - s_{k-1}) / (s_k - s_{k-1}), x = the extend step's interpolate(r_{k-1}, r_k, t), (y, ok) =
 *                    project(x) in the problem's Jacobian mode; ok: y (_PROJECTED); else r_{k-1} when (h_j - s_{k-1}) <= (s_k - h_j), else r_k
 *                    (_FALLBACK).  The result carries its own path_first [F + 1], arc [rows] and length [F] (the dense arc rule on the new
 *                    rows), kind [rows] (uint8), status [F] and counts [F][4] (int32, indexed by kind).  Resampled rows are NEW states: they
 *                    go to the host's validity test before use.
 *     time stamps    on any packed rows [total_rows][14] with path_first [F + 1]; the path parameter is the row index.  vmax[14], amax[14]
 *                    (HOST arrays in every form: checked before the first launch, handed to the kernels by value) finite and > 0;
 *                    0 < beta < 1 = the share of the acceleration budget given to curvature.  status [F]: _EMPTY, _NONFINITE, else _OK.
 *                    One row: t_0 = +0.0.  Otherwise d_i[c] = r_{i+1}[c] - r_i[c] (the plain difference, not interpolate's wrap),
 *                    V_i = min_c vmax_c / |d_i[c]|; ceilings on z = (index speed)^2: x_0 = x_{R-1} = +0.0, interior x_i = min(V_{i-1}^2,
 *                    V_i^2, min_c fl(beta amax_c) / |d_i[c] - d_{i-1}[c]|); A = min_{i,c} fl((1 - beta) amax_c) / |d_i[c]|, g = 2 A;
 *                    envelope y_i = min_k e(i, k), e(i, i) = x_i, e(i, k) = fl(x_k + fl(g |i - k|)); R >= 3: dt_i = 2 / (sqrt(y_i) +
 *                    sqrt(y_{i+1})); R == 2: dt_0 = 2 / sqrt(min(V_0^2, fl(0.5 g))); t_0 = +0.0, t_{i+1} = fl(t_i + dt_i); duration [F]
 *                    = t_{R-1} (+0.0 for _EMPTY, NaN for _NONFINITE, whose time / ceiling / envelope rows are not written).
 *                    By construction y_i <= x_i, 1 / dt_i <= V_i (the velocity limit on every interval) and |y_{i+1} - y_i| <= g up to
 *                    rounding: at the grid rows |q''| z <= beta amax and |q'| |z'| / 2 <= (1 - beta) amax.  That bounds the PROFILE; it is
 *                    NOT a bound on finite differences of the sampled trajectory.
 *   ccmp_path_resample   reads a dense result where it lies.  SYNCHRONOUS on its stream (it reads path_first, the F lengths, seg_first /
 *                    seg_ok and F status words to size the result): not capturable.  The blends of all paths go through the projector in
 *                    ONE ccmp_project_batch call.  opts == NULL: the defaults.  On any error no handle and no partial output.
 *   ccmp_resample_opts_default   count 0, spacing = the problem's delta (0 for a NULL problem), max_rows 65 536.
 *   ccmp_sampled_paths_info / _copy / _copy_host / _destroy   the result: F and the row count; copies into device (asynchronous on
 *                    hip_stream) or host (synchronous) destinations, each nullable: rows_out [rows][14], path_first [F + 1], arc [rows],
 *                    length [F], kind [rows], status [F], counts [F][4].
 *   ccmp_path_timestamps   device pointers (rows, path_first, time [total_rows], duration [F], status [F]; ceiling, envelope [total_rows]
 *                    nullable), asynchronous on hip_stream, no host read: capturable once the context's workspace holds the call (A per
 *                    path, and a ceiling / envelope array where the caller gave none: the first call at a size grows it — never capture
 *                    that one).  total_rows is what the caller sized `time` by.  path_first cannot be checked on the host here: a path
 *                    whose range is negative, decreasing or beyond total_rows is never read and answers _EMPTY.
 *   _host            host pointers, synchronous on the context's stream; rows of time / ceiling / envelope that the rule does not write
 *                    keep the caller's values.
 *   ccmp_path_timestamps_ref   the same rule text as pure host code, one thread, no device, never CCMP_ENODEV.
 *   ccmp_arc_bracket_ref   the bracket alone: arcs [n], n >= 2, 0 < h <= arcs[n-1] (else CCMP_EINVAL) -> *k, *t, *lower.
 *   ccmp_resample_targets_ref   the count and the targets alone: *N = the rows out (1 when not T > 0, 0 for _FULL), h_out [*N] (nullable) =
 *                    +0.0, the h_j, T.
 * Conventions as everywhere: every check runs before the first launch; a NULL context answers CCMP_ENODEV without a device and CCMP_EINVAL
 * with one; F == 0 gives an empty result / touches nothing.  CCMP_EINVAL: count == 1 or < 0, count 0 with spacing not > 0, max_rows < 2, a
 * limit that is not finite and positive, beta outside (0, 1), (host and _ref forms) a path_first that is negative, decreases or ends beyond
 * total_rows, a dense result of another device, a NULL dense, out, vmax, amax, path_first, duration or status, NULL rows or time with
 * total_rows > 0.  Order of use: shortcut -> smooth -> densify -> resample -> the host's validity test over the new rows -> time stamps. */
enum { CCMP_RETIME_OK = 0, CCMP_RETIME_EMPTY = 1, CCMP_RETIME_BROKEN = 2, CCMP_RETIME_NONFINITE = 3, CCMP_RETIME_POINT = 4, CCMP_RETIME_FULL = 5 };
enum { CCMP_SAMPLE_PROJECTED = 0, CCMP_SAMPLE_FALLBACK = 1, CCMP_SAMPLE_DEGENERATE = 2, CCMP_SAMPLE_COPIED = 3 };
typedef struct ccmp_resample_opts {
  int count;      /* rows out per path, >= 2; 0 = by spacing */
  double spacing; /* arc between rows when count == 0, > 0 */
  int max_rows;   /* a path that would get more rows is CCMP_RETIME_FULL, >= 2 */
} ccmp_resample_opts;
void ccmp_resample_opts_default(const ccmp_problem *p, ccmp_resample_opts *opts);
typedef struct ccmp_sampled_paths ccmp_sampled_paths;
int ccmp_path_resample(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_dense_paths *dense, const ccmp_resample_opts *opts, ccmp_sampled_paths **out,
                       void *hip_stream);
int ccmp_sampled_paths_info(const ccmp_sampled_paths *h, size_t *F, size_t *rows);
int ccmp_sampled_paths_copy(ccmp_sampled_paths *h, double *rows_out, int32_t *path_first, double *arc, double *length, uint8_t *kind, int32_t *status,
                            int32_t *counts, void *hip_stream);
int ccmp_sampled_paths_copy_host(ccmp_sampled_paths *h, double *rows_out, int32_t *path_first, double *arc, double *length, uint8_t *kind, int32_t *status,
                                 int32_t *counts);
void ccmp_sampled_paths_destroy(ccmp_sampled_paths *h);
int ccmp_path_timestamps(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax, const double *amax,
                         double beta, double *time, double *duration, double *ceiling, double *envelope, int32_t *status, void *hip_stream);
int ccmp_path_timestamps_host(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax,
                              const double *amax, double beta, double *time, double *duration, double *ceiling, double *envelope, int32_t *status);
int ccmp_path_timestamps_ref(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const double *vmax, const double *amax, double beta,
                             double *time, double *duration, double *ceiling, double *envelope, int32_t *status);
int ccmp_arc_bracket_ref(const double *arcs, int n, double h, int *k, double *t, int *lower);
int ccmp_resample_targets_ref(double T, int count, double spacing, int max_rows, int *N, double *h_out);

/* ---- executing a path: controller-rate setpoints and an execution audit ------------------------------------------------------------- */
/* Time stamps end at packed rows with one time per row; a robot is commanded at a fixed period (a Panda: 1 kHz).  ccmp_path_setpoints turns
 * (rows, stamps, period) into what is commanded at every controller tick and says what that motion does between the rows.  The rule is
 * csrc/ccmp_setpoints.h, stated once for the kernels and the _ref forms (no fused operation), bit for bit against each other.
 *     status         [F], tested in this order: CCMP_SETPOINTS_EMPTY R == 0 (device form: also a range that is negative, decreasing or
 *                    beyond total_rows, never read); _NONFINITE a row coordinate or a stamp is not finite; _UNORDERED t_0 != 0, some
 *                    t_{i+1} < t_i, or t_{i+1} == t_i while rows i and i + 1 differ; _POINT R == 1 or D = t_{R-1} not > 0 (one tick: q = r_0,
 *                    qd = 0, tau = +0.0); _FULL N > max_ticks or beyond INT32_MAX (no tick); else _OK, N ticks.
 *     ticks          N = 1 + (int64)ceil(D / period), at least 2; tau_0 = +0.0, tau_{N-1} = D, else tau_j = min(fl((double)j period), D).
 *     setpoints      q, qd [ticks][14], tau [ticks]: a C1 piecewise cubic through the rows at their stamps with PCHIP (Fritsch-Butland)
 *                    tangents, at rest at both ends: it cannot overshoot its rows.  Tangents, bracket and the operation order of q and qd:
 *                    csrc/ccmp_setpoints.h.  Setpoints are NOT projected, deliberately: a projection moves a point by up to the
 *                    projector's tolerance, differently from tick to tick — divided by dt^2 = 1e-6 that is acceleration noise of order
 *                    1e3 rad/s^2.  The knob for the gap is the resample spacing; the audit says whether it is fine enough.
 *     per tick       f [ticks][2] = ccmp_function_batch's (|dp|, angle) of q, satisfied [ticks] = ccmp_is_satisfied_batch's, clearance
 *                    [ticks] = ccmp_clearance_batch's with a scene, NaN without: those launchers, unchanged, once each over all ticks.
 *     audit          per path: peak [F][5] and peak_tick [F][5] in the order speed ratio max |qd| / vmax, acceleration ratio max (|qd_{j+1} -
 *                    qd_j| / (tau_{j+1} - tau_j)) / amax over intervals of positive width (at the left tick), max |dp|, max angle, min
 *                    clearance; ties go to the smallest tick, a NaN never contributes, a peak without contributor is +0.0 (clearance
 *                    +inf) at tick -1.  counts [F][2] = ticks isSatisfied refuses, ticks with clearance < margin.  stretch [F] = max(1,
 *                    speed ratio, sqrt(acceleration ratio)): the factor on all stamps that would scale the measured peaks to the limits
 *                    — a report; the stretched call has another tick grid and nothing is claimed for it.  The acceleration figure is
 *                    the mean acceleration over a tick interval of the interpolant's exact derivative, not a second difference of
 *                    positions.  The time stamps bound their profile at the rows; THIS is where the executed motion is measured.
 *   ccmp_path_setpoints   device pointers; vmax, amax HOST arrays.  SYNCHRONOUS on its stream (it reads F status words and F tick counts
 *                    to size the result): not capturable.  scene nullable.  opts == NULL: the defaults.  On any error no handle and no
 *                    partial output.
 *   ccmp_setpoint_opts_default   period 0.001, max_ticks 65 536.
 *   _host            host pointers (rows, path_first, time), synchronous on the context's stream.
 *   ccmp_setpoints_info / _copy / _copy_host / _destroy   the result: F and the tick count; copies into device (asynchronous on hip_stream)
 *                    or host (synchronous) destinations, each nullable: q, qd [ticks][14], tau [ticks], tick_first [F + 1], f [ticks][2],
 *                    satisfied [ticks] (uint8), clearance [ticks], status [F], peak [F][5], peak_tick [F][5] (int32), counts [F][2],
 *                    stretch [F].
 *   ccmp_setpoints_ref   the interpolation and the speed and acceleration audit as pure host code, one thread, no device, never
 *                    CCMP_ENODEV: tick_first [F + 1] and status [F] always; q, qd, tau, peak [F][2] (speed, acceleration), peak_tick [F][2],
 *                    stretch [F] where given (two-call sizing: NULL arrays first).  f and the clearance are other units' rules.
 *   ccmp_setpoint_tangents_ref   the tangents of ONE path alone: rows [R][14], time [R] -> w_out [R][14].
 * CCMP_EINVAL: a period that is not finite and > 0, max_ticks < 2, a limit that is not finite and positive, a NULL out, problem, vmax, amax,
 * path_first, tick_first or status, NULL rows or time with total_rows > 0, (host and _ref forms) a path_first that is negative, decreases
 * or ends beyond total_rows, a scene of another device or a NaN margin with one.  CCMP_EOVERFLOW: more than INT32_MAX ticks in all.
 * Order of use: shortcut -> smooth -> densify -> resample -> the host's validity test over the new rows -> time stamps -> fit (below) ->
 * setpoints and audit -> execute. */
enum { CCMP_SETPOINTS_OK = 0, CCMP_SETPOINTS_EMPTY = 1, CCMP_SETPOINTS_NONFINITE = 2, CCMP_SETPOINTS_UNORDERED = 3, CCMP_SETPOINTS_POINT = 4,
       CCMP_SETPOINTS_FULL = 5 };
typedef struct ccmp_setpoint_opts {
  double period; /* the controller's period, seconds, finite and > 0 */
  int max_ticks; /* a path that would get more ticks is CCMP_SETPOINTS_FULL, >= 2 */
} ccmp_setpoint_opts;
void ccmp_setpoint_opts_default(ccmp_setpoint_opts *opts);
typedef struct ccmp_setpoints ccmp_setpoints;
int ccmp_path_setpoints(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first,
                        const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax, const ccmp_setpoint_opts *opts,
                        ccmp_setpoints **out, void *hip_stream);
int ccmp_path_setpoints_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first,
                             const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax, const ccmp_setpoint_opts *opts,
                             ccmp_setpoints **out);
int ccmp_setpoints_info(const ccmp_setpoints *h, size_t *F, size_t *ticks);
int ccmp_setpoints_copy(ccmp_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied, double *clearance,
                        int32_t *status, double *peak, int32_t *peak_tick, int32_t *counts, double *stretch, void *hip_stream);
int ccmp_setpoints_copy_host(ccmp_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied, double *clearance,
                             int32_t *status, double *peak, int32_t *peak_tick, int32_t *counts, double *stretch);
void ccmp_setpoints_destroy(ccmp_setpoints *h);
int ccmp_setpoints_ref(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                       const ccmp_setpoint_opts *opts, int32_t *tick_first, int32_t *status, double *q, double *qd, double *tau, double *peak,
                       int32_t *peak_tick, double *stretch);
int ccmp_setpoint_tangents_ref(const double *rows, const double *time, size_t R, double *w_out);

/* ---- executing a path: time stamps fitted to the limits at the controller's rate ---------------------------------------------------- */
/* The time stamps bound their profile at the rows; the setpoints' audit measures what is commanded between them, and on the recorded paths
 * it measures up to 1.1 x vmax and 3.5 x amax at 1 ms.  ccmp_path_fit_timestamps is the step between the two: it measures the commanded
 * motion at the ticks of the stated period, dilates ONLY the row intervals in which it exceeds a limit, measures again and repeats until the
 * audit passes.  The rule is csrc/ccmp_fit.h, stated once for the kernels and the _ref form (no fused operation), bit for bit against each
 * other; status, ticks, tangents and qd are the setpoints rule's, unchanged.  Per path, with stamps t (the input's at pass 0), passes = 0:
 *     status         the setpoints status of (rows, t).  _EMPTY, _NONFINITE, _UNORDERED, _POINT and _FULL end the path with that value and the
 *                    stamps it was found on (at pass 0: the input's; a device range that is never read is never written); _FULL can arise
 *                    after a dilation.  peak then holds the last measurement made, +0.0 without one.
 *     measurement    over the ticks of the setpoints rule, never materialised: k_j the bracket of tau_j (k_0 = k_1), s_j = max_c |qd_j[c]| /
 *                    vmax_c, a_j = max_c (|qd_{j+1}[c] - qd_j[c]| / (tau_{j+1} - tau_j)) / amax_c over intervals of positive width; per row
 *                    interval k = 1 .. R-1: S_k = max{ s_j : k_j = k }, A_k = max{ a_j : k_j <= k <= k_{j+1} }, +0.0 for an empty set; a NaN
 *                    never contributes.  P_s = max_k S_k, P_a = max_k A_k: the speed and acceleration peaks ccmp_path_setpoints' audit
 *                    reports for the same stamps, bit for bit.
 *     done           P_s <= 1 and P_a <= 1: CCMP_FIT_FITTED (0), stamps untouched; else passes == max_passes: CCMP_FIT_PASSES, stamps as
 *                    measured.
 *     dilation       f_k = max(1, S_k / aim, sqrt(A_k / aim)), h'_k = (t_k - t_{k-1}) f_k, t'_0 = +0.0, t'_k = t'_{k-1} + h'_k left to right;
 *                    passes += 1; again.
 *   outputs          time_out [total_rows]; status [F]; passes [F] the dilations applied; peak [F][2] = (P_s, P_a) of the last measurement;
 *                    duration [F] the last stamp of time_out (+0.0 _EMPTY, NaN _NONFINITE); factor [total_rows], nullable: time_out's
 *                    interval over the input's at the interval's right row, 1.0 at row 0 and for intervals without positive input width.
 *                    f_k >= 1: stamps stay ordered, an interval without width keeps none, and no interval or duration shrinks by more than
 *                    the rounding of the stamps' sum (a factor can read one spacing of its stamp below 1); a path that is done is never
 *                    touched again, whatever its batch neighbours do; the result is a function of the inputs alone.
 *   what it is NOT   not TOPP-RA: no optimality, only the audit's figures; no jerk limit; a bound only at the ticks of the stated period (another
 *                    period is another grid); convergence is observed on the recorded inputs (profiles/fit.md), not proven — with aim = 1 the
 *                    peaks are observed to creep towards 1 from above without reaching it, hence aim < 1 and hence CCMP_FIT_PASSES is a status.
 *   ccmp_path_fit_timestamps   device pointers; vmax, amax HOST arrays.  SYNCHRONOUS on its stream: per pass one status launch, one read of F
 *                    status words and F tick counts (they size the measure launch and tell when no path is open), then tangent ->
 *                    measure -> dilate; nothing else is read on the host and no allocation is sized by the ticks.  time_out must not overlap
 *                    time.  opts == NULL: the defaults.
 *   ccmp_fit_opts_default   period 0.001, max_ticks 65 536, aim 0.95, max_passes 8.
 *   _host            host pointers throughout, synchronous on the context's stream.
 *   _ref             pure host code, one thread, no device, never CCMP_ENODEV.
 * CCMP_EINVAL: a period that is not finite and > 0, max_ticks < 2, aim outside (0, 1], max_passes < 0, a limit that is not finite and
 * positive, a NULL vmax, amax, path_first, status, passes, peak or duration with F > 0, NULL rows, time or time_out with total_rows > 0, a
 * time_out that overlaps time, (host and _ref forms) a path_first that is negative, decreases or ends beyond total_rows.  CCMP_EOVERFLOW: more
 * than INT32_MAX tick intervals in one pass.
 * Order of use: ... -> time stamps -> fit -> setpoints and audit -> execute. */
enum { CCMP_FIT_FITTED = 0, CCMP_FIT_PASSES = 6 }; /* 1 .. 5: CCMP_SETPOINTS_EMPTY .. CCMP_SETPOINTS_FULL */
typedef struct ccmp_fit_opts {
  double period;  /* the controller's period, seconds, finite and > 0 */
  int max_ticks;  /* a path that would get more ticks is CCMP_SETPOINTS_FULL, >= 2 */
  double aim;     /* the share of a limit an interval in excess is dilated to, 0 < aim <= 1 */
  int max_passes; /* dilations per path at most, >= 0 */
} ccmp_fit_opts;
void ccmp_fit_opts_default(ccmp_fit_opts *opts);
int ccmp_path_fit_timestamps(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows,
                             const double *vmax, const double *amax, const ccmp_fit_opts *opts, double *time_out, int32_t *status, int32_t *passes,
                             double *peak, double *duration, double *factor, void *hip_stream);
int ccmp_path_fit_timestamps_host(ccmp_ctx *ctx, const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows,
                                  const double *vmax, const double *amax, const ccmp_fit_opts *opts, double *time_out, int32_t *status, int32_t *passes,
                                  double *peak, double *duration, double *factor);
int ccmp_path_fit_timestamps_ref(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax,
                                 const double *amax, const ccmp_fit_opts *opts, double *time_out, int32_t *status, int32_t *passes, double *peak,
                                 double *duration, double *factor);

/* ---- executing a path: jerk-bounded setpoints ----------------------------------------------------------------------------------------- */
/* ccmp_path_setpoints commands a C1 piecewise cubic: its acceleration jumps at every row, and a robot that limits jerk (a Panda: 7500 ..
 * 10000 rad/s^3 and a 1 kHz interface that refuses a discontinuous acceleration) refuses it however the stamps were fitted.
 * ccmp_path_jerk_setpoints delivers the setpoints of a moving average of W consecutive ticks of that interpolant, measures jerk, and
 * chooses W per path.  The rule is csrc/ccmp_jerk.h, stated once for the kernels and the _ref form (no fused operation), bit for bit
 * against each other; status, tangents, q, qd and the bracket are the setpoints rule's, unchanged.
 *     status         [F]: CCMP_JERK_EMPTY, _NONFINITE, _UNORDERED, _POINT as the setpoints rule tests them (a _POINT path: one tick, q = r_0,
 *                    qd = +0.0, tau = +0.0, window 0); _FULL the ticks of the window do not fit max_ticks (no tick); _WINDOW the jerk peak of
 *                    the delivered window is still above 1; else _OK.
 *     input          n = (int64)ceil(D / period), D the last stamp.  x_i = (r_0, 0) for i <= 0, (r_{R-1}, 0) for i >= n, else (q, qd) of the
 *                    setpoints rule's interior tick at min(fl(i period), D): the arrival sits on the grid at n period, not at D.
 *     output for W   M = n + W ticks, tau_j = fl(j period); ticks 0 and M - 1 are copies of r_0 and r_{R-1} with qd = +0.0; else q_j[c] =
 *                    (x_{j-W+1}[c] + ... + x_j[c]) / W summed from the oldest term to the newest, then one division, and qd_j[c] the same
 *                    over the qd parts.
 *     per tick       f, satisfied, clearance: ccmp_function_batch's, ccmp_is_satisfied_batch's and (with a scene) ccmp_clearance_batch's
 *                    of the FILTERED q, those launchers unchanged, once each over all ticks.
 *     audit          peak [F][6] and peak_tick [F][6] in the order speed, acceleration, jerk, |dp|, angle, clearance, under the setpoints
 *                    audit's order (ties to the smallest tick, a NaN never contributes, none: +0.0 — clearance +inf — at tick -1).  Jerk:
 *                    a_j[c] = (qd_{j+1}[c] - qd_j[c]) / (tau_{j+1} - tau_j), signed; jerk_j[c] = (|a_{j+1}[c] - a_j[c]| / (0.5 (tau_{j+2} - tau_j))) /
 *                    jmax_c for 0 <= j <= M - 3, at the middle tick j + 1.  counts [F][2] as in the setpoints unit.
 *     the window     opts.window > 0: that W for every path, one measurement, passes = 0, _OK or _WINDOW by jerk peak <= 1.  0: per path
 *                    W = 1; measure the jerk peak P; P <= 1: _OK; else W == max_window: _WINDOW (ticks and audit of max_window are
 *                    delivered); else W <- min(max_window, max(W + 1, (int)ceil(W P / aim))), passes += 1, again.  A W whose ticks do
 *                    not fit ends the path _FULL; window and passes then name that W.
 *   by construction  a mean cannot exceed the largest of its terms: the speed and acceleration peaks do not rise above those of W = 1 and
 *                    q stays in the hull of its window's inputs (both up to the rounding of W - 1 additions and a division); the jerk of
 *                    joint c is at most 2 A_c / (W period), A_c its acceleration peak at W = 1 in rad/s^2, so every W >= W* = ceil(max_c 2 A_c /
 *                    (period jmax_c)) passes and the search ends _OK whenever W* <= max_window, within max_window passes.  The motion
 *                    grows by W - 1 ticks.
 *   what it is NOT   a bound at the ticks of the stated period on the qd sequence, as the setpoints audit is, not a third difference of
 *                    positions (two rows with D <= period: n = 1, every qd zero, whatever the rows).  The filtered ticks no longer pass
 *                    through the rows: they lag by (W - 1) / 2 ticks and cut corners by the order of a (W period)^2 / 24; f, satisfied and
 *                    clearance of this call tell whether that matters.  Not a jerk-optimal profile.
 *   ccmp_path_jerk_setpoints   device pointers; vmax, amax, jmax HOST arrays.  SYNCHRONOUS on its stream (per pass of the search it reads F
 *                    words that size the next launch and tell when no path is open): not capturable.  scene nullable.  opts == NULL: the
 *                    defaults.  On any error no handle and no partial output.
 *   ccmp_jerk_opts_default   period 0.001, max_ticks 65 536, window 0, max_window 64, aim 0.95, tile_ticks 0.
 *   _host            host pointers (rows, path_first, time), synchronous on the context's stream.
 *   ccmp_jerk_setpoints_info / _copy / _copy_host / _destroy   the result: F and the tick count; copies into device (asynchronous on
 *                    hip_stream) or host (synchronous) destinations, each nullable: q, qd [ticks][14], tau [ticks], tick_first [F + 1],
 *                    f [ticks][2], satisfied [ticks] (uint8), clearance [ticks], status [F], window [F], passes [F], peak [F][6],
 *                    peak_tick [F][6] (int32), counts [F][2].
 *   ccmp_jerk_setpoints_ref   the rule and the speed, acceleration and jerk audit as pure host code, one thread, no device, never
 *                    CCMP_ENODEV: tick_first [F + 1], status [F], window [F], passes [F] always; q, qd, tau, peak [F][3], peak_tick [F][3]
 *                    where given (two-call sizing: NULL arrays first).
 *   ccmp_jerk_next_window_ref   the search's update alone: *next = min(max_window, max(W + 1, (int)ceil(W P / aim))) for 1 <= W < max_window
 *                    <= 256, any P that is no NaN, 0 < aim <= 1 (else CCMP_EINVAL).  Inside the search P > 1 and aim <= 1 make the
 *                    ceiling at least W + 1 by themselves; the W + 1 term is what makes the growth unconditional.
 * CCMP_EINVAL: what ccmp_path_setpoints refuses; a jmax that is NULL or not finite and positive; window outside 0 .. max_window; max_window
 * outside 1 .. 256; aim outside (0, 1]; a negative tile_ticks; a NULL window or passes (_ref form).  CCMP_EOVERFLOW: more than INT32_MAX ticks
 * in all.  Order of use: ... -> time stamps -> fit -> jerk-bounded setpoints and audit -> execute. */
enum { CCMP_JERK_OK = 0, CCMP_JERK_EMPTY = 1, CCMP_JERK_NONFINITE = 2, CCMP_JERK_UNORDERED = 3, CCMP_JERK_POINT = 4, CCMP_JERK_FULL = 5,
       CCMP_JERK_WINDOW = 6 }; /* 0 .. 5: the values of CCMP_SETPOINTS_* */
typedef struct ccmp_jerk_opts {
  double period;  /* the controller's period, seconds, finite and > 0 */
  int max_ticks;  /* a path whose window would give more ticks is CCMP_JERK_FULL, >= 2 */
  int window;     /* 0: chosen per path; else 1 .. max_window, the same for every path */
  int max_window; /* the largest window the search tries, 1 .. 256 */
  double aim;     /* the share of jmax the next window of the search aims at, 0 < aim <= 1 */
  int tile_ticks; /* output ticks per block of the search's measure launch; 0 or beyond the default (128): the default.  The result
                     does not depend on it */
} ccmp_jerk_opts;
void ccmp_jerk_opts_default(ccmp_jerk_opts *opts);
typedef struct ccmp_jerk_setpoints ccmp_jerk_setpoints;
int ccmp_path_jerk_setpoints(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows, const int32_t *path_first,
                             const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax, const double *jmax,
                             const ccmp_jerk_opts *opts, ccmp_jerk_setpoints **out, void *hip_stream);
int ccmp_path_jerk_setpoints_host(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *rows,
                                  const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax, const double *amax,
                                  const double *jmax, const ccmp_jerk_opts *opts, ccmp_jerk_setpoints **out);
int ccmp_jerk_setpoints_info(const ccmp_jerk_setpoints *h, size_t *F, size_t *ticks);
int ccmp_jerk_setpoints_copy(ccmp_jerk_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied,
                             double *clearance, int32_t *status, int32_t *window, int32_t *passes, double *peak, int32_t *peak_tick, int32_t *counts,
                             void *hip_stream);
int ccmp_jerk_setpoints_copy_host(ccmp_jerk_setpoints *h, double *q, double *qd, double *tau, int32_t *tick_first, double *f, uint8_t *satisfied,
                                  double *clearance, int32_t *status, int32_t *window, int32_t *passes, double *peak, int32_t *peak_tick,
                                  int32_t *counts);
void ccmp_jerk_setpoints_destroy(ccmp_jerk_setpoints *h);
int ccmp_jerk_setpoints_ref(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const double *vmax,
                            const double *amax, const double *jmax, const ccmp_jerk_opts *opts, int32_t *tick_first, int32_t *status, int32_t *window,
                            int32_t *passes, double *q, double *qd, double *tau, double *peak, int32_t *peak_tick);
int ccmp_jerk_next_window_ref(int W, double P, double aim, int max_window, int *next);

/* ---- the planner's loop on the store: stefanBiPRM::solve as one resumable object ------------------------------------------------------- */
/* stefanBiPRM::solve / constructRoadmap / checkForSolution (stefanBiPRM.cpp:692-899) and the start and goal set-up of
 * ConstrainedPlanningCommon.cpp:147-207 over the calls above: a ccmp_plan takes (the problem's start state, its goal object pose) and
 * grows the store until a start vertex and a goal vertex share a component.  The reference runs constructRoadmap and checkForSolution
 * as two racing threads; this unit states their STRUCTURE as one deterministic sequence, not their interleaving: the result is a
 * function of the arguments and rng_seed alone.  csrc/ccmp_plan.h states the rule once, for the kernels of ccmp_kernels_plan.hip and
 * for the *_ref forms.  The planner's state (ccmp_plan_state) lives on the device; a cycle costs the host one read of it, the commits'
 * own read-backs, and one 16-byte read in a cycle whose check ran.
 *   open (ccmp_plan_create)   the start vertex (p->start_joint, the pose of p->obj_start_*) goes through startgoalMilestone:
 *       ccmp_roadmap_connect on the object metric with check_target = 1 (k neighbours, checkMotion from each), then ccmp_roadmap_commit
 *       with CCMP_COMMIT_KEEP_ISOLATED (no states: no mid-stones, no slot unsettled by its length).  The goal vertex is goal_joints[14]
 *       or, when that is NULL, ccmp_pose_ik_* (the vetted form when a scene is given) towards the pose of p->obj_goal_* seeded from the
 *       start state (one seed slot, draw index next_index); no solution: status CCMP_PLAN_INVALID_GOAL and nothing more is appended.  It
 *       goes through startgoalMilestone too, with the goal pose as its pose row.  next_index = first_index + 1 afterwards, in both cases.
 *       prev_from_goal = prev_from_start = ccmp_pose_distance(start pose, goal pose); nearest = starts[0], nearest_pose = the start
 *       pose; sprevious = goals[0]; size_at_check = the size after open; then the solution test.
 *   one cycle (ccmp_plan_run runs up to max_cycles of them)
 *     0. FULL       size + width (1 + k) + 11 > max_vertices: status CCMP_PLAN_FULL, nothing runs.
 *     1. growth     ccmp_object_propose_batch from nearest_pose (width rows) towards the goal pose with t, sigma, lo, hi, attempts,
 *                   inflate, draw indices next_index .. next_index + width - 1; ccmp_roadmap_grow (the vetted form with a scene) on ALL
 *                   width rows (a row without a valid candidate is NaN: a target without a state) with k, check_target 0, max_states,
 *                   the same first_index; ccmp_roadmap_commit with vertex_ok = ik_ok, the states, the goal pose and roots = starts.
 *                   next_index += width.  A query that is UNSETTLED is not continued: it is left out and counted.
 *     2. check      only if size > size_at_check + 3 (strict).  With (c, d) = closestFromGoal(starts, goals[0]) and (s, d2) =
 *                   closestFromGoal(goals, starts[0]) — both from ccmp_roadmap_closest on the store as the growth left it, folded by the
 *                   carry rule: val = +inf; per from f in order: val = min(val, from_dist) (strict <), closest = f, and if idx >= 0 and
 *                   dist < val (strict) then (closest, val) = (idx, dist) —
 *                     goal side    d < prev_from_goal - 0.1 (strict; a NaN never passes): nearest = c, nearest_pose = pose[c],
 *                                  prev_from_goal = d; the goal IK target is the goal pose seeded from joints[c] (with n_goals == 8 it is not
 *                                  tried and push_refused counts it); the ladder targets are ccmp_pose_interpolate(pose[c], goal, 0.1 i), i =
 *                                  1 .. 9, seeded from joints[c].
 *                     start side   sprevious = s; d2 < prev_from_start - 0.1: prev_from_start = d2; the start IK target is the start pose
 *                                  seeded from joints[s] (n_starts == 8: not tried, counted).
 *                   size_at_check = size; next_index += 11 (the eleven IK targets take indices next_index .. + 10 in the order goal,
 *                   ladder 1 .. 9, start, whether or not their branch fired).  Then ccmp_object_valid_batch on the ladder, ONE IK call over
 *                   the eleven targets (one seed slot each), the ladder's PREFIX = the longest run from i = 1 in which every pose is valid
 *                   and solved, and in this order: the goal vertex through startgoalMilestone and onto goals; the prefix through addMilestone
 *                   (ccmp_roadmap_connect with check_target 1, commit without KEEP_ISOLATED) as ONE batch; the start vertex through
 *                   startgoalMilestone and onto starts.  With n_goals == 0 neither side fires.
 *     3. cycle += 1, then the solution test: the first pair (s, g), start-major and goal-minor, with label[starts[s]] == label[goals[g]]
 *                   gives status CCMP_PLAN_SOLVED and the pair (the reference's cost threshold is infinite: the first connected pair is
 *                   the answer).  The path itself is ccmp_roadmap_shortest_paths' on that pair.
 *   TWO STATED DIFFERENCES from the reference: a cycle grows width candidates that do not see each other and adds the ladder's prefix as
 *   one batch (the reference adds one candidate per cycle and the nine ladder poses one after the other); and an UNSETTLED query is
 *   skipped, not continued.  With width == 1 a growth step is the reference's growTree.
 * ccmp_plan_create runs open; it remembers the store, the object and the scene, which must outlive it (their life-cycle rules are the
 * handle's).  ccmp_plan_run is synchronous and not capturable; it waits for the device at entry, so appends made on any stream before it
 * are seen.  After CCMP_PLAN_SOLVED or CCMP_PLAN_INVALID_GOAL a run returns at once with the same report.  On an error the store is as the
 * last completed call inside the cycle left it.  Every check comes before the first launch; a NULL store / handle answers CCMP_ENODEV on
 * a machine without a HIP device and CCMP_EINVAL otherwise.  CCMP_EINVAL: width outside 1 .. CCMP_PLAN_MAX_WIDTH, k outside 1 ..
 * CCMP_IK_MAX_SEEDS, attempts or max_states out of ccmp_object_propose_batch's / ccmp_roadmap_grow's range, a non-finite option (t, sigma,
 * inflate, lo, hi) or a NaN margin, max_vertices below the store's size + 2 at open, an object or a scene of another device
 * than the store's, a NULL problem, object, opts or out, an invalid problem or IK options.
 * The *_ref forms are the rule's pure parts on host memory: no device, never CCMP_ENODEV.
 *   ccmp_plan_check_ref      step 2's decisions: state in and out; size; the closest arrays of both sides (a_* [n_starts], b_* [n_goals]);
 *                            store_poses [size][8] (nullable: nearest_pose is then left alone); triggers[4] = {the check ran, the goal side
 *                            fired, the start side fired, the vertex c whose joints seed the goal side or -1}.
 *   ccmp_plan_prefix_ref     valid[9], ik_ok[9] -> vertex_ok[9] (1 on the prefix), returns nothing else; *prefix_len its length.
 *   ccmp_plan_connected_ref  labels [N], state -> state (status, solved pair); an index outside [0, N) never matches. */
#define CCMP_PLAN_MAX_STARTS 8
#define CCMP_PLAN_MAX_GOALS 8
#define CCMP_PLAN_MAX_WIDTH 256
#define CCMP_PLAN_LADDER 9
enum { CCMP_PLAN_OPEN = 0, CCMP_PLAN_SOLVED = 1, CCMP_PLAN_BUDGET = 2, CCMP_PLAN_FULL = 3, CCMP_PLAN_INVALID_GOAL = 4 };
typedef struct ccmp_plan_opts {
  int32_t width;         /* 32     candidates per growth step */
  int32_t k;             /* 5      DEFAULT_NEAREST_NEIGHBORS */
  int32_t attempts;      /* 2      draws per candidate (stefanBiPRM.cpp:262) */
  int32_t max_states;    /* 64     the traversals' list length */
  double t;              /* 0.3    the interpolation towards the goal pose */
  double sigma;          /* 0.2    the draw's standard deviation */
  double inflate;        /* 0      the mesh test's box inflation */
  double lo[3], hi[3];   /* -1e30, 1e30: the draw's position bounds */
  uint64_t max_vertices; /* 2^31 - 1 */
} ccmp_plan_opts;
typedef struct ccmp_plan_counters {
  int32_t proposals, valid_proposals, ik_successes, vertices_kept, mid_stones, unsettled, checks, goal_pushes, start_pushes, ladder_vertices,
      push_refused, reserved;
} ccmp_plan_counters;
typedef struct ccmp_plan_state {
  int32_t n_starts, n_goals;
  int32_t starts[CCMP_PLAN_MAX_STARTS], goals[CCMP_PLAN_MAX_GOALS];
  int32_t nearest, sprevious;
  int32_t status, cycle;
  int32_t solved_start, solved_goal; /* vertices; -1 until SOLVED */
  int32_t size_at_check, reserved;
  uint64_t next_index;
  double nearest_pose[8];
  double prev_from_goal, prev_from_start;
  ccmp_plan_counters counters;
} ccmp_plan_state;
typedef struct ccmp_plan_report {
  int32_t status, cycles_run, cycles_total, reserved;
  uint64_t size, edges;
  int32_t solved_start, solved_goal, nearest, reserved2;
  double prev_from_goal, prev_from_start;
  ccmp_plan_counters counters;
} ccmp_plan_report;
typedef struct ccmp_plan ccmp_plan;
void ccmp_plan_default_opts(ccmp_plan_opts *opts);
int ccmp_plan_create(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_object *object, const ccmp_scene *scene, double margin,
                     const ccmp_ik_opts *ik_opts, const ccmp_plan_opts *opts, const double *goal_joints, uint64_t rng_seed, uint64_t first_index,
                     ccmp_plan **out);
int ccmp_plan_run(ccmp_plan *plan, int max_cycles, ccmp_plan_report *out);
int ccmp_plan_state_read(ccmp_plan *plan, ccmp_plan_state *out);
void ccmp_plan_destroy(ccmp_plan *plan);
int ccmp_plan_check_ref(ccmp_plan_state *state, size_t size, const int32_t *a_idx, const double *a_dist, const double *a_from, const int32_t *b_idx,
                        const double *b_dist, const double *b_from, const double *store_poses, int32_t triggers[4]);
int ccmp_plan_prefix_ref(const uint8_t valid[9], const uint8_t ik_ok[9], uint8_t vertex_ok[9], int32_t *prefix_len);
int ccmp_plan_connected_ref(const int32_t *labels, size_t N, ccmp_plan_state *state);

/* ---- RRT-Connect on the store: the reference's other planner ------------------------------------------------------------------------------ */
/* The reference offers RRT, RRTConnect and StefanBiPRM behind ConstrainedProblem::setPlanner (ConstrainedPlanningCommon.h:141-157, the
 * commented switch at src/main.cpp:46-47); ccmp_plan_* above is the third, this is the second: two trees in JOINT space, grown from
 * nothing but the constraint, the projected sampler and a validity test — no object checker, no IK.  A ccmp_rrtc is a resumable
 * sibling of ccmp_plan on a roadmap store; csrc/ccmp_rrtc.h states its rule once, for the kernels of ccmp_kernels_rrtc.hip and for the
 * *_ref forms.  The caller has appended up to CCMP_PLAN_MAX_STARTS start vertices and CCMP_PLAN_MAX_GOALS goal vertices and hands over
 * their indices (host arrays).  A side's TREE is every vertex v whose label[v] equals the label of one of that side's roots: no
 * per-vertex array is kept, vertices of other components are ignored, pose-only vertices (NaN joints) are never a nearest neighbour.
 *   nearest_in_tree   for each of queries [Q][14]: the vertex with the smallest (ccmp_joint_distance(joints[v], query), v) among the
 *       vertices of the tree of roots [n_roots], 0 <= n_roots <= 8 — the arithmetic of ccmp_knn_batch (the FMA chain, then the correctly
 *       rounded square root), so with every vertex in the tree the answer is ccmp_roadmap_knn's with CCMP_METRIC_JOINT and k = 1.  A NaN
 *       distance is never a candidate; no candidate: idx -1, dist +inf.  roots is a device pointer in the device form; a root outside
 *       [0, size) is CCMP_EINVAL from the _host and _ref forms and contributes no label in the device form.  Asynchronous and capturable
 *       (after one eager call at that size: the partitions' bests go through the context's k-NN workspace).  The result is a function of
 *       the arguments alone: (distance, index) is a total order and the reduction compares pairs, so the launch shape
 *       (csrc/ccmp_policy.cpp: plan_rrtc_nearest, from Q, N and the CU count; no option) never changes it.  ccmp_rrtc_nearest_shape
 *       reports that shape (ctx NULL: a 256-CU device), for tests and tools.
 *   one cycle (ccmp_rrtc_run runs up to max_cycles of them)
 *     0. FULL      size + 2 width > max_vertices: status CCMP_RRTC_FULL, nothing runs.
 *     1. samples   width rows of ccmp_sample_project_batch at draw indices next_index .. next_index + width - 1; next_index += width.  A
 *                  row whose projection failed or which is not jointValid (ccmp_joint_valid_batch) is no sample and is counted
 *                  (samples - projected); with a scene neither is a row whose clearance (ccmp_clearance_batch) is not above the margin.
 *     2. extend    tree A = the start side in even cycles, the goal side in odd ones.  n = nearest_in_tree(A, sample), d its distance;
 *                  ONE traversal n -> sample through ccmp_geodesic_scene_batch (with a scene) or ccmp_geodesic_batch_ex, with max_states,
 *                  round_budget and check_target = 0.  With m = min(n_states, max_states) listed states, s_0 = 0, s_j = fl(s_{j-1} +
 *                  ccmp_joint_distance(state_{j-1}, state_j)) and cut = (n_states > max_states or ok == 2), the pick decides (rrtc_extend of
 *                  csrc/ccmp_rrtc.h; on its own: ccmp_rrtc_pick_ref / ccmp_rrtc_pick_batch):
 *                    d <= range   ok == 1: REACHED, the new vertex is the sample row itself; else cut: UNSETTLED; else TRAPPED.
 *                    d > range    m < 2: TRAPPED.  Else j = the largest listed index with s_j <= range, but at least 1.  cut, j == m - 1
 *                                 and s_j <= range: UNSETTLED (the arc was not used up inside the list).  Otherwise ADVANCED, the new
 *                                 vertex is listed state j.
 *                    a NaN in d, in range or in any s_j, or no nearest vertex: TRAPPED.
 *                  An UNSETTLED sample is skipped and counted, as ccmp_plan does.
 *     3. connect   for every vertex v that step 2 produced: u = nearest_in_tree(B, v) with B the OTHER side as of cycle entry, ONE traversal
 *                  u -> v with the same list length: ok == 1: the edge (u, v), the trees are joined (JOINED); else with two or more
 *                  listed states the last stored state becomes a vertex of B with the edge (u, that state) (ADDED: a cut list and a
 *                  blocked list count here too — every listed state passed the validity test, so this is valid progress); else NOTHING.
 *                  gap = ccmp_joint_distance(last stored state, v); the smallest gap seen so far (strict <, samples in ascending order)
 *                  is kept as best_gap with its pair (best_a on the start side, best_b on the goal side): the approximate solution's pair.
 *     4. commit    new indices in a total order: step 2's vertices in ascending sample order, then step 3's in ascending sample order;
 *                  the edges likewise, each (tree vertex, new vertex).  The rows go through ccmp_roadmap_append, the fixed-size uv array
 *                  (an entry of a sample without an edge is (-1, -1)) through ccmp_roadmap_add_edges: weights and labels are that call's.
 *     5. cycle += 1, then the solution test: the first pair (s, g), start-major and goal-minor, whose labels agree gives
 *                  CCMP_RRTC_SOLVED and the pair.  The path is ccmp_roadmap_shortest_paths' on that pair.
 *   The samples of a cycle do not see each other; with width == 1 a cycle is one iteration of the sequential algorithm.
 *
 *   STATED DIFFERENCES FROM OMPL'S RRTConnect
 *   (a) One traversal per extension, clipped at range.  OMPL runs interpolate(n, sample, range / d) and then a fresh checkMotion(n,
 *       dstate); its constrained interpolate returns the listed state NEARER to the fraction of the achieved length.  Here one traversal
 *       is clipped at an absolute arc, with at least one step of progress.  With the reference's own values, range 0.1
 *       (ConstrainedPlanningCommon.cpp:124) and delta 0.25 (:118), the nearer-state rule returns `from` itself whenever the first listed
 *       step is longer than 2 range, and OMPL then answers TRAPPED (DESIGN.md §5.22 records the share).
 *   (b) The connect phase is one traversal and adds its end state; OMPL adds a chain of range-spaced vertices.
 *   (c) UNSETTLED is skipped, not continued.
 *   (d) Both trees extend from the tree vertex towards the target; OMPL checks the goal tree's motion in the other direction.
 *   (e) The random numbers are the library's counter-based draws, not OMPL's RNG.
 *   (f) Validity is the proxy scene's, not MoveIt's; isValid over the dense rows of a solution stays a host call.
 *   What follows from (a) and (d): an edge (parent, child) was validated as a PREFIX of a traversal towards something else.
 *   ccmp_path_densify runs a fresh traversal parent -> child, and child -> parent where the path uses the edge reversed; that traversal
 *   is expected to arrive, it is not guaranteed to (its seg_ok says).
 *
 * ccmp_rrtc_create checks, uploads the state and runs the solution test once (roots that already share a component: SOLVED, cycle 0);
 * it remembers the store and the scene, which must outlive it.  ccmp_rrtc_run is synchronous and not capturable; it waits for the device
 * at entry.  Per cycle the host reads 16 bytes of counts after the commit kernel and the state block at the end, besides the read-back
 * of ccmp_roadmap_add_edges.  After CCMP_RRTC_SOLVED a run returns at once with the same report.  Every check comes before the first
 * launch; a NULL store / handle answers CCMP_ENODEV on a machine without a HIP device and CCMP_EINVAL otherwise.  CCMP_EINVAL: a root
 * outside [0, size), n_starts or n_goals of 0 or above the caps, width outside 1 .. CCMP_PLAN_MAX_WIDTH, a non-finite or non-positive
 * range, a NaN margin, max_states < 2, round_budget < 0, max_vertices beyond 2^31 - 1, a scene of another device than the store's, a NULL
 * or invalid problem, NULL opts, starts, goals or out.
 * The *_ref forms are the rule on host memory: no device, never CCMP_ENODEV.
 *   ccmp_rrtc_pick_ref        mode 0 (extend) / 1 (connect) on E lists: states [E][max_states][14], n_states [E], ok [E], use [E]
 *                             (nullable; 0: no sample / no vertex -> outcome CCMP_RRTC_NONE, 2: no nearest vertex -> TRAPPED / NOTHING),
 *                             to [E][14] (the sample / v), d [E] (mode 0: the nearest distance) -> outcome [E], row_index [E] (the listed
 *                             state that becomes the vertex, -1: the target row or none), row [E][14] (zeros without a vertex), gap [E]
 *                             (nullable; mode 1, NaN without a listed state).
 *   ccmp_rrtc_connected_ref   labels [N], state -> state (status, solved pair); an index outside [0, N) never matches. */
enum { CCMP_RRTC_OPEN = 0, CCMP_RRTC_SOLVED = 1, CCMP_RRTC_BUDGET = 2, CCMP_RRTC_FULL = 3 };
enum { CCMP_RRTC_NONE = -1, CCMP_RRTC_TRAPPED = 0, CCMP_RRTC_ADVANCED = 1, CCMP_RRTC_REACHED = 2, CCMP_RRTC_UNSETTLED = 3 };
enum { CCMP_RRTC_CONNECT_NOTHING = 0, CCMP_RRTC_CONNECT_ADDED = 1, CCMP_RRTC_CONNECT_JOINED = 2 };
#define CCMP_RRTC_MAX_ROOTS 8
typedef struct ccmp_rrtc_opts {
  int32_t width;         /* 32     samples per cycle */
  int32_t max_states;    /* 64     the traversals' list length */
  int32_t round_budget;  /* 0      the traversals' Newton-round bound (0: none) */
  int32_t reserved;
  double range;          /* 0.1    the reference's (ConstrainedPlanningCommon.cpp:124) */
  uint64_t max_vertices; /* 2^31 - 1 */
} ccmp_rrtc_opts;
typedef struct ccmp_rrtc_counters {
  int32_t samples, projected, trapped, advanced, reached, unsettled, connect_reached, connect_added, connect_nothing, vertices, edges, reserved;
} ccmp_rrtc_counters;
typedef struct ccmp_rrtc_state {
  int32_t n_starts, n_goals;
  int32_t starts[CCMP_PLAN_MAX_STARTS], goals[CCMP_PLAN_MAX_GOALS];
  int32_t status, cycle;
  uint64_t next_index;
  int32_t solved_start, solved_goal; /* vertices; -1 until SOLVED */
  int32_t best_a, best_b;            /* the pair of best_gap: a start-side and a goal-side vertex; -1 until a connect traversal ran */
  double best_gap;                   /* +inf until then */
  ccmp_rrtc_counters counters;
} ccmp_rrtc_state;
typedef struct ccmp_rrtc_report {
  int32_t status, cycles_run, cycles_total, reserved;
  uint64_t size, edges;
  int32_t solved_start, solved_goal, best_a, best_b;
  double best_gap;
  ccmp_rrtc_counters counters;
} ccmp_rrtc_report;
typedef struct ccmp_rrtc ccmp_rrtc;
void ccmp_rrtc_default_opts(ccmp_rrtc_opts *opts);
int ccmp_rrtc_create(ccmp_roadmap *rm, const ccmp_problem *p, const ccmp_scene *scene, double margin, const ccmp_rrtc_opts *opts, const int32_t *starts,
                     int n_starts, const int32_t *goals, int n_goals, uint64_t rng_seed, uint64_t first_index, ccmp_rrtc **out);
int ccmp_rrtc_run(ccmp_rrtc *plan, int max_cycles, ccmp_rrtc_report *out);
int ccmp_rrtc_state_read(ccmp_rrtc *plan, ccmp_rrtc_state *out);
void ccmp_rrtc_destroy(ccmp_rrtc *plan);
int ccmp_roadmap_nearest_in_tree(ccmp_roadmap *rm, const int32_t *roots, int n_roots, const double *queries, size_t Q, int32_t *idx, double *dist,
                                 void *hip_stream);
int ccmp_roadmap_nearest_in_tree_host(ccmp_roadmap *rm, const int32_t *roots, int n_roots, const double *queries, size_t Q, int32_t *idx, double *dist);
int ccmp_roadmap_nearest_in_tree_ref(const double *store_joints, const int32_t *labels, size_t N, const int32_t *roots, int n_roots, const double *queries,
                                     size_t Q, int32_t *idx, double *dist);
int ccmp_rrtc_nearest_shape(const ccmp_ctx *ctx, size_t Q, size_t N, unsigned int *part, unsigned int *partitions);
int ccmp_rrtc_pick_ref(int mode, const double *states, const int32_t *n_states, const uint8_t *ok, const uint8_t *use, const double *to, const double *d,
                       size_t E, int max_states, double range, int32_t *outcome, int32_t *row_index, double *row, double *gap);
int ccmp_rrtc_connected_ref(const int32_t *labels, size_t N, ccmp_rrtc_state *state);
/* ccmp_rrtc_pick_ref's arguments as device pointers: the pick kernel of a cycle on its own (rrtc_pick_kernel, sixteen lanes per list),
 * asynchronous on hip_stream and capturable; the same bits as the _ref form */
int ccmp_rrtc_pick_batch(ccmp_ctx *ctx, int mode, const double *states, const int32_t *n_states, const uint8_t *ok, const uint8_t *use, const double *to,
                         const double *d, size_t E, int max_states, double range, int32_t *outcome, int32_t *row_index, double *row, double *gap,
                         void *hip_stream);

/* ---- diagnostics ---------------------------------------------------------------------------------- */
/* (test and tool hooks — the device probe of ccmp_detmath.h, an externally supplied processing order, the scout's predictions, fault
 * injection — are not part of this library: include/ccmp_debug.h, lib/libccmp_debug.so) */
const char *ccmp_strerror(int code);
const char *ccmp_last_hip_error(void);
int ccmp_version(void);
size_t ccmp_problem_sizeof(void);

#ifdef __cplusplus
}
#endif
#endif /* CCMP_H */
