/* ccmp_launch.h — the kernel launchers of libccmp (defined in the ccmp_kernels_*.hip units, called by the host units): the one
 * declaration of each, with C++ linkage (a definition that drifts from it does not compile) and hidden visibility (not exported).
 * Also the layout facts that host and kernels share: the work-queue words, the hand-over record sizes, a split launch's cut. */
#ifndef CCMP_LAUNCH_H
#define CCMP_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct ccmp_consts;
struct ccmp_plan_state;
struct ccmp_rrtc_state;
namespace ccmp { struct scene_dev; struct scene_arm_dev; struct ik_arms; struct ik_params; struct object_boxes; struct object_sphere; struct object_draw; struct graph_roots; struct dense_chunk; struct dense_open_seg; struct shortcut_open; struct smooth_path; struct retime_limits; struct setpoint_limits; struct jerk_limits; }

/* What a split launch asks of the counting sort that precedes it: the cut of the descending order between the latency blocks
 * (front) and the throughput layout (rest), decided by the sort's own kernel from its histogram and left in words 0, 3 and 4 of
 * the block (QueueWord, BulkWord).  Until round 5 two launches of their own: two of the five kernel boundaries before the fork. */
struct ccmp_split_req {
  unsigned long long *queue; /* the block of queue words; nullptr: no split */
  int kind;                  /* 1: the units predicted >= p_low, at most `limit` (projector: fd_split_kernel's rule);
                                2: >= p_high where those carry permille / 1000 of the predicted work, else >= p_low (extend step: apply_split's
                                   second rule, ccmp_kernels_scout.hip) */
  int p_low, p_high, permille;
  unsigned int limit;
  int clear;                 /* this many 64-bit words from queue[0] on are zeroed first (the others of the launch's block) */
};

namespace ccmp_launch {

constexpr int kPoolEntry = 18;    // projector hand-over record, in doubles: x[14], idx, (iter, updates), norm1, norm2
// head -> resume launch of a large projector batch (ccmp_kernels_fd.hip: FdPart): one row per sample, in doubles.  A sample that is
// still iterating behind the head's last function(x) leaves what that evaluation computed — the first kStagedLds doubles of its
// group's LDS record (x 14, sin / cos 28, arm 0's prefix frames 84, both tool poses 24) and the residual pair — with the hand-over
// record's index and counters, so the resume launch takes it up at the Jacobian.  16-byte pieces: the stride is even.
constexpr int kStagedLds = 150;
constexpr int kStagedF = kStagedLds;        // f0, f1
constexpr int kStagedTag = kStagedLds + 2;  // index (-1: the head has written the sample back), (iter, updates) behind the loop test's increment
constexpr int kStagedNorm = kStagedLds + 4; // norm1, norm2
constexpr int kStagedX0 = kStagedLds + 6;   // 1.0: some joint of x failed rot_x0_round_ok in that evaluation (ccmp_kin.h), else 0.0; pad
constexpr int kStagedRow = kStagedLds + 8;
static_assert(kStagedRow % 2 == 0 && kStagedLds % 2 == 0, "rows and their parts are moved in 16-byte pieces");
constexpr int kGeoPoolEntry = 40; // extend-step hand-over of an edge in the middle of a projection: x[14], previous[14], dist, total,
                                  // maxd, edge, (n, its), (rounds, iter), updates, norm1, norm2 (geodesic_group_kernel -> geodesic_flat_kernel)
constexpr int kFastQueues = 64;   // ticket words of the analytic mode's lane-pair kernel: one per lane of a wavefront

/* ctx->queue, in 64-bit words; each launch sequence clears the words it uses */
enum QueueWord : int {
  kQTicket = 0,                                 // projector: throughput kernel's ticket (split launch: starts behind the front)
  kQPool = 1,                                   // projector: hand-over pool's fill count (the kernels count from the back at kQPool + 5)
  kQLatency = 2,                                // projector: latency kernel's ticket
  kQFinished = 3,                               // projector: throughput kernel's finished samples (its occupancy hand-over)
  kQFrontLen = 4,                               // projector, split launch: the front's length
  kQScout = 5,                                  // projector: the scout pass's queue
  kQFront = 7,                                  // projector, split launch: the front's ticket
  kQGeoTicket = 3,                              // extend step: ticket (the projector's words: a call runs one or the other)
  kQGeoOrder = 4,                               // extend step: the ordering pass's two 32-bit counters
  kQAnalytic = 8,                               // analytic projector: kFastQueues lane-pair tickets, pool fill count, latency kernel's ticket
  kQGeoAnalytic = kQAnalytic + kFastQueues + 2, // extend step in analytic mode: ticket
  kQBulk = kQGeoAnalytic + 1,                   // bulk extend step: a block of eight (BulkWord)
  kQueueWords = kQBulk + 8,
};
/* the bulk extend step's block: the group kernel's ticket (starts behind the front) and finished edges (its hand-over rule), the
 * front's length and ticket, the hand-over pool's fill count, the ticket of the launch that drains the pool */
enum BulkWord : int { kBTicket = 0, kBFinished = 3, kBFrontLen = 4, kBFront = 5, kBPool = 6, kBDrain = 7 };

/* what every launch of one projector call shares */
struct ProjectCall {
  const ccmp_consts *K;
  int mode;                       // 0: project q_in, 1: fused sampleUniform
  const double *q_in;
  double *q_out;
  uint8_t *ok;
  uint16_t *iters;                // nullable
  double *q_ambient;              // nullable: the fused sampler's ambient samples
  size_t B;
  unsigned long long seed, first; // the sampler's stream
};

/* what every launch of one extend-step call shares */
struct GeoCall {
  const ccmp_consts *K;
  double delta, lambda;
  const double *from, *to;
  size_t E;
  int max_states;
  double *states;
  int32_t *n_states;
  uint8_t *ok;
  int32_t *newton_iters;
  const double *carry_in; // nullable: a continuation's carries
  double *carry_out;      // nullable
  int round_budget;       // 0: none
  int check_target;       // checkMotion: isSatisfied(to) of every edge
};

/* what an extend-step call with a proxy scene adds (ccmp_geodesic_scene_batch) */
struct GeoScene {
  const ccmp::scene_dev *scene;
  double margin;     // a state is valid when its clearance exceeds this
  uint8_t *blocked;  // nullable, [E]
  double *clearance; // nullable, [E][max_states]
};

/* one launch of project_fd_flat_kernel, the projector's latency kernel */
struct FlatLaunch {
  int blocks = 0;
  unsigned long long *queue = nullptr;                                      // ticket word; nullptr: one block per sample, static striding
  bool from_pool = false;                                                   // the samples handed over through the pool, else the call's
  const double *pool = nullptr; const unsigned long long *pool_count = nullptr; // the pool and its fill count
  size_t pool_records = 0;                                                  // two-class pool: its capacity (0: filled from the front only)
  const unsigned int *order = nullptr;                                      // processing order ...
  const unsigned long long *total = nullptr;                                // ... of which a split launch's front takes the first *total
  unsigned int *done_flag = nullptr, done_seq = 0;                          // single-state call: completion word (one block only), value
};

/* one launch of geodesic_flat_kernel, the extend step's latency kernel */
struct GeoLaunch {
  int blocks = 0;
  unsigned long long *queue = nullptr;                                     // ticket word; nullptr: one block per edge, static striding
  const unsigned int *order = nullptr;                                     // processing order ...
  const unsigned long long *total = nullptr;                               // ... of which a bulk call's front takes the first *total
  const double *pool = nullptr; const unsigned long long *pool_count = nullptr; // drain of a bulk call: the edges handed over, their count
};

/* one k-nearest-neighbour call (ccmp_knn_batch) ... */
struct KnnCall {
  const double *nodes; size_t N;
  const double *queries; size_t Q;
  int k, mode;
  size_t self_base;
  int32_t *nbr_idx;  // [Q][k]
  double *nbr_dist;  // [Q][k], nullable
};
/* ... and its launch shape (ccmp_policy.cpp: plan_knn).  No field changes a result bit. */
constexpr int kKnnThreads = 256; // threads per block of every k-NN kernel; queries per block of the many-query kernel
constexpr int kKnnTile = 256;    // nodes per LDS tile of the many-query kernel (28 KB)
constexpr int kKnnMaxPartitions = 256; // the merge kernel holds one partition's list per thread
constexpr int kKnnPoseTile = 512; // poses per LDS tile of the many-query kernel of the object metric (64-byte rows: 32 KB)
struct KnnShape {
  bool few = false;            // knn_few_kernel: one block per (partition, query), else knn_many_kernel: one query per thread
  unsigned int groups = 0;     // many-query kernel: blocks of kKnnThreads queries
  unsigned int partitions = 1; // cuts of the node range; > 1: partial lists in the workspace + knn_merge_kernel
  unsigned int part = 0;       // nodes per partition (a multiple of kKnnTile)
  int kc = 0;                  // list capacity the kernels are instantiated for: 1, 4, 8 or 16 (>= k)
  size_t workspace_bytes = 0;  // Q * partitions * kc * 12, 0 with one partition
};

/* one pose-targeted IK call (ccmp_pose_ik_batch; csrc/ccmp_ik.h): T targets x S seed slots x 2 arms x (1 + restarts) candidates, their
 * records in the context's workspace at candidate index ((t S + s) 2 + a) (1 + restarts) + r */
struct IkCall {
  const ccmp_consts *K;
  const ccmp::ik_arms *arms;
  const ccmp::ik_params *P;
  const double *poses;  // [T][8]
  const double *seeds;  // [T][S][14]
  size_t T; int S;
  unsigned long long rng_seed, first_index;
  double *rec_q;        // [candidates][7]
  int32_t *rec_rounds;  // [candidates]
  double *rec_d2;       // [candidates]
};

/* one call on an object checker (ccmp_object_*; csrc/ccmp_object.h): the mesh as nine planes of `plane` doubles on the device, the boxes
 * and the bounding sphere as the kernels take them by value */
constexpr int kObjectThreads = 256; // lanes per block of the object kernels: one block per pose / grow index, the triangles strided over them
struct ObjectCall {
  const ccmp::object_boxes *boxes;
  const ccmp::object_sphere *sphere;
  const double *tri; // [9][plane]
  int M; size_t plane;
  int n_boxes;
};

/* one call on the roadmap graph (ccmp_roadmap_commit / _add_edges / _closest; csrc/ccmp_graph.h): the store's arrays and the call's
 * workspace.  Per slot (S = Q k of a commit): flags, label, weight, mid_pose; per item of the scan (a commit's queries, add_edges'
 * edges): the decision's masks, the counts and the bases; totals = {vertices added, edges added, new edge floor}. */
constexpr int kGraphThreads = 256;          // lanes per block of the graph kernels; the hooking rounds and the scan run in ONE such block
constexpr int kClosestMaxPartitions = 256;  // cuts of the vertex range of a closest call: its merge holds one partition's best per lane
struct GraphStore {
  double *joints, *poses; // [cap][14], [cap][8]
  int32_t *labels;        // [cap]
  int32_t *uv;            // [cap_e][2]
  double *w;              // [cap_e]
  size_t N, E, floor;     // size, edge count and edge floor at call entry
};
struct GraphWork {
  uint32_t *flags;   // [S]
  int32_t *label;    // [S]
  double *weight;    // [S]
  double *mid_pose;  // [S][8]
  uint32_t *masks;   // [n]: reached | mid << 16
  int32_t *cnt_v, *cnt_e, *hi, *base_v, *base_e; // [n] each
  int32_t *totals;   // [4]
};
struct GraphCommit {
  const ccmp_consts *K; // nullable: no mid-stones
  const int32_t *nbr_idx; const uint8_t *edge_ok; const int32_t *n_states; const double *states; int max_states;
  const double *new_joints, *new_poses; const uint8_t *vertex_ok;
  size_t Q; int k;
  double goal[8]; int has_goal; // the goal pose, by value; has_goal == 0: no mid-stones
  const ccmp::graph_roots *roots;
  int keep_isolated;
  int32_t *new_index, *mid_index, *grow_state;
};

/* one shortest-path call (ccmp_roadmap_shortest_paths; csrc/ccmp_path.h): the pairs, the per-pair arrays of the handle's workspace and
 * the caller's outputs.  d holds the distances' bits. */
constexpr int kPathThreads = 1024;  // lanes of the ONE block that runs a pair's relaxation and hop rounds
struct GraphPath {
  const int32_t *src, *dst; int F; // [F] each
  unsigned long long *d;           // [F][N]
  int32_t *hops, *pred, *stamp;    // [F][N] each
  int32_t *rounds;                 // [F][2]: the relaxation and hop rounds the call took
  int max_len;
  double *cost; int32_t *path_len, *path; // [F], [F], [F][max_len]
  double *path_joints, *path_poses;       // [F][max_len][14], [F][max_len][8]; nullable
};

/* one check of the planner's loop (csrc/ccmp_plan.h): ccmp_roadmap_closest's arrays of both sides (a: from starts towards goals[0], b: from
 * goals towards starts[0]), the goal and start poses by value, and what the kernel writes for the IK call that follows */
struct PlanCheck {
  const int32_t *a_idx; const double *a_dist, *a_from;
  const int32_t *b_idx; const double *b_dist, *b_from;
  double goal[8], start[8];
  double *targets; // [11][8]: goal, ladder 1 .. 9, start; a NaN row where the branch did not fire
  double *seeds;   // [11][14]
  int32_t *trig;   // [4]
};

/* RRT-Connect on the store (csrc/ccmp_rrtc.h).  One pick over E traversal lists: mode 0 = step 2 (d: the nearest distances), 1 = step 3
 * (gap out); use [E] (nullable: all 1) as rrtc_edges wrote it; nearest [E] (nullable) -> parent [E] (nullable) where an edge results */
constexpr int kRrtcThreads = 256;          // lanes per block of the RRT-Connect kernels; the commit kernel's ONE block bounds the width
constexpr int kRrtcMaxPartitions = 256;    // cuts of the vertex range of a nearest-in-tree call: its merge holds one partition's best per lane
struct RrtcPick {
  int mode;
  const double *states; const int32_t *n_states; const uint8_t *ok; const uint8_t *use;
  const double *to, *d; const int32_t *nearest;
  size_t E; int max_states; double range;
  int32_t *outcome, *row_index; double *row; // [E], [E], [E][14]
  int32_t *parent; uint8_t *made; double *gap; // nullable, [E] each
};
/* one commit of a cycle of width W <= kRrtcThreads: step 2's (A) and step 3's (B) picks -> rows [2 W][14], uv [2 W][2], counts [4] =
 * {vertices, edges, step 2's vertices, step 3's vertices} */
struct RrtcCommit {
  int W, a_is_start;
  const uint8_t *useA;
  const int32_t *outA, *parA; const double *rowA;
  const int32_t *outB, *parB, *idxB; const double *rowB, *gapB;
  double *rows; int32_t *uv, *counts;
};

#pragma GCC visibility push(hidden)
/* label[first + i] = first + i (an append) */
hipError_t graph_iota(int32_t *labels, size_t first, size_t n, hipStream_t st);
/* slots -> decisions -> scan -> scatter (rows, edges, labels, the caller's index arrays); totals are on the device afterwards */
hipError_t graph_commit(const GraphStore &s, const GraphWork &w, const GraphCommit &c, hipStream_t st);
/* explicit edges: validity and scan, then the weights and the scatter */
hipError_t graph_add_edges(const GraphStore &s, const GraphWork &w, const int32_t *uv, size_t E, hipStream_t st);
/* the call's new edges (uv[E .. E + totals[1])) into the labels: hooking rounds in one block, then label[i] = root(label[i]) over the
 * s.N + totals[0] labels that exist (at most n_after: the grid) as a launch of its own; max_new bounds every loop */
hipError_t graph_components(const GraphStore &s, const int32_t *totals, size_t n_after, size_t max_new, hipStream_t st);
/* blocks over (partition, from), bests of one, then the exact merge (partitions > 1: ws_d [F][P], ws_i [F][P]) */
hipError_t graph_closest(const GraphStore &s, const int32_t *from_idx, size_t F, const double *target, unsigned int part, unsigned int partitions,
                         double *ws_d, int32_t *ws_i, int32_t *idx, double *dist, double *from_dist, hipStream_t st);
/* init -> rounds in one block per pair -> extract (cost, length, path, rows); s.N == 0: the extract alone */
hipError_t graph_paths(const GraphStore &s, const GraphPath &p, hipStream_t st);
/* dense solution paths (ccmp_path_densify; csrc/ccmp_dense.h).  Endpoint gather of one extend call's E open segments: from / to [E][14] and,
 * for a continuation (prev_states, prev_carry given), carry_in [E][2]; waypoints = path_joints seen as rows [F * max_len][14] */
hipError_t dense_gather(const ccmp::dense_open_seg *open, size_t E, const double *waypoints, const double *prev_states, int chunk_states,
                        const double *prev_carry, double *from, double *to, double *carry_in, hipStream_t st);
/* one wavefront per chunk: its rows to their final place (a chunk reaching beyond total_rows is skipped), its Newton count into seg_newton */
hipError_t dense_pack(const ccmp::dense_chunk *chunks, size_t n, double *rows, size_t total_rows, int32_t *seg_newton, size_t slots, hipStream_t st);
/* one block per path: the serial arc chain and the path's length */
hipError_t dense_arc(const double *rows, const int32_t *path_first, size_t F, double *arc, double *length, hipStream_t st);
/* one block per path: (min clearance, first row attaining it) and the first row below the margin */
hipError_t dense_clearance_summary(const double *clearance, const int32_t *path_first, size_t F, double margin, double *min_clear, int32_t *min_row,
                                   int32_t *first_blocked, hipStream_t st);
/* shortcut solution paths (ccmp_path_shortcut, ccmp_shortcut_select; csrc/ccmp_shortcut.h).  One tile of pair slots [first, first + T) of the
 * enumeration over all paths (prefix [F + 1] = the slots before each path, from path_len and max_span alone): slot k's matrix entry
 * cell[k] = (f max_len + i) max_len + j and its endpoint rows from / to [T][14]; a slot with a non-finite row is no candidate: cell -1 and
 * zero rows (no NaN endpoint reaches a traversal) */
hipError_t shortcut_enumerate(const double *path_joints, const int32_t *path_len, const long long *prefix, size_t F, int max_len, int max_span,
                              long long first, size_t T, long long *cell, double *from, double *to, hipStream_t st);
/* the endpoints of a continuation's E open pairs: from = the last stored row of the previous call's list, to and carry as they were */
hipError_t shortcut_regather(const ccmp::shortcut_open *open, size_t E, const double *prev_states, int chunk_states, const double *prev_to,
                             const double *prev_carry, double *from, double *to, double *carry_in, hipStream_t st);
/* after an extend call over E open pairs (open == nullptr: the tile's first call, pair k = slot k): the states and Newton rounds the call
 * contributed are added to the pair's matrix entries, and the flag of a pair that is no longer open is written; cell == nullptr (a tile of
 * explicit pairs): slot k's entry is cell_base + k */
hipError_t shortcut_scatter(const ccmp::shortcut_open *open, size_t E, const long long *cell, long long cell_base, const int32_t *n_states, const uint8_t *ok,
                            const int32_t *newton, const uint8_t *blocked, int chunk_states, size_t cells, uint8_t *pair_ok, int32_t *pair_states,
                            int32_t *pair_newton, hipStream_t st);
/* one block per path: the forward sweep over the DAG of admitted edges, the walk of pred, the costs */
hipError_t shortcut_select(const double *path_joints, const int32_t *path_len, size_t F, int max_len, const uint8_t *pair_ok, int32_t *out_len,
                           int32_t *kept, double *cost_in, double *cost_out, hipStream_t st);
/* out_joints[f][k] = path_joints[f][kept[f][k]] for k < out_len[f]; rows behind are not written */
hipError_t shortcut_gather_kept(const double *path_joints, const int32_t *out_len, const int32_t *kept, size_t F, int max_len, double *out_joints,
                                hipStream_t st);
/* smooth solution paths (ccmp_path_smooth; csrc/ccmp_smooth.h).  The caller's rows k < path_len[f] into buf [F][cap][14]; bad[f] = 1 where one
 * of them is not finite */
hipError_t smooth_load(const double *path_joints, const int32_t *path_len, size_t F, int max_len, int cap, double *buf, uint8_t *bad, hipStream_t st);
/* the E pairs of one stage of a pass over the nA active paths (cur = the current path buffer [F][cap][14]): stage 0 (w_i, w_{i+1}) per
 * segment, 1 (m_{i-1}, w_i), (w_i, m_i) per interior vertex, 2 (t1, t2) — into pairs [E][2][14], pair_path [E] = the pair's path — and 3 the two
 * tests (m_{i-1}, c_i), (c_i, m_i) into from / to [E][14] */
hipError_t smooth_gather(int stage, const ccmp::smooth_path *paths, size_t nA, size_t E, const double *cur, int cap, const double *m, const double *t12,
                         const double *cand, double *pairs, double *from, double *to, int32_t *pair_path, hipStream_t st);
/* per pair e with the dense rows [path_first[e], path_first[e + 1]) and their arcs: x[e] = the blend at half the arc (row 0 for a degenerate
 * list), choice[e] = the fallback row, -1 for a degenerate list */
hipError_t smooth_bracket(const double *rows, const double *arc, const int32_t *path_first, size_t E, size_t total_rows, double *x, int32_t *choice,
                          hipStream_t st);
/* mid[e] = degenerate: row 0; ok[e]: y[e]; else the fallback row; the kind is counted in stats [F][5] of the pair's path */
hipError_t smooth_pick(const double *rows, const int32_t *path_first, const int32_t *choice, const double *y, const uint8_t *ok, const int32_t *pair_path,
                       size_t E, size_t total_rows, size_t F, double *mid, int32_t *stats, hipStream_t st);
/* the subdivided paths of the active paths into `next`: items = their vertices; moved [F] and stats [F][5] are added to */
hipError_t smooth_accept(const ccmp::smooth_path *paths, size_t nA, size_t items, const double *cur, int cap, const double *m, const double *cand,
                         const uint8_t *test_ok, const double *clear_m, const double *clear_c, double margin, double min_change, double *next,
                         int32_t *moved, int32_t *stats, hipStream_t st);
/* length[f] = the left-to-right sum of the adjacent joint distances of path f's first len[f] rows in buf0 (where[f] != 0: buf1) */
hipError_t smooth_length(const double *buf0, const double *buf1, const uint8_t *where, const int32_t *len, size_t F, int cap, double *length, hipStream_t st);
/* out_joints[f][k] = the path's row k for k < len[f]; rows behind are not written */
hipError_t smooth_store(const double *buf0, const double *buf1, const uint8_t *where, const int32_t *len, size_t F, int cap, double *out_joints,
                        hipStream_t st);
/* resample and time stamps (ccmp_path_resample, ccmp_path_timestamps; csrc/ccmp_retime.h).  status [F] of the packed rows' paths: EMPTY (also a
 * range that is negative, decreasing or beyond total_rows), NONFINITE, else OK; a_bits [F] (nullable) reset to "no interval yet" */
hipError_t retime_status(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, int32_t *status, unsigned long long *a_bits, hipStream_t st);
/* per output row g < M of the paths' output ranges out_first [F + 1]: x[g] = the blend at h_j (a copied or degenerate row: its source row),
 * choice[g] = the fallback (or source) dense row, kind[g] = the kind so far (kRetimePending: the projector's flag decides) */
hipError_t resample_bracket(const double *rows, const double *arc, const int32_t *path_first, const int32_t *status, const int32_t *out_first, size_t F, size_t M,
                            size_t total_rows, double *x, int32_t *choice, uint8_t *kind, hipStream_t st);
/* out_rows[g] = y[g] (projected) or the dense row choice[g]; kind [M] final; counts [F][4] are added to */
hipError_t resample_pick(const double *rows, const int32_t *out_first, size_t F, size_t M, size_t total_rows, const int32_t *choice, const uint8_t *kind_so_far,
                         const double *y, const uint8_t *ok, double *out_rows, uint8_t *kind, int32_t *counts, hipStream_t st);
/* ceiling[r] = x_i of every row of an OK path; a_bits[f] = the bits of the path's minimum of A */
hipError_t retime_ceiling(const double *rows, const int32_t *path_first, size_t F, size_t total_rows, const int32_t *status, const ccmp::retime_limits &lim,
                          double *ceiling, unsigned long long *a_bits, hipStream_t st);
/* envelope[r] = y_i */
hipError_t retime_envelope(const double *ceiling, const int32_t *path_first, size_t F, size_t total_rows, const int32_t *status, const unsigned long long *a_bits,
                           double *envelope, hipStream_t st);
/* time[r] and duration[f]; rows of a path that is not OK are not written, its duration is +0.0 (EMPTY) or NaN (NONFINITE) */
hipError_t retime_stamp(const double *rows, const double *envelope, const int32_t *path_first, const int32_t *status, const unsigned long long *a_bits,
                        const ccmp::retime_limits &lim, size_t F, double *time, double *duration, hipStream_t st);
/* controller-rate setpoints and the execution audit (ccmp_path_setpoints; csrc/ccmp_setpoints.h).  status [F] and ticks [F] of the packed rows'
 * paths under their stamps: EMPTY (also a range that is negative, decreasing or beyond total_rows), NONFINITE, UNORDERED, POINT (one tick), FULL, OK */
hipError_t setpoints_status(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, double period, int max_ticks,
                            int32_t *status, int32_t *ticks, hipStream_t st);
/* tangent [total_rows][14] = w_i of every row of an OK path */
hipError_t setpoints_tangent(const double *rows, const int32_t *path_first, const double *time, size_t F, size_t total_rows, const int32_t *status,
                             double *tangent, hipStream_t st);
/* per tick g < M of the paths' tick ranges tick_first [F + 1]: q, qd [M][14], tau [M]; clearance [M] = NaN (a scene's answer replaces it) */
hipError_t setpoints_sample(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *status,
                            const int32_t *tick_first, size_t F, size_t M, size_t total_rows, double period, double *q, double *qd, double *tau,
                            double *clearance, hipStream_t st);
/* one block per path: peak, peak_tick [F][5], counts [F][2], stretch [F] */
hipError_t setpoints_peak(const double *qd, const double *tau, const double *f, const uint8_t *satisfied, const double *clearance, const int32_t *tick_first,
                          size_t F, size_t M, const ccmp::setpoint_limits &lim, double margin, double *peak, int32_t *peak_tick, int32_t *counts,
                          double *stretch, hipStream_t st);
/* time stamps fitted to the limits at the controller's rate (ccmp_path_fit_timestamps; csrc/ccmp_fit.h).  time_out = time over every path's
 * checked range; status [F] = open, passes [F] = 0, peak [F][2] and duration [F] = +0.0 */
hipError_t fit_begin(const int32_t *path_first, const double *time, size_t F, size_t total_rows, double *time_out, int32_t *status, int32_t *passes,
                     double *peak, double *duration, hipStream_t st);
/* per tick interval g < M of the paths' ranges tick_first [F + 1] (N - 1 intervals for a path that is measured, none for any other): s_j and
 * a_j folded into S and A [total_rows] (bit patterns, cleared before) at the rows of the interval's brackets */
hipError_t fit_measure(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *tick_first, size_t F,
                       size_t M, size_t total_rows, double period, const ccmp::setpoint_limits &lim, unsigned long long *S, unsigned long long *A,
                       hipStream_t st);
/* one wavefront per open path: sp_status (this pass's setpoints status) ends it, or the done test does, or its stamps are dilated in place
 * and its S and A cleared */
hipError_t fit_dilate(const int32_t *path_first, const int32_t *sp_status, size_t F, double aim, int max_passes, double *time, unsigned long long *S,
                      unsigned long long *A, int32_t *status, int32_t *passes, double *peak, double *duration, hipStream_t st);
/* factor[r] = time_out's interval over time's at its right row; row 0 of a path and intervals without positive input width: 1.0 */
hipError_t fit_factor(const int32_t *path_first, size_t F, size_t total_rows, const double *time, const double *time_out, double *factor, hipStream_t st);
/* jerk-bounded setpoints (ccmp_path_jerk_setpoints; csrc/ccmp_jerk.h).  The tile lengths of the two staging kernels, whose static LDS they size */
constexpr int kJerkTile = 128, kJerkSampleTile = 32;
/* one block per tile < tiles of tile_ticks output ticks of the open paths (tile_first [F + 1]; word [f] = M, window [f] = W, sp_ticks [f] = n + 1): the
 * path's jerk peak for W folded into P [f] (bit patterns, cleared before) */
hipError_t jerk_measure(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *tile_first, size_t tiles,
                        const int32_t *word, const int32_t *window, const int32_t *sp_ticks, size_t F, size_t total_rows, double period, int tile_ticks,
                        const ccmp::jerk_limits &lim, unsigned long long *P, hipStream_t st);
/* one lane per path.  begin: the setpoints status ends a path or it opens with its first window; else an open path's P [f] is read and cleared
 * and the path ends OK / WINDOW / FULL or goes on with the next window.  word [f] = M of an open path, -1 - M of a closed one */
hipError_t jerk_decide(const int32_t *sp_status, const int32_t *sp_ticks, size_t F, bool begin, int fixed_window, int max_window, double aim, int max_ticks,
                       unsigned long long *P, int32_t *status, int32_t *window, int32_t *passes, int32_t *word, hipStream_t st);
/* one block per tile < tiles of tile_ticks ticks of the delivered paths (tile_first [F + 1] over tick_first [F + 1]): q, qd [total_ticks][14], tau
 * [total_ticks]; clearance [total_ticks] = NaN (a scene's answer replaces it) */
hipError_t jerk_sample(const double *rows, const int32_t *path_first, const double *time, const double *tangent, const int32_t *tile_first, size_t tiles,
                       const int32_t *tick_first, const int32_t *status, const int32_t *window, const int32_t *sp_ticks, size_t F, size_t total_ticks,
                       size_t total_rows, double period, int tile_ticks, double *q, double *qd, double *tau, double *clearance, hipStream_t st);
/* one block per path: peak, peak_tick [F][6], counts [F][2] */
hipError_t jerk_peak(const double *qd, const double *f, const uint8_t *satisfied, const double *clearance, const int32_t *tick_first, size_t F, size_t total_ticks,
                     double period, const ccmp::jerk_limits &lim, double margin, double *peak, int32_t *peak_tick, int32_t *counts, hipStream_t st);
/* ccmp_object_create: rows [M][9] -> planes [9][plane] */
hipError_t object_planes(const double *rows, int M, size_t plane, double *planes, hipStream_t st);
/* one block per pose; hit_mask == nullptr: the form that leaves at the first chunk with a hit (the same `valid`) */
hipError_t object_valid(const ObjectCall &c, const double *poses, size_t T, double inflate, uint8_t *valid, uint32_t *hit_mask, hipStream_t st);
/* one block per grow index: interpolate, draw, test, attempt by attempt */
hipError_t object_propose(const ObjectCall &c, const ccmp::object_draw &D, const double *from_poses, const double *to_poses, size_t G, double *pose_out,
                          int32_t *which, double *cand_pose, uint8_t *cand_valid, hipStream_t st);
hipError_t ik_solve(const IkCall &c, hipStream_t st);
hipError_t ik_select(const IkCall &c, double *q_out, uint8_t *ok, int32_t *which, hipStream_t st);
/* the vetted IK (csrc/ccmp_ik_vet.h).  ik_vet: the arm clearance of n_rows rows of seven joints for each of the arms arm0 .. arm0 + n_arms - 1
 * (the grid's second dimension); per > 0: the rows are a pose-IK call's records, row n = ts per + r of an arm at record (2 ts + arm) per + r,
 * -inf where rounds < 0; per == 0: the caller's own rows (rounds == nullptr).  ik_assemble: the per-arm rule per slot -> slot_q [slots][14]
 * (zeros without a state), slot_has.  ik_pick: the first slot with a state and a slot clearance > margin */
hipError_t ik_vet(const ccmp_consts *K, const ccmp::scene_dev *scene, const ccmp::scene_arm_dev *arms, const double *q7, const int32_t *rounds, size_t n_rows,
                  int per, int arm0, int n_arms, double margin, double *clear, uint8_t *free_out, hipStream_t st);
hipError_t ik_assemble(const double *rec_q, const int32_t *rec_rounds, const double *rec_d2, const double *cand_clear, size_t slots, int R, double margin,
                       double *slot_q, uint8_t *slot_has, hipStream_t st);
hipError_t ik_pick(const double *slot_q, const uint8_t *slot_has, const double *slot_clear, size_t T, int S, double margin, double *q_out, uint8_t *ok,
                   int32_t *which, double *clearance, double *slot_out, hipStream_t st);
/* ccmp_roadmap_grow: seeds[q][r] = the store's joint row nbr_idx[q][r] (NaN for an empty slot) */
hipError_t ik_gather_seeds(const double *joints, const int32_t *nbr_idx, size_t slots, double *seeds, hipStream_t st);
/* ccmp_roadmap_grow: what the traversal sees — masked[q][r] = nbr_idx[q][r] where target q has a state and the neighbour's joint row is
 * finite, else -1 (an empty slot); q_trav[q] = q_new[q], or zeros for a target without a state (no NaN endpoint reaches a traversal) */
hipError_t ik_grow_prepare(const double *joints, const int32_t *nbr_idx, const uint8_t *ik_ok, const double *q_new, size_t Q, int k, int32_t *masked,
                           double *q_trav, hipStream_t st);
hipError_t knn(const KnnCall &c, const KnnShape &s, void *workspace, hipStream_t st);
/* the same call on the object metric: nodes = the store's pose rows [N][8], queries [Q][8]; shape from plan_knn_pose (part a multiple of kKnnPoseTile) */
hipError_t knn_pose(const KnnCall &c, const KnnShape &s, void *workspace, hipStream_t st);
/* what an append to the roadmap store runs: poses[i] = pose of joints[i] (t_wo_kernel's arithmetic, then Quaterniond(Matrix3d)); the caller's
 * poses with the pad zeroed; NaN joint rows */
hipError_t pose_from_joints(const ccmp_consts *K, const double *joints, double *poses, size_t n, hipStream_t st);
hipError_t pose_store(const double *src, double *dst, size_t n, hipStream_t st);
hipError_t joints_fill_nan(double *dst, size_t n, hipStream_t st);
hipError_t connect_gather(const double *nodes, const double *queries, const int32_t *nbr_idx, size_t E, int k, double *from, double *to, hipStream_t st);
hipError_t connect_fix(const int32_t *nbr_idx, size_t E, int32_t *n_states, uint8_t *ok, int32_t *newton_iters, uint8_t *blocked, double *carry_out,
                       hipStream_t st);
hipError_t clear_words(void *words, size_t n_u32, hipStream_t st);
/* which part of a projector call a launch of project_fd_kernel is (ccmp_kernels_fd.hip): all of it, or — large batches without
 * hand-over — every sample's first rounds in index order (head), then the persistent kernel on the rows the head left (resume) */
enum FdPart : int { kFdWhole = 0, kFdHead = 1, kFdResume = 2 };
hipError_t project_group(const ProjectCall &c, int blocks, unsigned long long *queue, double *pool, int dump_threshold, const unsigned int *order,
                         const uint16_t *pred, int long_remaining, size_t pool_records, hipStream_t st, FdPart part = kFdWhole,
                         double *state = nullptr, int head_rounds = 0);
hipError_t project_wave(const ProjectCall &c, bool from_pool, int blocks, unsigned long long *queue, const double *pool,
                        const unsigned long long *pool_count, hipStream_t st);
hipError_t project_flat(const ProjectCall &c, const FlatLaunch &l, hipStream_t st);
hipError_t project_analytic(const ProjectCall &c, int pair_blocks, int dump_below, int latency_blocks, double *pool, unsigned long long *queue, hipStream_t st);
/* the launches of scout_order: the histogram's clear, the scout pass (-> pred), the counting sort (pred -> order) */
enum ScoutStep : int { kScoutClear = 1, kScoutPass = 2, kScoutSort = 4, kScoutAll = 7 };
hipError_t scout_order(const ProjectCall &c, uint16_t *pred, unsigned int *hist, unsigned int *order, unsigned long long *queue, int blocks,
                       int pair_max_blocks, const ccmp_split_req *split, hipStream_t st, int steps = kScoutAll);
/* the counting sort both scout orders end with: n keys (pred, clamped to 1023) -> order, descending; hist[k] = the keys >= k afterwards;
 * split.queue != nullptr: the cut of the order too.  One launch where !sort_needs_clear(n); else histogram (hist_blocks blocks), scan over
 * nbins bins (every key < nbins), scatter — on a hist whose 1024 words the caller has cleared */
bool sort_needs_clear(size_t n);
hipError_t sort_desc(const uint16_t *pred, size_t n, int nbins, int hist_blocks, unsigned int *hist, unsigned int *order, const ccmp_split_req &split,
                     hipStream_t st);
hipError_t fd_split(const unsigned int *hist, int pred_min, unsigned int limit, unsigned long long *queue, hipStream_t st);
hipError_t geo_split(const unsigned int *hist, int p_min, int p_max, int permille, unsigned long long *queue, hipStream_t st);
hipError_t geodesic(const GeoCall &g, const GeoLaunch &l, hipStream_t st);
hipError_t geodesic_lat(const GeoCall &g, const GeoLaunch &l, hipStream_t st);
hipError_t geodesic_group(const GeoCall &g, int blocks, unsigned long long *queue, const unsigned int *order, double *pool,
                          unsigned long long *pool_count, int handover_pct, const uint8_t *target_ok, hipStream_t st);
hipError_t geodesic_analytic(const GeoCall &g, int blocks, unsigned long long *queue, hipStream_t st);
hipError_t geodesic_scene(const GeoCall &g, const GeoScene &s, int blocks, unsigned long long *queue, hipStream_t st);
hipError_t geodesic_analytic_scene(const GeoCall &g, const GeoScene &s, int blocks, unsigned long long *queue, hipStream_t st);
hipError_t geodesic_scout_order(const GeoCall &g, int round_cap, uint16_t *pred, unsigned int *hist, unsigned int *order, int pairs,
                                const ccmp_split_req *split, hipStream_t st);
hipError_t geodesic_order(const double *from, const double *to, size_t E, double long_dist, unsigned int *counters, unsigned int *order, hipStream_t st);
hipError_t function(const ccmp_consts *K, const double *q, double *f, size_t B, unsigned int *done_flag, unsigned int done_seq, hipStream_t st);
hipError_t is_satisfied(const ccmp_consts *K, const double *q, uint8_t *ok, size_t B, unsigned int *done_flag, unsigned int done_seq, hipStream_t st);
hipError_t joint_valid(const ccmp_consts *K, const double *q, uint8_t *ok, size_t B, unsigned int *done_flag, unsigned int done_seq, hipStream_t st);
hipError_t ambient_uniform(const ccmp_consts *K, unsigned long long seed, unsigned long long first, double *q, size_t B, hipStream_t st);
hipError_t ambient_ref(const ccmp_consts *K, int kind, unsigned long long seed, unsigned long long first, const double *ref, int ref_stride,
                       double param, double *q, size_t B, hipStream_t st);
hipError_t t_wo(const ccmp_consts *K, const double *q, int q_stride, double *out, size_t B, hipStream_t st);
hipError_t enforce_bounds(double *q, size_t B, hipStream_t st);
hipError_t compact(const double *q, const uint8_t *ok, size_t B, double *out, size_t capacity, unsigned int *block_counts, unsigned long long *total, hipStream_t st);
size_t clearance_lds_bytes(int n_spheres);
hipError_t clearance(const ccmp_consts *K, const ccmp::scene_dev *scene, int n_spheres, int n_pairs, const double *q, const uint8_t *ok_in, size_t B,
                     double margin, double *clearance, int32_t *pair, uint8_t *free_out, int blocks, int per_state, unsigned int *done_flag,
                     unsigned int done_seq, hipStream_t st);
hipError_t resident(int stock, void *box_dev, unsigned long long last_tag, unsigned long long idle_ticks, hipStream_t st);
hipError_t resident_row16(int diag, void *box_dev, unsigned long long last_tag, unsigned long long idle_ticks, hipStream_t st);
/* the planner's loop (ccmp_plan_*; csrc/ccmp_plan.h, ccmp_kernels_plan.hip): one block each, on the state block of the handle */
hipError_t plan_front(const ccmp_plan_state *state, double *from, size_t W, hipStream_t st);
/* a growth step's outputs (ladder == 0: all counters, proposals += W, next_index += W) or a ladder's new_index [W] (ladder == 1) */
hipError_t plan_tally(ccmp_plan_state *state, const int32_t *which, const uint8_t *ik_ok, const int32_t *new_index, const int32_t *mid_index,
                      const int32_t *grow_state, size_t W, int k, int ladder, hipStream_t st);
hipError_t plan_check(const GraphStore &s, ccmp_plan_state *state, const PlanCheck &c, hipStream_t st);
/* valid [9], ik_ok [11] (goal, ladder, start) -> vertex_ok [9], summary [4] = {prefix length, goal solved, start solved, the check ran} */
hipError_t plan_prefix(const ccmp_plan_state *state, const int32_t *trig, const uint8_t *valid, const uint8_t *ik_ok, uint8_t *vertex_ok, int32_t *summary,
                       hipStream_t st);
hipError_t plan_push(ccmp_plan_state *state, int which, const int32_t *new_index, hipStream_t st);
/* cycle += bump_cycle, then the solution test on the store's labels: one kernel text for both planners' state blocks */
hipError_t plan_connected(const GraphStore &s, ccmp_plan_state *state, int bump_cycle, hipStream_t st);
hipError_t plan_connected(const GraphStore &s, ccmp_rrtc_state *state, int bump_cycle, hipStream_t st);
/* RRT-Connect on the store (ccmp_rrtc_*, ccmp_roadmap_nearest_in_tree; csrc/ccmp_rrtc.h, ccmp_kernels_rrtc.hip).  Blocks over (partition,
 * query), then the exact merge (partitions > 1: ws_d [Q][P], ws_i [Q][P]); roots [n_roots] is device memory */
hipError_t rrtc_nearest(const GraphStore &s, const int32_t *roots, int n_roots, const double *queries, size_t Q, unsigned int part, unsigned int partitions,
                        double *ws_d, int32_t *ws_i, int32_t *idx, double *dist, hipStream_t st);
/* from [E][14] = the store's joints at idx [E], to = rows [E][14]; use [E] = 0 where one of the (nullable) flag arrays is 0, 2 without a nearest
 * vertex, else 1; an edge that is not used runs from a zero row to a zero row */
hipError_t rrtc_edges(const GraphStore &s, const int32_t *idx, const double *rows, const uint8_t *f0, const uint8_t *f1, const uint8_t *f2, size_t E,
                      double *from, double *to, uint8_t *use, hipStream_t st);
hipError_t rrtc_pick(const RrtcPick &c, hipStream_t st);
hipError_t rrtc_commit(const GraphStore &s, ccmp_rrtc_state *state, const RrtcCommit &c, hipStream_t st);
// lib/libccmp_debug.so only (ccmp_kernels_debug.hip)
hipError_t detmath_probe(const double *x, const double *y, double *out, size_t n, hipStream_t st);
hipError_t div_probe(const double *num, const double *den, double *out, size_t n, hipStream_t st);
hipError_t round_facts_probe(const double *m, const double *y, const unsigned char *store, double *out, size_t n, hipStream_t st);
#pragma GCC visibility pop

}  // namespace ccmp_launch

#endif /* CCMP_LAUNCH_H */
