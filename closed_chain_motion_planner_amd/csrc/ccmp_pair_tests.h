/* ccmp_pair_tests.h — what the path units share on the host (ccmp_shortcut.cpp, ccmp_dense.cpp, ccmp_smooth.cpp, ccmp_retime.cpp): the
 * checks every traversing entry point begins with, the tile and continuation loop of checkMotion tests over pairs of rows, and the
 * dense form of a batch of paths as the library keeps it.  Host only, C++ linkage, hidden: nothing here is exported. */
#ifndef CCMP_PAIR_TESTS_H
#define CCMP_PAIR_TESTS_H
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/ccmp.h"
#include "ccmp_scene.h"
#include "ccmp_stage.h"

/* the result of ccmp_path_densify: one allocation, the arrays point into it */
struct ccmp_dense_paths {
  ccmp_ctx *ctx = nullptr;
  int device = 0;
  size_t F = 0, rows = 0, slots = 0; // slots = F (max_len - 1)
  int max_len = 0, calls = 0;
  size_t read_bytes = 0; // what the continuation loop read on the host: n_states and ok of every open segment of every extend call
  bool has_scene = false;
  void *block = nullptr; // one allocation; the arrays below point into it
  double *d_rows = nullptr, *arc = nullptr, *length = nullptr, *clearance = nullptr, *min_clear = nullptr;
  int32_t *path_first = nullptr, *seg_first = nullptr, *seg_newton = nullptr, *min_row = nullptr, *first_blocked = nullptr;
  uint8_t *seg_ok = nullptr;
};

#pragma GCC visibility push(hidden)
namespace ccmp_host {

/* Where the endpoints of a tile of pair tests come from: the enumeration of a batch of paths (shortcut_enumerate_kernel: path_joints,
 * path_len and the prefix over paths on the device; a slot's matrix entry from the kernel) or explicit rows from / to [total][14] on the
 * device (slot g's entry is g). */
struct PairSource {
  const double *path_joints = nullptr;
  const int32_t *path_len = nullptr;
  const long long *d_prefix = nullptr;
  size_t F = 0;
  int max_len = 0, max_span = 0;
  const double *from = nullptr, *to = nullptr;
};

struct PairLoopOpts {
  int chunk_states, round_budget, max_calls, tile_edges;
};

/* what a loop did, added to: extend calls made, bytes read on the host */
struct PairLoopCounts {
  long long calls = 0, read_bytes = 0;
};

/* what every entry point that traverses checks first of all, in this order (problem_ok can answer more than CCMP_EINVAL): its problem,
 * its options — opts_rc = what the unit's own opts_ok answered — and its scene */
inline int traversal_checks(const ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, int opts_rc)
{
  { const int rc = problem_ok(p); if (rc != CCMP_OK) return rc; }
  if (!(p->delta > 0) || !(p->lambda > 0)) return CCMP_EINVAL;
  if (opts_rc != CCMP_OK) return opts_rc;
  if (scene && (scene->device != ctx->device || std::isnan(margin))) return CCMP_EINVAL;
  return CCMP_OK;
}

/* `total` pair slots in tiles of at most tile_edges, each tile continued until no pair is open: ONE uninterrupted checkMotion per pair
 * (ccmp_geodesic_batch_ex, with a scene ccmp_geodesic_scene_batch), its flag, list length and Newton total into w_ok / w_states /
 * w_newton [cells] (the last two nullable) at the slot's entry.  Synchronous; CCMP_EOVERFLOW when max_calls extend calls are spent on a
 * tile with a pair open.  The buffers come from `mem`; `what` names the entry point in an error text; counts (nullable) is added to. */
int pair_tests(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const PairLoopOpts &o, long long total, const PairSource &src,
               size_t cells, uint8_t *w_ok, int32_t *w_states, int32_t *w_newton, CallArena &mem, hipStream_t st, const char *what,
               PairLoopCounts *counts = nullptr);

/* ccmp_path_densify behind its checks on device rows: `len` = the path lengths on the host.  On any failure *out stays NULL. */
int densify_rows(ccmp_ctx *ctx, const ccmp_problem *p, const ccmp_scene *scene, double margin, const double *path_joints, const std::vector<int32_t> &len,
                 size_t F, int max_len, const ccmp_dense_opts &o, ccmp_dense_paths **out, hipStream_t st);

}  // namespace ccmp_host
#pragma GCC visibility pop

#endif /* CCMP_PAIR_TESTS_H */
