/* ccmp_debug.h — test and tool hooks of libccmp.  NOT part of the product ABI.
 *
 * The default library (lib/libccmp.so) exports none of these symbols and does not know the options named here; the same sources
 * built with -DCCMP_DEBUG_HOOKS (closed_chain_motion_planner_amd/build.py links them as lib/libccmp_debug.so beside the default
 * library — every kernel object is shared, only ccmp_api.cpp and ccmp_policy.cpp are compiled twice) do.  The GPU suite runs the
 * tests that need a hook in processes of their own against the debug library (tests/test_gpu_debug_hooks.py, test_gpu_scout_slices.py,
 * test_gpu_scout_sort.py); tools/ that read the scout's predictions select it through CCMP_LIBRARY.
 *
 * The reference has no counterpart for any of this (no tracing, no fault injection). */
#ifndef CCMP_DEBUG_H
#define CCMP_DEBUG_H
#include "ccmp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* runs ccmp_detmath.h's sincos / atan2 / sqrt / div on the device: out[i] = {sin, cos, atan2_nn(|x|, |y|), sqrt(|x|), x / y} —
 * how the tests prove the device arithmetic bit-identical to the host's */
int ccmp_detmath_probe(ccmp_ctx *ctx, const double *x_dev, const double *y_dev, double *out_dev, size_t n, void *hip_stream);
/* the quotient n / d three ways on the device: out[i] = {ccmp_div_steps (the lean sequence, forced), ccmp_div_lean (wave-uniform
 * choice), the compiler's n / d} — the lean sequence must equal n / d wherever both operands are in 2^-300 <= |v| < 2^300, and
 * ccmp_div_lean everywhere */
int ccmp_detmath_div_probe(ccmp_ctx *ctx, const double *n_dev, const double *d_dev, double *out_dev, size_t count, void *hip_stream);
/* the forms an in-range Newton round of the throughput kernels runs, beside the forms they stand in for, one wavefront per 64 inputs
 * (n a multiple of 64; anything else is refused with CCMP_EINVAL): m_dev[n][9] row-major matrices, y_dev[n] angles, store_dev[n] flags.
 * out_dev[i][13] = {quat_of_t<true> (x, y, z, w), quat_of (x, y, z, w), ccmp_sincos_inr (sin, cos), ccmp_sincos (sin, cos), the path
 * lane i's wavefront took through the quaternion, written by quat_of_t<true> itself inside the branch it took: case 0..3 (one case
 * body behind the scalar branch) or 4 (the branch-free text)}; where store_dev[i] == 0 the lane computes on its input all the same and row i is left untouched */
int ccmp_detmath_round_facts_probe(ccmp_ctx *ctx, const double *m_dev, const double *y_dev, const unsigned char *store_dev, double *out_dev, size_t n,
                                   void *hip_stream);
/* an externally supplied processing order for the reference-arithmetic projector (device array of B sample indices, NULL = none) */
int ccmp_ctx_set_order_experimental(ccmp_ctx *ctx, const unsigned int *order_dev);
/* a copy of the FP32 scout's predicted iteration counts of the last call that ran one */
int ccmp_ctx_debug_lpt_pred(ccmp_ctx *ctx, uint16_t *host_out, size_t B);
/* beside it: the processing order the counting sort made of those predictions (order_host[n]), the sort's histogram (hist_host[1024]: at k
 * the number of keys >= k) and the context's queue words (queue_host[queue_words]; queue_words must be the library's count, 83) as the
 * last call left them */
int ccmp_ctx_debug_lpt_order(ccmp_ctx *ctx, unsigned int *order_host, size_t n, unsigned int *hist_host, unsigned long long *queue_host,
                             size_t queue_words);
/* the first n rows of the workspace between the head and the resume launch of a large reference-arithmetic projector batch on stock twin
 * arms (calibrated arms leave the shorter hand-over record: not this layout), as the last such call left them: row i = sample i, row_doubles doubles each (the library's count, returned in *row_doubles_out: ccmp_launch.h, kStagedRow) —
 * the first 150 of a row what the head's last function(x) left in the group's record (x 14, sin / cos 28, arm 0's frames 84, tool poses 24),
 * then f0, f1, the index as a 64-bit integer (-1: the head has written the sample back), (iter | updates << 32), norm1, norm2, and 1.0 where some
 * joint of x failed rot_x0_round_ok in that evaluation, else 0.0; one pad.  rows_host NULL: the count alone */
int ccmp_ctx_debug_fd_state(ccmp_ctx *ctx, double *rows_host, size_t n, int *row_doubles_out);
/* the scouts' descending counting sort on the caller's device buffers: keys_dev[n] (uint16, clamped to 1023) -> order_dev[n], hist_dev[1024],
 * and — kind 1 or 2 — the cut of the order into queue_dev (a block of 16 64-bit words: 0, 3, 4 = the front's length, the other words
 * below `clear` zeroed, the rest untouched).  Above 16 384 keys (the three-kernel form) every key must be below nbins, the histogram runs on
 * hist_blocks blocks, and clear_first != 0 clears hist_dev first as the library's callers do (0: it must hold zeros already); at or
 * below, one launch that ignores all three.  What would make a kernel leave the buffers is refused with CCMP_EINVAL.  kind 1: the keys >= p_low, at most limit; kind 2: >= p_high where those carry permille / 1000 of the sum of the keys, else
 * >= p_low; kind 0: no cut, queue_dev is not touched */
int ccmp_debug_sort_probe(ccmp_ctx *ctx, const uint16_t *keys_dev, size_t n, int nbins, int hist_blocks, int clear_first, unsigned int *order_dev,
                          unsigned int *hist_dev, unsigned long long *queue_dev, int kind, int p_low, int p_high, int permille, unsigned int limit,
                          int clear, void *hip_stream);
/* the two stand-alone cut kernels on a caller-supplied histogram hist_dev[1024] (at k: keys >= k); they write words 0, 3 and 4 of queue_dev.
 * kernel 1: the keys >= p_min, at most limit; kernel 2: the largest cut P in (p_min, p_max] whose front carries permille / 1000 of the sum
 * of the keys, else p_min */
int ccmp_debug_split_probe(ccmp_ctx *ctx, int kernel, const unsigned int *hist_dev, int p_min, int p_max, int permille, unsigned int limit,
                           unsigned long long *queue_dev, void *hip_stream);
/* fault injection: the next n compute entry points of this context return CCMP_EHIP before anything is launched */
int ccmp_debug_fail_calls(ccmp_ctx *ctx, int n);
/* option "fail_after_fork" (ccmp_ctx_set_option; listed by ccmp_ctx_option_info of the debug library only): 1 / 2 = the split
 * launches of the projector and of the extend step's bulk form report a failure in front of / behind their side-stream part */

#ifdef __cplusplus
}
#endif
#endif /* CCMP_DEBUG_H */
