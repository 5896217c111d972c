// ccmp_kernels_geo_scene.hip — the extend step with the StateValidityChecker's proxy pre-filter on the device, reference arithmetic
// (ccmp_geodesic_scene_batch in FD mode): geodesic_flat_kernel's edge body (ccmp_geo_edge_body.inc with CCMP_GEO_SCENE) on the
// latency kernels' Newton routine, with the clearance of ccmp_clearance.h between the projection and the step test.  Built with the
// latency flavour's flags (build.py: 256-register budget, no scratch) in a unit of its own, so that the existing extend-step
// objects compile to what they compiled to before.
#include "ccmp_flat_newton.h"
#include "ccmp_geo_edge.h"
#include "ccmp_clearance.h"

namespace {

// geodesic_scene_kernel — the same traversal with the StateValidityChecker's proxy pre-filter on the device
// (ccmp_geodesic_scene_batch): the reference's loop with interpolate == false, where svc->isValid(scratch) is "the scene's
// clearance of scratch > margin" (ccmp_clearance.h, computed by the block's 128 threads between the projection and the step
// test).  A refused state ends the edge with blocked = 1; the list holds the states before it.  Persistent blocks, first
// ticket = own index, the rest from the queue word; no bulk form, no pool.
template <bool STOCK>
__global__ __launch_bounds__(128, CCMP_FLAT_MIN_WAVES) void geodesic_scene_kernel(
    const ccmp_consts K, const double delta, const double lambda, const double *__restrict__ from,
    const double *__restrict__ to, unsigned long long E, int max_states, double *__restrict__ states,
    int *__restrict__ n_states, uint8_t *__restrict__ ok_out, int *__restrict__ newton_iters, int check_target,
    unsigned long long *queue, const double *__restrict__ carry_in, double *__restrict__ carry_out, int round_budget,
    const scene_dev *__restrict__ scene, const double margin, uint8_t *__restrict__ blocked_out, double *__restrict__ clearance_out)
{
  __shared__ __attribute__((aligned(16))) double lds[gRec];
  __shared__ double ktab[kConstsDoubles + 1];
  __shared__ __attribute__((aligned(16))) double steptab[kStepTab];
  __shared__ double clr_ws[kClrFrames + kClrCentres + 2]; // frames, centres, two partial minima
  __shared__ unsigned long long ticket;
  const int tid = threadIdx.x, lane = tid & 63;
  {
    const double *src = reinterpret_cast<const double *>(&K);
    for (int k = tid; k < kConstsDoubles; k += 128) ktab[k] = src[k];
  }
  stage_step_table(K, steptab, tid);
  __syncthreads();
  const ccmp_consts &KL = *reinterpret_cast<const ccmp_consts *>(ktab);
  double *rec = lds;
  const double pi = 3.14159265358979323846;
  const double *const ent = nullptr; // never a hand-over
  unsigned long long t = blockIdx.x;
  for (bool first = true;; first = false) {
    if (!first) {
      if (tid == 0) ticket = (unsigned long long)gridDim.x + atomicAdd(queue, 1ull);
      __syncthreads();
      t = ticket;
    }
    if (t >= E) break;
#define CCMP_GEO_SCENE
#include "ccmp_geo_edge_body.inc"
#undef CCMP_GEO_SCENE
  }
}

} // namespace

namespace ccmp_launch {

// the scene variant: `blocks` persistent blocks on the ticket word `queue` (cleared here by a kernel, so that a capture replays it)
hipError_t geodesic_scene(const GeoCall &g, const GeoScene &s, int blocks, unsigned long long *queue, hipStream_t st)
{
  if (blocks <= 0) return hipErrorInvalidValue;
  hipError_t e = clear_words(queue, 2, st);
  if (e != hipSuccess) return e;
#define CCMP_LAUNCH_GEO_SCENE(STOCK)                                                                                                  \
  hipLaunchKernelGGL(geodesic_scene_kernel<STOCK>, dim3(blocks), dim3(128), 0, st, *g.K, g.delta, g.lambda, g.from, g.to, (unsigned long long)g.E, \
                     g.max_states, g.states, g.n_states, g.ok, g.newton_iters, g.check_target, queue, g.carry_in, g.carry_out, g.round_budget,  \
                     s.scene, s.margin, s.blocked, s.clearance)
  if (g.K->stock) CCMP_LAUNCH_GEO_SCENE(true);
  else CCMP_LAUNCH_GEO_SCENE(false);
#undef CCMP_LAUNCH_GEO_SCENE
  return hipGetLastError();
}

}  // namespace ccmp_launch
