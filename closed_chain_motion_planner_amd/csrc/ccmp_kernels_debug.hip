// ccmp_kernels_debug.hip — device side of include/ccmp_debug.h; linked into lib/libccmp_debug.so only.
// Built in the canonical rounding model with the throughput kernel's elementary functions (-DCCMP_LEAN_SQRT included): what the
// probe reports is what project_fd_kernel computes with.
#include <hip/hip_runtime.h>

#include "ccmp_kin.h"
#include "ccmp_launch.h"

namespace {

__global__ void detmath_probe_kernel(const double *__restrict__ x, const double *__restrict__ y, double *__restrict__ out, size_t n)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double s, c;
  ccmp_sincos(x[i], &s, &c);
  out[5 * i + 0] = s;
  out[5 * i + 1] = c;
  out[5 * i + 2] = ccmp_atan2_nn(ccmp_abs(x[i]), ccmp_abs(y[i]));
  out[5 * i + 3] = ccmp_sqrt(ccmp_abs(x[i]));
  out[5 * i + 4] = x[i] / y[i];
}

// ccmp_div_lean's two paths (the unit is built with -DCCMP_LEAN_DIV): the lean sequence forced on every lane, the wave-uniform
// choice, and the compiler's division
__global__ void div_probe_kernel(const double *__restrict__ num, const double *__restrict__ den, double *__restrict__ out, size_t n)
{
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[3 * i + 0] = ccmp_div_steps(num[i], den[i]);
  out[3 * i + 1] = ccmp_div_lean(num[i], den[i]);
  out[3 * i + 2] = num[i] / den[i];
}

// The forms an in-range round of the throughput kernels runs (ccmp_kin.h: quat_of_t<true>, ccmp_detmath.h: ccmp_sincos_inr)
// beside the forms they stand in for, one matrix (9 doubles) and one angle per lane, one wavefront per block so that a block of 64
// inputs is exactly what one wavefront's case test sees.  out[i] = {quat_of_t<true> (4), quat_of (4), ccmp_sincos_inr (2),
// ccmp_sincos (2), the path the wavefront took AS quat_of_t REPORTS IT from inside its branch: case 0..3, or 4 for the branch-free text}; a lane with store[i] == 0
// computes on whatever it was given — NaN, garbage — and writes nothing, as a lane without a live sample does in the kernels.
__global__ __launch_bounds__(64) void round_facts_probe_kernel(const double *__restrict__ m, const double *__restrict__ y,
                                                               const unsigned char *__restrict__ store, double *__restrict__ out)
{
  const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
  double a[9], qt[4], qf[4], s1, c1, s0, c0;
#pragma unroll
  for (int k = 0; k < 9; k++) a[k] = m[9 * i + k];
  int path = -1; // reported by quat_of_t itself, from inside the branch it took
  ccmp::quat_of_t<true>(a, qt, &path);
  ccmp::quat_of(a, qf);
  ccmp_sincos_inr(y[i], &s1, &c1);
  ccmp_sincos(y[i], &s0, &c0);
  if (store[i]) {
    double *o = out + 13 * i;
#pragma unroll
    for (int k = 0; k < 4; k++) { o[k] = qt[k]; o[4 + k] = qf[k]; }
    o[8] = s1; o[9] = c1; o[10] = s0; o[11] = c0;
    o[12] = (double)path;
  }
}

} // namespace

hipError_t ccmp_launch::round_facts_probe(const double *m, const double *y, const unsigned char *store, double *out, size_t n, hipStream_t st)
{
  if (n == 0 || n % 64 != 0) return hipErrorInvalidValue; // whole wavefronts only: every lane of a block reads its own input
  hipLaunchKernelGGL(round_facts_probe_kernel, dim3((unsigned)(n / 64)), dim3(64), 0, st, m, y, store, out);
  return hipGetLastError();
}

hipError_t ccmp_launch::detmath_probe(const double *x, const double *y, double *out, size_t n, hipStream_t st)
{
  hipLaunchKernelGGL(detmath_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, x, y, out, n);
  return hipGetLastError();
}

hipError_t ccmp_launch::div_probe(const double *num, const double *den, double *out, size_t n, hipStream_t st)
{
  hipLaunchKernelGGL(div_probe_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, num, den, out, n);
  return hipGetLastError();
}
