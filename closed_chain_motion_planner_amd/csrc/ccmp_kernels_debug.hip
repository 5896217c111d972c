// ccmp_kernels_debug.hip — device side of include/ccmp_debug.h; linked into lib/libccmp_debug.so only.
// Built in the canonical rounding model with the throughput kernel's elementary functions (-DCCMP_LEAN_SQRT included): what the
// probe reports is what project_fd_kernel computes with.
#include <hip/hip_runtime.h>

#include "ccmp_detmath.h"
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

} // namespace

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
