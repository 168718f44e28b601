// cert_eps.h -- the per-query error bound eps_q of the exactness certificate (derivation: exact.hip), shared by
// refine_cert_kernel (exact.hip) and large_cert_kernel (large_k.hip) so that both certify against the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "dot_f32.h"

namespace crs {
namespace {

__device__ __forceinline__ float wmax(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}

// Called by the first 256 threads (t = 0..255) of a workgroup: |q16 - q|^2, |q|^2 and max |q16| over the padded row
// (elements past dim: q = 0), one partial per wave into red[wave].  The caller synchronises before cert_query_eps.
__device__ __forceinline__ void cert_query_partials(const float* __restrict__ a, const _Float16* __restrict__ a16, int dim, int pdim, int t,
                                                    float (*red)[3]) {
  const int lane = t & 63, wave = t >> 6;
  float d2 = 0.f, n2 = 0.f, am = 0.f;
  for (int e = t; e < pdim; e += 256) {
    const float x = e < dim ? a[e] : 0.f, h = (float)a16[e];
    d2 = fmaf(h - x, h - x, d2);
    n2 = fmaf(x, x, n2);
    am = fmaxf(am, fabsf(h));
  }
  d2 = wsum(d2); n2 = wsum(n2); am = wmax(am);
  if (lane == 0) { red[wave][0] = d2; red[wave][1] = n2; red[wave][2] = am; }
}

// eps_q = dq (1 + E) + |q| E + arith from the four partials (dq: + the 16-bit fixed-point query term on int8 slabs)
__device__ __forceinline__ float cert_query_eps(const float (*red)[3], int pdim, int is_i8, float err_rows, float err_arith) {
  const float dd = red[0][0] + red[1][0] + red[2][0] + red[3][0];
  const float nn = red[0][1] + red[1][1] + red[2][1] + red[3][1];
  const float mx = fmaxf(fmaxf(red[0][2], red[1][2]), fmaxf(red[2][2], red[3][2]));
  float dq = sqrtf(dd) * 1.0001f;
  if (is_i8) dq += sqrtf((float)pdim) * mx * (1.0001f / 65024.0f);
  return dq * (1.0f + err_rows) * 1.0001f + sqrtf(nn) * err_rows * 1.0002f + err_arith;
}

}  // namespace
}  // namespace crs
