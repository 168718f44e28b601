// dot_f32.h -- the fp32 candidate scoring of the exactness certificate (exact.hip) and of the fused search tail (finish.hip).
// One definition, so that a candidate's fp32 score does not depend on which kernel scored it.
#pragma once
#include <hip/hip_runtime.h>

namespace crs {
namespace {

__device__ __forceinline__ float wsum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// up to four rows at once (loads of all rows in flight together: one HBM round trip instead of four); per row the
// identical FMA order as a single-row lane-strided FMA chain + butterfly (crs_refine_f32, convert.hip)
__device__ __forceinline__ void dot4_f32(const float* __restrict__ a, const float* const* __restrict__ rows, int n, int dim, int lane,
                                         float* __restrict__ out) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e = lane; e < dim; e += 64) {
    const float x = a[e];
    float y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) y[u] = (u < n) ? rows[u][e] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(x, y[u], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) out[u] = wsum(acc[u]);
}

}  // namespace
}  // namespace crs
