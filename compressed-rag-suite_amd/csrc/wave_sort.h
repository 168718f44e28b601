// wave_sort.h -- one value per lane, sorted across a wave64 with shuffles (merge.hip, finish.hip: the k-th largest
// "bucket maximum" of a workgroup).
#pragma once
#include <hip/hip_runtime.h>

namespace crs {
namespace {

// full bitonic sort (descending by lane) of one value per lane across a wave64
__device__ __forceinline__ float wave_sort_desc(float v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const float o = __shfl_xor(v, j);
      const bool lower = (lane & j) == 0;
      const bool desc = (lane & k) == 0;       // k == 64: always descending
      const bool want_max = (lower == desc);
      v = want_max ? fmaxf(v, o) : fminf(v, o);
    }
  }
  return v;
}
// v is a bitonic sequence across the wave -> sorted descending
__device__ __forceinline__ float wave_clean_desc(float v, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const float o = __shfl_xor(v, j);
    v = ((lane & j) == 0) ? fmaxf(v, o) : fminf(v, o);
  }
  return v;
}

}  // namespace
}  // namespace crs
