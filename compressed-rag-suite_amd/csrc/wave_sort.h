// wave_sort.h -- one wave sorts 64 E 64-bit keys held E per lane; shared by the kernels that select in the sweep with
// (ordered score << 32 | ~row) keys (scan_mxfp4.hip, ivf_probe.hip).  Header-only, anonymous namespace of the including unit.
#pragma once
#include <hip/hip_runtime.h>

namespace crs {
namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 umax64(u64 a, u64 b) { return a > b ? a : b; }
__device__ __forceinline__ u64 umin64(u64 a, u64 b) { return a < b ? a : b; }

// element e = lane + 64 u of 64 E keys -> descending
template <int E>
__device__ __forceinline__ void wave_sort_keys(u64 (&key)[E], int lane) {
#pragma unroll
  for (int k = 2; k <= 64 * E; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (j >= 64) {
#pragma unroll
        for (int u = 0; u < E; ++u) {
          const int u2 = u ^ (j >> 6);
          if (u2 > u) {
            const bool desc = ((64 * u) & k) == 0;      // lane < 64 <= j < k: the lane bits do not reach k
            const u64 hi = umax64(key[u], key[u2]), lo = umin64(key[u], key[u2]);
            key[u] = desc ? hi : lo;
            key[u2] = desc ? lo : hi;
          }
        }
      } else {
#pragma unroll
        for (int u = 0; u < E; ++u) {
          const int e = lane + 64 * u;
          const u64 other = __shfl_xor(key[u], j);
          const bool keep_max = ((e & j) == 0) == ((e & k) == 0);
          key[u] = keep_max ? umax64(key[u], other) : umin64(key[u], other);
        }
      }
    }
  }
}

// orders a wave's own LDS writes before its own LDS reads (the lanes of a wave run in lockstep, the compiler must not reorder)
__device__ __forceinline__ void lds_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace
}  // namespace crs
