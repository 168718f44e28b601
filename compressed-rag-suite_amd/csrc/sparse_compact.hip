// sparse_compact.hip -- a dense [batch, Vp] row of non-negative weights to a bounded sparse row (gfx950): crs_sparse_compact
// (DESIGN 3.16).
//
// Per text: the ids whose weight is > 0 (a NaN or a negative zero is not), minus the skip list; when more than `cap` remain, the cap
// largest weights, ties at the threshold by lower id; emitted in ascending id order as (ids int32, weights fp32), the unused slots
// filled with (-1, 0), and the number kept in counts[b].  Exact and deterministic: no floating-point arithmetic at all -- a
// positive float orders as its bit pattern, so the threshold is found by building the cap-th largest pattern bit by bit (31
// counting passes), and the emission is a stable prefix count.
//
// One workgroup of 1024 threads per text.  A row of V <= kStageMaxV fp32 (30522: 119 KB) is staged once into LDS, with skipped and
// non-positive entries already zeroed, and every pass reads LDS; a longer row is re-read from global memory (it stays in L2).  No
// scratch, no atomics, no host synchronisation.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"

namespace crs {
namespace {

constexpr int kCpThreads = 1024;
constexpr int kCpWaves = kCpThreads / 64;
constexpr int kStageMaxV = 38912;              // 152 KB of the CU's 160 KB of LDS
static_assert(kStageMaxV * 4 + 1024 <= 160 * 1024, "the staged row and the small arrays fit one CU's LDS");

// the pattern an id competes with: 0 = not a term
__device__ __forceinline__ unsigned cp_bits(float w, int v, const int* skip, int n_skip) {
  if (!(w > 0.0f)) return 0u;
  for (int i = 0; i < n_skip; ++i)
    if (skip[i] == v) return 0u;
  return __float_as_uint(w);
}

// sum of `x` over the workgroup, the same in every thread; red is kCpWaves ints of LDS
__device__ __forceinline__ int cp_block_sum(int x, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                                     // the previous sum has been read
  if ((threadIdx.x & 63) == 0) red[wave] = x;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int w = 0; w < kCpWaves; ++w) s += red[w];
  return s;
}

template <bool kStaged>
__global__ __launch_bounds__(kCpThreads) void sparse_compact_kernel(const float* __restrict__ weights, int V, int Vp, int cap,
                                                                   const int* __restrict__ skip_ids, int n_skip, int* __restrict__ out_ids,
                                                                   float* __restrict__ out_w, int* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char cp_smem[];
  unsigned* srow = reinterpret_cast<unsigned*>(cp_smem);     // [V] when staged
  __shared__ int red[kCpWaves];
  __shared__ int red_gt[kCpWaves], red_eq[kCpWaves];
  __shared__ int skip[CRS_SPARSE_MAX_SKIP];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const float* wrow = weights + (size_t)b * Vp;
  if (tid < n_skip) skip[tid] = skip_ids[tid];
  __syncthreads();
  if (kStaged) {
    for (int v = tid; v < V; v += kCpThreads) srow[v] = cp_bits(wrow[v], v, skip, n_skip);
    __syncthreads();
  }
  auto bits = [&](int v) -> unsigned { return kStaged ? srow[v] : cp_bits(wrow[v], v, skip, n_skip); };

  int c = 0;
  for (int v = tid; v < V; v += kCpThreads) c += bits(v) != 0u;
  const int n_pos = cp_block_sum(c, red);

  // thr: keep every pattern > thr, and the first `tie_keep` ids whose pattern == thr
  unsigned thr = 0u;
  int tie_keep = 0;
  if (n_pos > cap) {                                   // (uniform) thr = the cap-th largest pattern
    for (int bit = 30; bit >= 0; --bit) {
      const unsigned cand = thr | (1u << bit);
      c = 0;
      for (int v = tid; v < V; v += kCpThreads) c += bits(v) >= cand;
      if (cp_block_sum(c, red) >= cap) thr = cand;
    }
    c = 0;
    for (int v = tid; v < V; v += kCpThreads) c += bits(v) > thr;
    tie_keep = cap - cp_block_sum(c, red);
  }

  // ---- emission in ascending id: slot = (ids before with pattern > thr) + min(ids before with pattern == thr, tie_keep)
  int base_gt = 0, base_eq = 0;
  int* oi = out_ids + (size_t)b * cap;
  float* ow = out_w + (size_t)b * cap;
  for (int v0 = 0; v0 < V; v0 += kCpThreads) {
    const int v = v0 + tid;
    const unsigned x = v < V ? bits(v) : 0u;
    const bool gt = x > thr, eq = tie_keep > 0 && x == thr;
    const unsigned long long m_gt = __ballot(gt), m_eq = __ballot(eq);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    __syncthreads();                                   // the previous chunk's totals have been read
    if (lane == 0) { red_gt[wave] = __popcll(m_gt); red_eq[wave] = __popcll(m_eq); }
    __syncthreads();
    int n_gt = base_gt + __popcll(m_gt & below), n_eq = base_eq + __popcll(m_eq & below);
    int tot_gt = 0, tot_eq = 0;
#pragma unroll
    for (int w = 0; w < kCpWaves; ++w) {
      if (w < wave) { n_gt += red_gt[w]; n_eq += red_eq[w]; }
      tot_gt += red_gt[w]; tot_eq += red_eq[w];
    }
    if (gt || (eq && n_eq < tie_keep)) {
      const int slot = n_gt + (n_eq < tie_keep ? n_eq : tie_keep);
      if (slot < cap) { oi[slot] = v; ow[slot] = __uint_as_float(x); }     // (slot < cap by construction)
    }
    base_gt += tot_gt; base_eq += tot_eq;
  }
  const int kept = n_pos > cap ? cap : n_pos;
  for (int i = kept + tid; i < cap; i += kCpThreads) { oi[i] = -1; ow[i] = 0.0f; }
  if (tid == 0) counts[b] = kept;
}

}  // namespace

int sparse_compact_launch(const float* weights, int batch, int V, int Vp, int cap, const int* skip_ids, int n_skip, int* out_ids,
                          float* out_w, int* counts, hipStream_t stream) {
  if (V <= kStageMaxV) {
    const size_t lds = (size_t)V * 4;
    if (lds > 48 * 1024) {
      const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(&sparse_compact_kernel<true>),
                                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (ae != hipSuccess) return (int)ae;
    }
    hipLaunchKernelGGL(sparse_compact_kernel<true>, dim3((unsigned)batch), dim3(kCpThreads), lds, stream, weights, V, Vp, cap, skip_ids,
                       n_skip, out_ids, out_w, counts);
  } else {
    hipLaunchKernelGGL(sparse_compact_kernel<false>, dim3((unsigned)batch), dim3(kCpThreads), 0, stream, weights, V, Vp, cap, skip_ids,
                       n_skip, out_ids, out_w, counts);
  }
  return (int)hipGetLastError();
}

}  // namespace crs
