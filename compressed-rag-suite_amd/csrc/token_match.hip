// token_match.hip -- BERTScore's greedy token matching on the device (gfx950): crs_token_match.
//
// The step behind the encoder in the reference's answer-quality metric (evaluation/retrieval/rag_metrics.py:179-207 calls
// bert_score.score): for a pair (candidate a, reference b) of token-state matrices, with x^ = x / |x|,
//     sim[i][j] = <a^_i, b^_j>                              i < len_a, j < len_b
//     P = sum_i w_a[i] max_j sim[i][j] / sum_i w_a[i]       R = sum_j w_b[j] max_i sim[i][j] / sum_j w_b[j]       F = 2PR / (P + R)
// One 256-thread workgroup per pair, one launch for all pairs, four phases:
//
//   1. Inverse norms.  A quarter wave per token row: fp32 sum of squares (fmaf per lane, xor butterfly over 16 lanes), 1 / sqrt into LDS;
//      0 for a zero row (its cosines are 0, never NaN, as in mmr.hip) and for every row at or past the length.
//   2. sim in 64 x 64 tiles with __builtin_amdgcn_mfma_f32_16x16x4f32 (gfx950 has no xf32; the f32-input MFMA is an exact fmaf chain
//      in k order).  K is staged through LDS in chunks of 64 columns, 64 rows of a and 64 of b, row pitch 68 floats: the 16 rows of a
//      quarter wave's 16-byte read fall in 16 distinct 16-byte slots.  Wave w owns rows 16 w .. 16 w + 15 of the tile and all 64
//      columns: four independent accumulators, which is what the 16x16x4 form needs to reach its issue rate.  A lane reads 4
//      consecutive k of its row at once and feeds them to 4 MFMAs, so MFMA t of a 16-column group sums k = 4 g + t, g = 0..3: a fixed
//      permutation of k, the same for a and b.  Rows at or past the length are staged as zeros -- padding is never loaded.
//      The (tile, chunk) steps form one flat walk and the global loads of the next step are issued ahead of a step's MFMAs.
//   3. Maxima.  acc * inv_a[i] * inv_b[j]; entries outside len_a x len_b become -inf.  Row maxima: over the lane's 4 column groups,
//      then an xor butterfly over the 16 lanes of a row; the wave owns its rows of the running array.  Column maxima: over the
//      lane's 4 rows and the 4 quarter waves, then the four waves' partial rows meet in LDS (no float atomics).
//   4. Weighted means.  Wave 0 forms P, wave 1 forms R: lane l adds tokens l, l + 64, ... in order, then an xor butterfly -- a fixed
//      order whatever the launch holds.  A weight sum that is not positive gives 0; F is 0 when P + R is 0 or not finite.
//
// A pair reads only its own rows below its lengths, and nothing in its arithmetic depends on seq_a / seq_b, n_pairs or blockIdx
// beyond addressing: its three numbers are bitwise independent of the launch it shares.  No scratch, no atomics, no workgroup
// depends on another.  LDS: 2 x 64 x 68 floats of staging + 4 x 512 of norms and maxima + 4 x 64 partials = 44 KB.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"

namespace crs {
namespace {

typedef float tm_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int kMaxSeq = 512;
constexpr int kTile = 64;            // rows of a / rows of b per tile
constexpr int kKC = 64;              // columns per staged chunk
constexpr int kPitch = kKC + 4;      // floats per staged row: 272 bytes, a multiple of 16 that is no multiple of 256

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// rows [r0, r0 + 64) x columns [c0, c0 + 64) of x -> sh[row][0, 64); rows at or past len are zeros and are not read
__device__ __forceinline__ void stage_load(const float* __restrict__ x, int hidden, int len, int r0, int c0, int tid, tm_f32x4 (&v)[4]) {
  const int c4 = tid & 15;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int r = r0 + (tid >> 4) + 16 * u;
    v[u] = tm_f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < len) v[u] = *reinterpret_cast<const tm_f32x4*>(x + (size_t)r * hidden + c0 + 4 * c4);
  }
}
__device__ __forceinline__ void stage_store(float* sh, int tid, const tm_f32x4 (&v)[4]) {
  const int c4 = tid & 15;
#pragma unroll
  for (int u = 0; u < 4; ++u) *reinterpret_cast<tm_f32x4*>(sh + ((tid >> 4) + 16 * u) * kPitch + 4 * c4) = v[u];
}

// acc[v] += the staged chunk's part of sim for the lane's row and column groups v < NV; xa / xb: the lane's row of the a tile and
// of column group 0 of the b tile, at its k offset 4 g
template <int NV>
__device__ __forceinline__ void mfma_chunk(const float* xa, const float* xb, tm_f32x4 (&acc)[4]) {
#pragma unroll
  for (int kk = 0; kk < kKC; kk += 16) {
    const tm_f32x4 fa = *reinterpret_cast<const tm_f32x4*>(xa + kk);
    tm_f32x4 fb[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) fb[v] = *reinterpret_cast<const tm_f32x4*>(xb + v * 16 * kPitch + kk);
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int v = 0; v < NV; ++v) acc[v] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[t], fb[v][t], acc[v], 0, 0, 0);
  }
}

// wave `row`'s tokens: weighted mean of best[0, len) in a fixed order
__device__ __forceinline__ float weighted_mean(const float* best, const float* __restrict__ w, int len, int lane) {
  float num = 0.f, den = 0.f;
  for (int i = lane; i < len; i += 64) {
    const float wi = w ? w[i] : 1.f;
    num = fmaf(wi, best[i], num);
    den += wi;
  }
  num = wave_sum(num);
  den = wave_sum(den);
  return den > 0.f ? num / den : 0.f;
}

__global__ __launch_bounds__(kThreads) void token_match_kernel(const float* __restrict__ a, const int* __restrict__ len_a, int seq_a,
                                                              const float* __restrict__ b, const int* __restrict__ len_b, int seq_b,
                                                              int hidden, const float* __restrict__ w_a,
                                                              const float* __restrict__ w_b, float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float sh_a[kTile * kPitch];
  __shared__ __attribute__((aligned(16))) float sh_b[kTile * kPitch];
  __shared__ float sh_inva[kMaxSeq], sh_invb[kMaxSeq];
  __shared__ float sh_rowmax[kMaxSeq], sh_colmax[kMaxSeq];
  __shared__ float sh_cpart[4][kTile];
  __shared__ float sh_pr[2];

  const int p = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int la = len_a[p], lb = len_b[p];
  la = la < 0 ? 0 : (la > seq_a ? seq_a : la);
  lb = lb < 0 ? 0 : (lb > seq_b ? seq_b : lb);
  la = __builtin_amdgcn_readfirstlane(la);
  lb = __builtin_amdgcn_readfirstlane(lb);
  float* o = out + (size_t)p * 3;
  if (la == 0 || lb == 0) {             // an empty sentence: P = R = F = 0
    if (tid < 3) o[tid] = 0.f;
    return;
  }
  const float* pa = a + (size_t)p * seq_a * hidden;
  const float* pb = b + (size_t)p * seq_b * hidden;
  const float ninf = -__builtin_huge_valf();

  // ---- 1. inverse norms ----
  for (int i = tid; i < kMaxSeq; i += kThreads) {
    sh_rowmax[i] = ninf;
    sh_colmax[i] = ninf;
    if (i >= la) sh_inva[i] = 0.f;
    if (i >= lb) sh_invb[i] = 0.f;
  }
  const int h4 = hidden >> 2;
  for (int r = wave * 4 + (lane >> 4); r < la + lb; r += 16) {      // a quarter wave per row: 16 rows in flight per workgroup
    const float* src = r < la ? pa + (size_t)r * hidden : pb + (size_t)(r - la) * hidden;
    float s = 0.f;
#pragma unroll 4
    for (int c = lane & 15; c < h4; c += 16) {
      const tm_f32x4 v = *reinterpret_cast<const tm_f32x4*>(src + 4 * c);
      s = fmaf(v.x, v.x, s);
      s = fmaf(v.y, v.y, s);
      s = fmaf(v.z, v.z, s);
      s = fmaf(v.w, v.w, s);
    }
#pragma unroll
    for (int o2 = 8; o2 > 0; o2 >>= 1) s += __shfl_xor(s, o2);
    const float inv = s > 0.f ? 1.f / sqrtf(s) : 0.f;
    if ((lane & 15) == 0) {
      if (r < la) sh_inva[r] = inv; else sh_invb[r - la] = inv;
    }
  }
  __syncthreads();

  // ---- 2 + 3. tiles of sim, running maxima ----
  // One flat walk over (row tile, column tile, K chunk): the global loads of step s + 1 are issued before the MFMAs of step s,
  // so their latency hides under the matrix work, across tile boundaries too.
  const int r16 = lane & 15, g = lane >> 4;
  int i0 = 0, j0 = 0, c0 = 0;
  tm_f32x4 va[4], vb[4], acc[4];
  stage_load(pa, hidden, la, i0, c0, tid, va);
  stage_load(pb, hidden, lb, j0, c0, tid, vb);
#pragma unroll
  for (int v = 0; v < 4; ++v) acc[v] = tm_f32x4{0.f, 0.f, 0.f, 0.f};
  for (;;) {
    __syncthreads();                                                 // the previous chunk (and tile) has been read
    stage_store(sh_a, tid, va);
    stage_store(sh_b, tid, vb);
    int ni0 = i0, nj0 = j0, nc0 = c0 + kKC;                          // the step after this one (uniform)
    bool more = true;
    if (nc0 == hidden) {
      nc0 = 0;
      nj0 += kTile;
      if (nj0 >= lb) {
        nj0 = 0;
        ni0 += kTile;
        more = ni0 < la;
      }
    }
    if (more) {
      stage_load(pa, hidden, la, ni0, nc0, tid, va);
      stage_load(pb, hidden, lb, nj0, nc0, tid, vb);
    }
    __syncthreads();
    const bool wave_live = i0 + wave * 16 < la;                      // uniform per wave
    const int nv = lb - j0 >= kTile ? 4 : (lb - j0 + 15) >> 4;       // live 16-column groups (uniform)
    if (wave_live) {
      const float* xa = sh_a + (wave * 16 + r16) * kPitch + 4 * g;
      const float* xb = sh_b + r16 * kPitch + 4 * g;
      switch (nv) {                                                  // straight-line code per count: no branch between MFMAs
        case 1: mfma_chunk<1>(xa, xb, acc); break;
        case 2: mfma_chunk<2>(xa, xb, acc); break;
        case 3: mfma_chunk<3>(xa, xb, acc); break;
        default: mfma_chunk<4>(xa, xb, acc); break;
      }
    }
    if (c0 + kKC == hidden) {
      // the tile is complete: lane holds sim[i0 + 16 wave + 4 g + r][j0 + 16 v + r16] in acc[v][r]
      float cmax[4];
#pragma unroll
      for (int v = 0; v < 4; ++v) cmax[v] = ninf;
      if (wave_live) {
        float rmax[4];
        float ib[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) ib[v] = sh_invb[j0 + v * 16 + r16];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i = i0 + wave * 16 + 4 * g + r;
          const float ia = sh_inva[i];
          rmax[r] = ninf;
#pragma unroll
          for (int v = 0; v < 4; ++v) {
            const bool live = i < la && j0 + v * 16 + r16 < lb;
            const float s = live ? acc[v][r] * ia * ib[v] : ninf;
            rmax[r] = fmaxf(rmax[r], s);
            cmax[v] = fmaxf(cmax[v], s);
          }
#pragma unroll
          for (int o2 = 8; o2 > 0; o2 >>= 1) rmax[r] = fmaxf(rmax[r], __shfl_xor(rmax[r], o2));
          if (r16 == 0) sh_rowmax[i] = fmaxf(sh_rowmax[i], rmax[r]);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          cmax[v] = fmaxf(cmax[v], __shfl_xor(cmax[v], 16));
          cmax[v] = fmaxf(cmax[v], __shfl_xor(cmax[v], 32));
        }
      }
      if (g == 0) {
#pragma unroll
        for (int v = 0; v < 4; ++v) sh_cpart[wave][v * 16 + r16] = cmax[v];
      }
      __syncthreads();
      if (tid < kTile) {
        const float m = fmaxf(fmaxf(sh_cpart[0][tid], sh_cpart[1][tid]), fmaxf(sh_cpart[2][tid], sh_cpart[3][tid]));
        sh_colmax[j0 + tid] = fmaxf(sh_colmax[j0 + tid], m);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) acc[v] = tm_f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (!more) break;
    i0 = ni0;
    j0 = nj0;
    c0 = nc0;
  }
  __syncthreads();

  // ---- 4. weighted means ----
  if (wave == 0) {
    const float v = weighted_mean(sh_rowmax, w_a ? w_a + (size_t)p * seq_a : nullptr, la, lane);
    if (lane == 0) sh_pr[0] = v;
  } else if (wave == 1) {
    const float v = weighted_mean(sh_colmax, w_b ? w_b + (size_t)p * seq_b : nullptr, lb, lane);
    if (lane == 0) sh_pr[1] = v;
  }
  __syncthreads();
  if (tid == 0) {
    const float P = sh_pr[0], R = sh_pr[1];
    const float sum = P + R;
    const bool good = sum != 0.f && sum - sum == 0.f;                // finite and non-zero
    o[0] = P;
    o[1] = R;
    o[2] = good ? 2.f * P * R / sum : 0.f;
  }
}

}  // namespace

int token_match_launch(const float* a, const int* len_a, int seq_a, const float* b, const int* len_b, int seq_b, int n_pairs, int hidden,
                       const float* w_a, const float* w_b, float* out, hipStream_t stream) {
  hipLaunchKernelGGL(token_match_kernel, dim3((unsigned)n_pairs), dim3(kThreads), 0, stream, a, len_a, seq_a, b, len_b, seq_b, hidden,
                     w_a, w_b, out);
  return (int)hipGetLastError();
}

}  // namespace crs
