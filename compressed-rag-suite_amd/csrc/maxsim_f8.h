// maxsim_f8.h -- the operand layout, the decode and the matrix step of the fp8 MaxSim kernels (maxsim_f8.hip, maxsim_scan_f8.hip;
// DESIGN 3.23).  Both kernels take their fragments and their products from here, which is what makes a swept score bit for bit
// the re-rank kernel's.  Device code only.
//
// A token row is dimp = 32 KS bytes of e4m3 = 2 KS chunks of 16 bytes.  Lane (r = lane & 15, h = lane >> 4) holds 32 bytes of
// token r: chunk h in registers 0..3 and chunk 4 + h in registers 4..7; a chunk at or past 2 KS is zeros (dimp 96: the upper
// halves of h = 2, 3; dimp 64: every upper half; dimp 32: everything but the lower halves of h = 0, 1).
//
// Why not the fp8 matrix instructions.  The format's contract is exact products and an fp32 accumulation.  Measured with one wave
// on unit-vector data: v_mfma_scale_f32_16x16x128_f8f6f4 (with 2^-8 scales and with unit scales) and four
// v_mfma_f32_16x16x32_fp8_fp8 return the SAME bits, and those differ from the exact sum by up to 1.24 on 64 547 (2e-5) and by
// thousands of ulps of a small result: the fp8 datapath aligns the products to the largest and keeps too few bits.  So the
// fragments are DECODED to fp16 in registers -- exactly: e4m3 bits (b & 0x7f) << 7 read as fp16 are the value times 2^-8, normal
// or subnormal, so one byte permute, one shift-and-mask and one and-or per two codes give stored * 2^-S = the unit-scale
// coordinate -- and multiplied by v_mfma_f32_16x16x32_f16, whose fp32 accumulation maxsim.hip already relies on.  A fragment's 32
// bytes become 4 (KS <= 2: the 2 non-zero) f16x8 k-steps, accumulated in ascending order from a zero accumulator; both operands
// are cut the same way, which is all a dot product needs.  The index, the LDS-DMA and the LDS reads keep the halved bytes; the
// halved fragment registers and the single instruction are given up.  The 2^(-2 S) of the score is in the decode.
#pragma once
#include <hip/hip_runtime.h>

#include "e4m3.h"

namespace crs {
namespace {

typedef int f8x32 __attribute__((ext_vector_type(8)));      // 32 e4m3 codes: one lane's share of an operand
typedef float f8_f32x4 __attribute__((ext_vector_type(4)));

template <int KS>
__device__ __forceinline__ bool f8_chunk_live(int c) { return c < 2 * KS; }

__device__ __forceinline__ f8x32 f8_frag(const uint4 lo, const uint4 hi) {
  return f8x32{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
}

// lane (r, h)'s fragment of the row at `row` (global memory, 16-byte aligned)
template <int KS>
__device__ __forceinline__ f8x32 f8_load_frag(const unsigned char* row, int h) {
  uint4 lo = uint4{0, 0, 0, 0}, hi = uint4{0, 0, 0, 0};
  if (f8_chunk_live<KS>(h)) lo = *reinterpret_cast<const uint4*>(row + 16 * h);
  if (KS > 2 && f8_chunk_live<KS>(4 + h)) hi = *reinterpret_cast<const uint4*>(row + 16 * (4 + h));
  return f8_frag(lo, hi);
}

typedef _Float16 f8_f16x8 __attribute__((ext_vector_type(8)));
template <int KS>
struct F8Frag16 {                                           // a fragment decoded: the k-steps that can be non-zero
  static constexpr int kSteps = KS > 2 ? 4 : 2;
  f8_f16x8 v[kSteps];
};

// two e4m3 codes (bytes `sel` picks into the upper byte of each half) -> two fp16 of value code * 2^-8: sign to bit 15, the seven
// other bits to bits 13..7
__device__ __forceinline__ unsigned f8_decode2(unsigned w, unsigned sel) {
  const unsigned y = __builtin_amdgcn_perm(0u, w, sel);
  return ((y >> 1) & 0x3f803f80u) | (y & 0x80008000u);
}
template <int KS>
__device__ __forceinline__ F8Frag16<KS> f8_decode(const f8x32 f) {
  F8Frag16<KS> out;
#pragma unroll
  for (int s = 0; s < F8Frag16<KS>::kSteps; ++s) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const unsigned w0 = (unsigned)f[2 * s], w1 = (unsigned)f[2 * s + 1];
    const u4 d = u4{f8_decode2(w0, 0x010c000cu), f8_decode2(w0, 0x030c020cu), f8_decode2(w1, 0x010c000cu), f8_decode2(w1, 0x030c020cu)};
    out.v[s] = __builtin_bit_cast(f8_f16x8, d);
  }
  return out;
}

// <16 query tokens, 16 document tokens> from a zero accumulator, k-steps in ascending order
template <int KS>
__device__ __forceinline__ f8_f32x4 f8_mfma(const F8Frag16<KS>& a, const F8Frag16<KS>& b) {
  f8_f32x4 acc = f8_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < F8Frag16<KS>::kSteps; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v[s], b.v[s], acc, 0, 0, 0);
  return acc;
}

// maxsim.hip step 4 for one query: the maxima of the lane's rows over the 16 columns of their row, added in (b, e) order within
// a 16-lane group, then the groups as ((g0 + g1) + g2) + g3; every lane returns the score.  A row at or past lq adds +0 through
// a select instead of being skipped by a branch (no lane mask lives in scalar registers): the partial sum starts at +0 and a
// sum of floats is never -0, so adding +0 changes no bit.
__device__ __forceinline__ float f8_row_sum(const float (&best)[4][4], int nrb, int lq, int h) {
  float sum = 0.f;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    if (b < nrb) {                                          // (uniform)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m = best[b][e];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        sum += 16 * b + 4 * h + e < lq ? m : 0.f;
      }
    }
  }
  const float g1 = __shfl(sum, 16), g2 = __shfl(sum, 32), g3 = __shfl(sum, 48);
  return __shfl(((sum + g1) + g2) + g3, 0);
}

}  // namespace
}  // namespace crs
