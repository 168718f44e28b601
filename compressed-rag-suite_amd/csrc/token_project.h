// token_project.h -- the token projection kernel (token_project.hip describes it), a template over the output format so that the
// fp16 launcher (token_project.hip) and the e4m3 launcher (token_project_f8.hip) instantiate one definition.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "e4m3.h"

namespace crs {
namespace {

typedef _Float16 tp_f16x8 __attribute__((ext_vector_type(8)));
typedef float tp_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTpThreads = 256;

template <int NJ, bool F8>   // column tiles of 16: dimp = 16 NJ; F8: out is uint8 e4m3 codes, else fp16
__global__ __launch_bounds__(kTpThreads) void token_project_kernel(const float* __restrict__ hidden, const _Float16* __restrict__ w16,
                                                                   const float* __restrict__ bias, const long long* __restrict__ dst,
                                                                   void* __restrict__ out, long long n_tok, int H, int dim) {
  constexpr int kDimp = 16 * NJ;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 15, h = lane >> 4;
  const long long tok0 = (long long)blockIdx.x * 64 + wave * 16;
  if (tok0 >= n_tok) return;                                // (wave-uniform)

  const long long tok = tok0 + r;
  const bool live = tok < n_tok && dst[tok] >= 0;
  const float* hrow = hidden + (size_t)(live ? tok : 0) * H + 8 * h;
  const _Float16* wrow = w16 + 8 * h;

  tp_f32x4 acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = tp_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int k0 = 0; k0 < H; k0 += 32) {
    tp_f16x8 af = tp_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
      const tp_f32x4 lo = *reinterpret_cast<const tp_f32x4*>(hrow + k0), hi = *reinterpret_cast<const tp_f32x4*>(hrow + k0 + 4);
      af = tp_f16x8{(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3],
                    (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
    }
    tp_f16x8 bf[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      bf[j] = tp_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (16 * j + r < dim) bf[j] = *reinterpret_cast<const tp_f16x8*>(wrow + (size_t)(16 * j + r) * H + k0);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[j], acc[j], 0, 0, 0);
  }

  // ---- epilogue: bias, row norm, scale, store
  float bj[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) bj[j] = (bias && 16 * j + r < dim) ? bias[16 * j + r] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      acc[j][e] += bj[j];
      ss = fmaf(acc[j][e], acc[j][e], ss);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    const float inv = ss > 0.f ? 1.f / sqrtf(ss) : 0.f;
    const long long t = tok0 + 4 * h + e;
    const long long d = t < n_tok ? dst[t] : -1;
    if (d >= 0) {
      if constexpr (F8) {
        unsigned char* o8 = static_cast<unsigned char*>(out) + (size_t)d * kDimp + r;
        constexpr float kUp = (float)(1 << CRS_F8_TOKEN_SHIFT);
#pragma unroll
        for (int j = 0; j < NJ; ++j) o8[16 * j] = (unsigned char)(16 * j + r < dim ? e4m3_signed_code(acc[j][e] * inv * kUp) : 0u);
      } else {
        _Float16* o16 = static_cast<_Float16*>(out) + (size_t)d * kDimp + r;
#pragma unroll
        for (int j = 0; j < NJ; ++j) o16[16 * j] = (_Float16)(acc[j][e] * inv);
      }
    }
  }
}

}  // namespace
}  // namespace crs
