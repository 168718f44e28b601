// token_project.hip -- hidden states to packed unit-length fp16 token vectors (gfx950): crs_token_project.
//
// The index-time half of late interaction: for every token with dst >= 0, v = W h (+ b), y = v / |v| (0 when |v| is 0), written as
// fp16 to row dst of the token array, zeros in [dim, dimp).  A row-complete MFMA tile, as enc_rowln.hip's: one wave owns 16 tokens
// and ALL dimp output columns (dimp / 16 accumulator tiles of v_mfma_f32_16x16x32_f16, at most 8 = 32 VGPRs), so the norm of a row
// is formed inside the wave that produced it and the projection never round-trips through memory.  Four waves per workgroup, 64
// tokens.
//   A operand: lane (r = lane & 15, h = lane >> 4) reads coordinates k0 + 8 h .. + 7 of token r's hidden row -- two 16-byte fp32
//     loads, rounded to fp16 (round to nearest even) in registers.  A token with dst < 0, or past n_tok, is NEVER read: it is a
//     padding position whose hidden state is undefined; its fragment is zeros and nothing is stored for it.
//   B operand: the same coordinates of row 16 j + r of W, one 16-byte load per column tile j, straight from global memory -- W is
//     at most 128 x 1024 fp16 = 256 KB and stays in L2 for the whole launch.  Rows at or past dim are zeros and are not read.
//     Every wave reads the whole of W for its 16 tokens and the four waves of a workgroup share nothing: about four times the L2
//     traffic of the hidden block itself (96 KB of W against 24 KB of hidden states per wave at 128 x 384).  Staging W through LDS
//     once per workgroup would remove three quarters of it; whether that matters has NOT been measured -- the index build is
//     bound by the encoder forward in front of this kernel.
//   Epilogue: accumulator register e of lane (c = lane & 15, g = lane >> 4), tile j is column 16 j + c of token 4 g + e.  Bias in
//     fp32, squares summed over the lane's tiles in j order, then an xor butterfly over the 16 lanes of the row; 1 / sqrt in fp32;
//     the scaled value is rounded to fp16 once.  The 16 lanes of a row store 32 contiguous bytes per tile.
// A token's arithmetic involves its own row of A alone: its output does not depend on what else is in the launch.  No scratch, no
// LDS, no atomics.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"

namespace crs {
namespace {

typedef _Float16 tp_f16x8 __attribute__((ext_vector_type(8)));
typedef float tp_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTpThreads = 256;

template <int NJ>   // column tiles of 16: dimp = 16 NJ
__global__ __launch_bounds__(kTpThreads) void token_project_kernel(const float* __restrict__ hidden, const _Float16* __restrict__ w16,
                                                                   const float* __restrict__ bias, const long long* __restrict__ dst,
                                                                   _Float16* __restrict__ out16, long long n_tok, int H, int dim) {
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
      _Float16* o16 = out16 + (size_t)d * kDimp + r;
#pragma unroll
      for (int j = 0; j < NJ; ++j) o16[16 * j] = (_Float16)(acc[j][e] * inv);
    }
  }
}

}  // namespace

int token_project_launch(const float* hidden, const void* w16, const float* bias, const int64_t* dst, void* out16, int64_t n_tok,
                         int H, int dim, hipStream_t stream) {
  const int dimp = (dim + 31) / 32 * 32;
  const dim3 grid((unsigned)((n_tok + 63) / 64)), block(kTpThreads);
#define CRS_TP_LAUNCH(NJ)                                                                                                          \
  hipLaunchKernelGGL(token_project_kernel<NJ>, grid, block, 0, stream, hidden, static_cast<const _Float16*>(w16), bias,            \
                     reinterpret_cast<const long long*>(dst), static_cast<_Float16*>(out16), (long long)n_tok, H, dim)
  switch (dimp) {
    case 32: CRS_TP_LAUNCH(2); break;
    case 64: CRS_TP_LAUNCH(4); break;
    case 96: CRS_TP_LAUNCH(6); break;
    case 128: CRS_TP_LAUNCH(8); break;
    default: return -1;
  }
#undef CRS_TP_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace crs
