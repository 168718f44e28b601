// The row LayerNorm of the encoder's HBM-bound kernels (enc_misc.hip; wave_sum also in enc_pair.hip): one wave64 per token row, statistics in
// fp32 with a two-pass (mean, then centred variance) form, eps inside the sqrt exactly as torch.nn.LayerNorm.  Each form writes
// the fp32 residual stream AND the fp16 copy the next GEMM reads.  One definition, so that kernels which build the same row the
// same way (the embedding kernels with and without per-token type ids) give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace crs {

__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}

// v[] holds this lane's strided elements (index c = lane + 64*i); normalise and store
template <int PL>
__device__ __forceinline__ void ln_store(float (&v)[PL], int hidden, int lane, const float* g,
                                         const float* b, float eps, float* x32, _Float16* x16) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PL; ++i) s += (lane + 64 * i < hidden) ? v[i] : 0.f;
  const float mean = wave_sum(s) / hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const float d = v[i] - mean;
    q += (lane + 64 * i < hidden) ? d * d : 0.f;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / hidden + eps);
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int c = lane + 64 * i;
    if (c < hidden) {
      const float o = (v[i] - mean) * rstd * g[c] + b[c];
      x32[c] = o;
      x16[c] = (_Float16)o;
    }
  }
}

// ---- float2 forms (hidden a multiple of 128): a lane owns columns 128 i + 2 lane + {0, 1}.  These kernels are
// bound by vector-memory ISSUE, not bytes -- a wave pays ~100 cycles per load/store instruction whatever its
// width, and the 4-byte form needs 48 of them per token at four split-K partials -- so 8 bytes per lane
// halves their time on the retrieve path (16 bytes would leave a third of the lanes without work at 384).
template <int P2>
__device__ __forceinline__ void ln_store2(float (&v)[P2][2], int hidden, int lane, const float* g, const float* b,
                                          float eps, float* x32, _Float16* x16) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < P2; ++i) s += v[i][0] + v[i][1];
  const float mean = wave_sum(s) / hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const float d0 = v[i][0] - mean, d1 = v[i][1] - mean;
    q += d0 * d0 + d1 * d1;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / hidden + eps);
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const int c = 128 * i + 2 * lane;
    const float2 gg = *reinterpret_cast<const float2*>(g + c), bb = *reinterpret_cast<const float2*>(b + c);
    float2 o;
    o.x = (v[i][0] - mean) * rstd * gg.x + bb.x;
    o.y = (v[i][1] - mean) * rstd * gg.y + bb.y;
    *reinterpret_cast<float2*>(x32 + c) = o;
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 h = {(_Float16)o.x, (_Float16)o.y};
    *reinterpret_cast<h2*>(x16 + c) = h;
  }
}

// ---- the pre-norm forms (add_layernorm*_kernel): v[] is the new residual row.  It is written to r32 AS IT IS, and its
// LayerNorm goes to x16 (fp16, the next GEMM's input) and, where n32 is given (the final norm), to n32 in fp32.  b may be null
// (a norm without bias).  Same statistics, in the same order, as the forms above.
template <int PL>
__device__ __forceinline__ void ln_store_pre(float (&v)[PL], int hidden, int lane, const float* g, const float* b, float eps,
                                             float* r32, _Float16* x16, float* n32) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < PL; ++i) s += (lane + 64 * i < hidden) ? v[i] : 0.f;
  const float mean = wave_sum(s) / hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const float d = v[i] - mean;
    q += (lane + 64 * i < hidden) ? d * d : 0.f;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / hidden + eps);
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int c = lane + 64 * i;
    if (c < hidden) {
      const float o = (v[i] - mean) * rstd * g[c] + (b ? b[c] : 0.f);
      r32[c] = v[i];
      x16[c] = (_Float16)o;
      if (n32) n32[c] = o;
    }
  }
}

template <int P2>
__device__ __forceinline__ void ln_store2_pre(float (&v)[P2][2], int hidden, int lane, const float* g, const float* b, float eps,
                                              float* r32, _Float16* x16, float* n32) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < P2; ++i) s += v[i][0] + v[i][1];
  const float mean = wave_sum(s) / hidden;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const float d0 = v[i][0] - mean, d1 = v[i][1] - mean;
    q += d0 * d0 + d1 * d1;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / hidden + eps);
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const int c = 128 * i + 2 * lane;
    const float2 gg = *reinterpret_cast<const float2*>(g + c), bb = b ? *reinterpret_cast<const float2*>(b + c) : float2{0.f, 0.f};
    float2 o;
    o.x = (v[i][0] - mean) * rstd * gg.x + bb.x;
    o.y = (v[i][1] - mean) * rstd * gg.y + bb.y;
    *reinterpret_cast<float2*>(r32 + c) = float2{v[i][0], v[i][1]};
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 h = {(_Float16)o.x, (_Float16)o.y};
    *reinterpret_cast<h2*>(x16 + c) = h;
    if (n32) *reinterpret_cast<float2*>(n32 + c) = o;
  }
}

}  // namespace crs
