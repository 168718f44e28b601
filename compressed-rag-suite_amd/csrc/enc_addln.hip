// enc_addln.hip -- the row step of a pre-norm layer (ModernBERT, CRS_ENC_PRENORM): residual add + LayerNorm with two outputs.
// HBM-bound, layernorm_kernel's shapes (enc_misc.hip): one wave64 per token row, four tokens per workgroup, statistics in fp32 with
// the two-pass form of enc_ln.h.

#include "enc.h"
#include "enc_ln.h"

namespace crs {
namespace {

// Pre-norm layers (x += attn(LN(x)), x += mlp(LN(x))): the residual add that CLOSES a block and the norm that OPENS the next one
// in one launch, so that a pre-norm layer has as many row launches as a post-norm one.  r = ((y[0] + ... + y[NS - 1]) + bias) +
// residual is the new residual stream, written to r32 as it is (residual may be r32: every element is read before its row is
// written, by the same lane); x16 = fp16(LN(r) g + b) feeds the next GEMM; n32 (final norm only) keeps LN(r) g + b in fp32 for the
// pooling kernel and hidden_out.  b may be null: ModernBERT's norms have no bias.  Shapes as layernorm*_kernel: a wave per token,
// four tokens per workgroup, the slab counts of CRS_LN_SLABS, exact-width forms at hidden 384 / 768.
template <int P2, int NS>
__global__ __launch_bounds__(256) void add_layernorm2_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                            const float* residual,   // may alias r32 (in place)
                                                            const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                            int tokens, int hidden, float* r32, _Float16* __restrict__ x16,
                                                            float* __restrict__ n32) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* src = y + (size_t)t * hidden;
  const size_t split_stride = (size_t)tokens * hidden;
  float2 part[NS][P2], extra[2][P2];
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const int c = 128 * i + 2 * lane;
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) part[sidx][i] = *reinterpret_cast<const float2*>(src + sidx * split_stride + c);
    extra[0][i] = bias ? *reinterpret_cast<const float2*>(bias + c) : float2{0.f, 0.f};
    extra[1][i] = residual ? *reinterpret_cast<const float2*>(residual + (size_t)t * hidden + c) : float2{0.f, 0.f};
  }
  float v[P2][2];
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    float a0 = part[0][i].x, a1 = part[0][i].y;
#pragma unroll
    for (int sidx = 1; sidx < NS; ++sidx) { a0 += part[sidx][i].x; a1 += part[sidx][i].y; }
    v[i][0] = (a0 + extra[0][i].x) + extra[1][i].x;
    v[i][1] = (a1 + extra[0][i].y) + extra[1][i].y;
  }
  ln_store2_pre<P2>(v, hidden, lane, g, b, eps, r32 + (size_t)t * hidden, x16 + (size_t)t * hidden, n32 ? n32 + (size_t)t * hidden : nullptr);
}

template <int PL, int NS>
__global__ __launch_bounds__(256) void add_layernorm_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                           const float* residual,   // may alias r32 (in place)
                                                           const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                           int tokens, int hidden, float* r32, _Float16* __restrict__ x16,
                                                           float* __restrict__ n32) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* src = y + (size_t)t * hidden;
  const size_t split_stride = (size_t)tokens * hidden;
  float part[NS][PL], extra[2][PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int c = lane + 64 * i;
    const bool in = c < hidden;
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) part[sidx][i] = in ? src[sidx * split_stride + c] : 0.f;
    extra[0][i] = (in && bias) ? bias[c] : 0.f;
    extra[1][i] = (in && residual) ? residual[(size_t)t * hidden + c] : 0.f;
  }
  float v[PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    float a = part[0][i];
#pragma unroll
    for (int sidx = 1; sidx < NS; ++sidx) a += part[sidx][i];
    v[i] = (a + extra[0][i]) + extra[1][i];
  }
  ln_store_pre<PL>(v, hidden, lane, g, b, eps, r32 + (size_t)t * hidden, x16 + (size_t)t * hidden, n32 ? n32 + (size_t)t * hidden : nullptr);
}

}  // namespace

int add_layernorm_launch(const float* y, int nsplit, const float* bias, const float* residual, const float* g, const float* b,
                         float eps, int tokens, int hidden, float* r32, _Float16* x16, float* n32, hipStream_t stream) {
#define CRS_LN_CASE(KERNEL, PL, NS)                                                                                        \
  case NS: hipLaunchKernelGGL((KERNEL<PL, NS>), dim3((tokens + 3) / 4), dim3(256), 0, stream, y, bias, residual, g, b, eps, tokens, \
                              hidden, r32, x16, n32); break;
#define CRS_LN(KERNEL, PL) switch (nsplit) { CRS_LN_SLABS(CRS_LN_CASE, KERNEL, PL) default: return -1; }
  if (hidden == 384) { CRS_LN(add_layernorm2_kernel, 3) } else if (hidden == 768) { CRS_LN(add_layernorm2_kernel, 6) }
  else if (hidden <= 64) { CRS_LN(add_layernorm_kernel, 1) } else { CRS_LN(add_layernorm_kernel, 16) }
#undef CRS_LN
#undef CRS_LN_CASE
  return (int)hipGetLastError();
}

}  // namespace crs
