// enc_rope.hip -- rotary position embedding of the Q and K column blocks of the QKV buffer, in place (CRS_ENC_ROTARY,
// include/crs_encoder.h): one launch between the QKV projection and attention, so every unfused attention kernel serves
// rotary models unchanged.  HBM-bound: 8 T H bytes per call (Q and K read and written once), no LDS.
//
// "Rotate-half" form over the whole head dimension: columns j and j + hd / 2 of a head are one pair,
//     t'[j]        = t[j]        cos - t[j + hd/2] sin
//     t'[j + hd/2] = t[j + hd/2] cos + t[j]        sin        cos / sin = table[pos][j], table[pos][hd / 2 + j]
// A thread owns 8 consecutive pairs of one head of Q or K of one token: two 16-byte fp16 loads, four 16-byte table loads,
// fp32 arithmetic, two 16-byte stores.  No thread reads what another writes.
// qk_norm_rope_kernel (below) is the rotation of Qwen3's grouped layout with the per-head RMSNorm in front of it.

#include "enc.h"

namespace crs {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int HD>
__global__ __launch_bounds__(forms::kRopeThreads) void rope_qk_kernel(_Float16* __restrict__ qkv, const float* __restrict__ table,
                                                                      long items, int seq, int hidden) {
  constexpr int kHalf = HD / 2, kPer = HD / 16;   // threads per head
  const long idx = (long)blockIdx.x * forms::kRopeThreads + threadIdx.x;
  if (idx >= items) return;
  const int per_tok = hidden >> 3, per_blk = hidden >> 4;   // Q and K; one of them
  const long t = idx / per_tok;
  const int r = (int)(idx - t * per_tok);
  const int qk = r / per_blk, rr = r - qk * per_blk;
  const int head = rr / kPer, j0 = (rr - head * kPer) * 8;
  const int pos = (int)(t % seq);
  _Float16* lo = qkv + (size_t)t * (3 * hidden) + qk * hidden + head * HD + j0;
  _Float16* hi = lo + kHalf;
  const float* c = table + (size_t)pos * HD + j0;
  const f16x8 a = *reinterpret_cast<const f16x8*>(lo), b = *reinterpret_cast<const f16x8*>(hi);
  const f32x4 c0 = *reinterpret_cast<const f32x4*>(c), c1 = *reinterpret_cast<const f32x4*>(c + 4);
  const f32x4 s0 = *reinterpret_cast<const f32x4*>(c + kHalf), s1 = *reinterpret_cast<const f32x4*>(c + kHalf + 4);
  f16x8 oa, ob;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = (float)a[e], y = (float)b[e];
    const float cs = e < 4 ? c0[e & 3] : c1[e & 3], sn = e < 4 ? s0[e & 3] : s1[e & 3];
    oa[e] = (_Float16)(x * cs - y * sn);
    ob[e] = (_Float16)(y * cs + x * sn);
  }
  *reinterpret_cast<f16x8*>(lo) = oa;
  *reinterpret_cast<f16x8*>(hi) = ob;
}

// Qwen3's QK-norm + rotation (CRS_ENC_CAUSAL): per (token, head) of the Q and K blocks of qkv [tokens, (Hq + 2 Hkv) hd], in place,
//     n = RMSNorm_hd(t; gain)   fp32: t * 1 / sqrt(mean(t^2) + eps) * gain      (g_q for the Hq query heads, g_k for the Hkv key heads)
//     t'[j] = n[j] cos - n[j + hd/2] sin,   t'[j + hd/2] = n[j + hd/2] cos + n[j] sin        (the table layout above)
// rounded ONCE to fp16; the V block is not touched.  A lane owns exactly one rotation pair (j, j + hd/2): at head_dim 128 a wave is one
// head and the sum of squares is a 64-lane reduction; at 64 a wave's halves are two heads (items 2 s and 2 s + 1 of the token-major
// (token, head) list) and the reduction stops at 32 lanes.  No LDS, no barrier.  The Q and K blocks are neighbours in a row, so head
// index h in [0, Hq + Hkv) sits at column h * hd.
template <int HD>
__global__ __launch_bounds__(forms::kQkNormThreads) void qk_norm_rope_kernel(_Float16* __restrict__ qkv, const float* __restrict__ table,
                                                                           const float* __restrict__ g_q, const float* __restrict__ g_k,
                                                                           float eps, long heads_total, int seq, int q_heads, int kv_heads) {
  constexpr int kHalf = HD / 2;
  const int lane = threadIdx.x & 63;
  const long slot = (long)blockIdx.x * (forms::kQkNormThreads / 64) + (threadIdx.x >> 6);
  const long item = HD == 128 ? slot : 2 * slot + (lane >> 5);      // index into the (token, head) list
  const bool live = item < heads_total;
  const int j = lane & (kHalf - 1);
  const int hqk = q_heads + kv_heads;
  const long it = live ? item : 0;
  const long t = it / hqk;
  const int head = (int)(it - t * hqk);
  _Float16* p = qkv + (size_t)t * ((size_t)(hqk + kv_heads) * HD) + (size_t)head * HD + j;
  const float* c = table + (size_t)(t % seq) * HD + j;
  const float* gain = (head < q_heads ? g_q : g_k) + j;
  const float x = (float)p[0], y = (float)p[kHalf];
  float ss = x * x + y * y;
#pragma unroll
  for (int o = kHalf / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o);   // 64 lanes at head_dim 128, a 32-lane half at 64
  const float r = 1.0f / sqrtf(ss / HD + eps);
  const float nx = x * r * gain[0], ny = y * r * gain[kHalf];
  const float cs = c[0], sn = c[kHalf];
  if (live) {
    p[0] = (_Float16)(nx * cs - ny * sn);
    p[kHalf] = (_Float16)(ny * cs + nx * sn);
  }
}

}  // namespace

int qk_norm_rope_launch(const Dims& d, int hd, _Float16* qkv, const float* table, const float* g_q, const float* g_k, float eps,
                        int tokens, int seq, int q_heads, int kv_heads, hipStream_t stream) {
  const long total = (long)tokens * (q_heads + kv_heads);
  switch (hd) {
    case 64: hipLaunchKernelGGL((qk_norm_rope_kernel<64>), dim3(d.gx), dim3(d.threads), 0, stream, qkv, table, g_q, g_k, eps, total, seq, q_heads, kv_heads); break;
    case 128: hipLaunchKernelGGL((qk_norm_rope_kernel<128>), dim3(d.gx), dim3(d.threads), 0, stream, qkv, table, g_q, g_k, eps, total, seq, q_heads, kv_heads); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

int rope_qk_launch(const Dims& d, int hd, _Float16* qkv, const float* table, int tokens, int seq, int hidden, hipStream_t stream) {
  const long items = forms::rope_items(tokens, hidden);
  switch (hd) {
    case 16: hipLaunchKernelGGL((rope_qk_kernel<16>), dim3(d.gx), dim3(d.threads), 0, stream, qkv, table, items, seq, hidden); break;
    case 32: hipLaunchKernelGGL((rope_qk_kernel<32>), dim3(d.gx), dim3(d.threads), 0, stream, qkv, table, items, seq, hidden); break;
    case 64: hipLaunchKernelGGL((rope_qk_kernel<64>), dim3(d.gx), dim3(d.threads), 0, stream, qkv, table, items, seq, hidden); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace crs
