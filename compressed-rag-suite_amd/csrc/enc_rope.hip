// enc_rope.hip -- rotary position embedding of the Q and K column blocks of the QKV buffer, in place (CRS_ENC_ROTARY,
// include/crs_encoder.h): one launch between the QKV projection and attention, so every unfused attention kernel serves
// rotary models unchanged.  HBM-bound: 8 T H bytes per call (Q and K read and written once), no LDS.
//
// "Rotate-half" form over the whole head dimension: columns j and j + hd / 2 of a head are one pair,
//     t'[j]        = t[j]        cos - t[j + hd/2] sin
//     t'[j + hd/2] = t[j + hd/2] cos + t[j]        sin        cos / sin = table[pos][j], table[pos][hd / 2 + j]
// A thread owns 8 consecutive pairs of one head of Q or K of one token: two 16-byte fp16 loads, four 16-byte table loads,
// fp32 arithmetic, two 16-byte stores.  No thread reads what another writes.

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

}  // namespace

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
