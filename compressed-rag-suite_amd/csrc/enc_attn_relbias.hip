// enc_attn_relbias.hip -- padding-masked, non-causal self-attention with an additive relative-position bias (gfx950).
//
//   ctx[b, s, h*hd : (h+1)*hd] = softmax(Q K^T / sqrt(hd) + bias[h][key - query] + mask) V        (per batch b, head h)
//
// What MPNet's layers compute (one bucketed bias table shared by all layers); the bias arrives RESOLVED per offset --
// fp32 rel_bias[heads][2 span - 1], entry (key - query) + span - 1, span >= seq -- so the bucket rule stays on the host
// and any other additive relative bias (T5-style, ALiBi slopes written out) runs through the same kernel.
//
// Same decomposition as the blocked attention_kernel of enc_attn.hip: one 256-thread workgroup per (64 queries, head,
// batch), computed transposed (S^T = K Q^T, O^T = V^T P^T), K row-major and V^T in LDS per 64-key block, online softmax
// in fp32 and in base 2, the same fp16 rounding points (Q, K, V as stored; the un-normalised probabilities; the
// output) and -1e30 for keys >= lens[b].  On top of it the workgroup stages its head's bias once: sBias[j] holds
// log2(e) * bias[h][j - (SP - 1)] for the offsets |j - (SP - 1)| < seq and 0 beyond, SP = seq rounded up to 64 -- every
// (query, key) pair of the padded tiles indexes inside the array, no clamp in the loop.  A score then costs one fma
// (raw product * log2(e) / sqrt(hd) + staged bias), a max, a subtract and one v_exp_f32; the running max is taken
// AFTER the bias is added (the bias can outweigh the product).  LDS: 2 x (64 x (hd + 4)) halves + 4 KB <= 21 KB.

#include "enc.h"

namespace crs {
namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;
constexpr int KB = 64;          // keys per block
constexpr int QB = 64;          // query rows per workgroup
constexpr int kMaxSeq = 512;    // sBias holds 2 * 512 - 1 offsets
constexpr float kLog2e = 1.44269504088896341f;

// One online-softmax step for this lane's query over the 16 scores it holds of a 64-key block: s = raw Q.K products of
// keys key0 + 16 ct + i; bias = this lane's window of the staged table (entry 16 ct + i belongs to that key).  Base-2
// domain: t = s * c + bias with c = log2(e) / sqrt(hd) and the bias already times log2(e).  Keys >= len get -1e30; every
// query sees key 0, so the running max is finite.
__device__ __forceinline__ void softmax_step_bias(f32x4 (&s)[4], const float* __restrict__ bias, int key0, int len, float c,
                                                  float& m_run, float& l_run, float& alpha, f16x4 (&pf)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) s[ct][i] = fmaf(s[ct][i], c, bias[ct * 16 + i]);
  if (key0 - (key0 & 15) + KB > len) {     // block reaches past len (wave-uniform: key0 = kb + 4 g)
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (key0 + ct * 16 + i >= len) s[ct][i] = -1e30f;
  }
  float mx = -1e30f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[ct][i]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float mn = fmaxf(m_run, mx);
  alpha = __builtin_amdgcn_exp2f(m_run - mn);
  m_run = mn;
  float rs = 0.f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = __builtin_amdgcn_exp2f(s[ct][i] - mn);
      rs += p;
      pf[ct][i] = (_Float16)p;
    }
  }
  rs += __shfl_xor(rs, 16);
  rs += __shfl_xor(rs, 32);
  l_run = l_run * alpha + rs;
}

template <int HD>
__global__ __launch_bounds__(kThreads) void attention_relbias_kernel(const _Float16* __restrict__ qkv,
                                                                    const int* __restrict__ lens,
                                                                    const float* __restrict__ rel_bias, int span,
                                                                    _Float16* __restrict__ ctx, int seq, int hidden) {
  constexpr int KS = HD / 16;          // k-steps of the Q K^T contraction
  constexpr int NT = HD / 16;          // 16-row tiles of O^T (head-dim index)
  constexpr int KROW = HD + 4;         // padded K row (halves)
  constexpr int VROW = KB + 4;         // padded V^T row (halves)
  __shared__ __attribute__((aligned(16))) _Float16 sK[KB * KROW];
  __shared__ __attribute__((aligned(16))) _Float16 sVt[HD * VROW];
  __shared__ float sBias[2 * kMaxSeq];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * QB + wave * 16;
  const int len = min(max(lens[b], 1), seq);
  const size_t row_stride = (size_t)3 * hidden;
  const _Float16* base = qkv + (size_t)b * seq * row_stride + h * HD;
  const float scale = kLog2e / sqrtf((float)HD);

  // ---- stage the head's bias, times log2(e): offsets -(SP - 1) .. SP - 1, zero where no (query, key) pair of real rows
  // has that offset (|offset| >= seq: rows of the padded tiles only).  Visible to every wave after the first barrier of
  // the key loop (len >= 1: the loop runs at least once).
  const int sp = (seq + KB - 1) / KB * KB;         // <= 512: the launcher checks seq
  {
    const float* hb = rel_bias + (size_t)h * (2 * span - 1) + (span - 1);     // offset 0 of this head
    for (int j = tid; j < 2 * sp - 1; j += kThreads) {
      const int d = j - (sp - 1);
      sBias[j] = (d > -seq && d < seq) ? hb[d] * kLog2e : 0.f;
    }
  }

  f16x4 qf[KS];                         // Q fragments (B operand of S^T): Q[query lr][hd 16 ks + 4 g .. + 4]
  {
    const int qr = q0 + lr;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      f16x4 z = {0, 0, 0, 0};
      qf[ks] = (qr < seq) ? *reinterpret_cast<const f16x4*>(base + (size_t)qr * row_stride + ks * 16 + g * 4) : z;
    }
  }
  f32x4 o[NT];                          // O^T tile n: rows = head-dim 16 n + 4 g + i, column = query lr
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;   // of this lane's query
  // this lane's keys of block kb are kb + 4 g + 16 ct + i, its query q0 + lr: staged entry (key - query) + sp - 1.
  // q0 + lr <= sp - 1 and key <= sp - 1, so the entries are within [0, 2 sp - 2]
  const int bias0 = 4 * g - (q0 + lr) + sp - 1;

  for (int kb = 0; kb < len; kb += KB) {
    __syncthreads();  // previous block's K / V^T fully consumed
    // ---- stage K (row-major): one 16-byte chunk per thread and pass
    constexpr int CH = HD / 8;  // 16-byte chunks per key row
    for (int id = tid; id < KB * CH; id += kThreads) {
      const int key = id / CH, c = id % CH;
      const int kr = kb + key;
      f16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (kr < seq) kv = *reinterpret_cast<const f16x8*>(base + (size_t)kr * row_stride + c * 8 + hidden);
      *reinterpret_cast<f16x4*>(&sK[key * KROW + c * 8]) = f16x4{kv[0], kv[1], kv[2], kv[3]};
      *reinterpret_cast<f16x4*>(&sK[key * KROW + c * 8 + 4]) = f16x4{kv[4], kv[5], kv[6], kv[7]};
    }
    // ---- stage V transposed: a thread takes 4 consecutive keys x 8 head-dim columns
    for (int id = tid; id < (KB / 4) * CH; id += kThreads) {
      const int kg = id / CH, c = id % CH;
      f16x8 vv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kr = kb + kg * 4 + j;
        const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
        vv[j] = (kr < seq) ? *reinterpret_cast<const f16x8*>(base + (size_t)kr * row_stride + c * 8 + 2 * hidden) : z;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e)
        *reinterpret_cast<f16x4*>(&sVt[(c * 8 + e) * VROW + kg * 4]) = f16x4{vv[0][e], vv[1][e], vv[2][e], vv[3][e]};
    }
    __syncthreads();

    // ---- S^T = K Q^T for 4 tiles of 16 keys: lane holds keys kb + 16 ct + 4 g + i of query lr
    f32x4 s[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      s[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x4 kf = *reinterpret_cast<const f16x4*>(&sK[(ct * 16 + lr) * KROW + ks * 16 + g * 4]);
        s[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[ks], s[ct], 0, 0, 0);
      }
    }
    float alpha;
    f16x4 pf[4];
    softmax_step_bias(s, &sBias[bias0 + kb], kb + 4 * g, len, scale, m_run, l_run, alpha, pf);
    // ---- O^T = O^T alpha + V^T P^T   (A = V^T[hd 16 n + lr][key 16 ct + 4 g + j], B = P^T from the registers)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[n][i] *= alpha;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[(n * 16 + lr) * VROW + ct * 16 + g * 4]);
        o[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[ct], o[n], 0, 0, 0);
      }
    }
  }
  // ---- normalise and store: this lane's query q0 + lr, head-dim columns 16 n + 4 g .. + 4 (8-byte stores)
  const int qr = q0 + lr;
  if (qr < seq) {
    const float inv = 1.0f / l_run;
    _Float16* dst = ctx + ((size_t)b * seq + qr) * hidden + h * HD;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const f16x4 v = {(_Float16)(o[n][0] * inv), (_Float16)(o[n][1] * inv), (_Float16)(o[n][2] * inv), (_Float16)(o[n][3] * inv)};
      *reinterpret_cast<f16x4*>(dst + n * 16 + 4 * g) = v;
    }
  }
}

}  // namespace

int attention_relbias_launch(const _Float16* qkv, const int* lens, const float* rel_bias, int span, _Float16* ctx, int batch,
                             int seq, int hidden, int heads, hipStream_t stream) {
  if (!rel_bias || seq < 1 || seq > kMaxSeq || span < seq || batch < 1 || batch > 65535) return -1;
  const int hd = hidden / heads;
  dim3 grid((seq + QB - 1) / QB, heads, batch);
  switch (hd) {
    case 16: hipLaunchKernelGGL((attention_relbias_kernel<16>), grid, dim3(kThreads), 0, stream, qkv, lens, rel_bias, span, ctx, seq, hidden); break;
    case 32: hipLaunchKernelGGL((attention_relbias_kernel<32>), grid, dim3(kThreads), 0, stream, qkv, lens, rel_bias, span, ctx, seq, hidden); break;
    case 64: hipLaunchKernelGGL((attention_relbias_kernel<64>), grid, dim3(kThreads), 0, stream, qkv, lens, rel_bias, span, ctx, seq, hidden); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace crs
