// enc_attn_steps.h -- the steps the attention kernels of enc_attn.hip and enc_attn_causal.hip are composed from, each defined once:
// softmax_step<Score> (the online-softmax step in its three score modes), load_q_frags, stage_k, stage_vt and store_o.  Everything is
// __forceinline__ in an unnamed namespace, so a translation unit that includes this compiles exactly what it compiled when the
// definitions stood in it.
#pragma once
#include <hip/hip_runtime.h>

#include "enc_forms.h"

namespace crs {
namespace {

typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = forms::kAttnThreads;
constexpr int KB = 64;   // keys per block
constexpr int QB = forms::kAttnQ;   // query rows per workgroup
constexpr int kMaxSeq = forms::kAttnMaxBiasSeq;    // relative bias: the staged table holds 2 * 512 - 1 offsets
constexpr float kLog2e = 1.44269504088896341f;

enum class Score { Plain, Bias, Window };

// What a step needs beyond the raw products to form and mask its scores.
struct KeyMask {
  int len;                 // keys >= len are right padding
  const float* bias;       // Bias: this lane's window of the staged table at this key block
  int q, window;           // Window: this lane's query and the largest allowed |key - query|
  bool inside;             // Window: the whole block is allowed for all 16 queries of the wave (wave-uniform): no test
};

// One online-softmax step for this lane's query over the 16 scores it holds of a 64-key block (raw Q.K products of keys
// key0 + 16 ct + i in s).  Works in the base-2 domain with the 1/sqrt(hd) scale folded into one constant c = log2(e) / sqrt(hd).
// A masked key is set to -1e30 before the max, so its weight is exp2(-huge) = 0.  The modes round differently and each keeps its
// own form; the reductions and the running sum are the same code:
//   Plain   keys >= len (right padding, last block only) are masked on the RAW product; every query sees key 0, so the running
//           max is finite.  Per score a max on the raw product, one fma and one v_exp_f32 (the softmax, not the MFMAs, bounds
//           this kernel: 16 scores per lane and block against 16 small MFMAs per wave);
//           (the causal kernel passes a len PER LANE -- min(query + 1, len) -- which is the same test: enc_attn_causal.hip)
//   Bias    m.bias = this lane's window of the staged table (entry 16 ct + i belongs to that key, already times log2(e)):
//           t = s * c + bias first, then the padding mask, and the max is taken AFTER the bias is added (the bias can outweigh
//           the product);
//   Window  t = s * c (a plain multiply), then a score outside the window or at key >= len is masked unless m.inside.
//           Two things the other modes' comments rule out happen here:
//     * a query's FIRST visited block can lie wholly outside its window (W = 8: rows 73 .. 127 of query block 1 against key block 0),
//       so "every row sees key 0, the max is finite" does not hold.  The running maximum then stays at the sentinel -1e30 and that
//       block's weights are exp2(-1e30 - -1e30) = 1, on finite V values; the first block with an allowed key rescales by
//       exp2(-1e30 - finite) = 0 exactly, which wipes the accumulator and the row sum.  That needs the masked score, the maximum and
//       the subtraction to be the SAME fp32 number: the step scales first (t = s c) and masks t, instead of masking the raw product and
//       folding c into an fma as Plain does -- fma(-1e30, c, fl(1e30 c)) is the product's rounding error, about 2^70, and
//       exp2 of that is infinity.  The sentinel is finite on purpose: with -inf the same subtraction is inf - inf = NaN.
//     * a padding query at q >= len + W has no allowed key at all (and a workgroup whose whole query block is such visits no block).
//       Its row is written as ZEROS (attention_window_kernel's store): the row sum would be 0 or a count of masked keys, and a NaN there
//       would poison real rows in the next layer's MFMAs (0 x NaN) although their weight for this position is 0.  Every real query
//       allows itself.
template <Score MODE>
__device__ __forceinline__ void softmax_step(f32x4 (&s)[4], const KeyMask m, int key0, float c, float& m_run, float& l_run,
                                             float& alpha, f16x4 (&pf)[4]) {
  if constexpr (MODE != Score::Plain) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) s[ct][i] = MODE == Score::Bias ? fmaf(s[ct][i], c, m.bias[ct * 16 + i]) : s[ct][i] * c;
  }
  // Plain / Bias: only a block that reaches past len (wave-uniform: key0 = kb + 4 g); Window: every block not inside (wave-uniform)
  // (the causal kernel's len is per lane, so there this branch DIVERGES within a wave: harmless, the four lanes of a query share the
  // limit and nothing inside the branch crosses lanes -- keep every shuffle outside it)
  const int len = m.len, q = m.q, window = m.window;
  if (MODE == Score::Window ? !m.inside : key0 - (key0 & 15) + KB > len) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = key0 + ct * 16 + i, d = key - q;
        if (MODE == Score::Window ? key >= len || d > window || d < -window : key >= len) s[ct][i] = -1e30f;
      }
  }
  float mx = -1e30f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[ct][i]);
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float mn = fmaxf(m_run, MODE == Score::Plain ? mx * c : mx);
  alpha = __builtin_amdgcn_exp2f(m_run - mn);
  m_run = mn;
  float rs = 0.f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float p = __builtin_amdgcn_exp2f(MODE == Score::Plain ? fmaf(s[ct][i], c, -mn) : s[ct][i] - mn);
      rs += p;
      pf[ct][i] = (_Float16)p;
    }
  }
  rs += __shfl_xor(rs, 16);
  rs += __shfl_xor(rs, 32);
  l_run = l_run * alpha + rs;
}

// ---- the steps every kernel is composed from (base = the (batch, head)'s Q column block of qkv; K at + hidden, V at
// + 2 hidden; rows >= seq read as zero).  The causal kernel's K / V blocks are narrower than its Q block: it passes the K (or V)
// head's own pointer as base and 0 as hidden.

// Q fragments of query row qr (B operand of S^T): lane group g holds Q[qr][hd N (4 ks + g) .. + N], N = 4 halves for the
// 16-deep MFMA (f16x4) and 8 for the 32-deep one (f16x8).
template <int KS, typename Frag>
__device__ __forceinline__ void load_q_frags(Frag (&qf)[KS], const _Float16* __restrict__ base, size_t row_stride, int qr, int seq, int g) {
  constexpr int N = sizeof(Frag) / sizeof(_Float16);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const Frag z = {};
    qf[ks] = (qr < seq) ? *reinterpret_cast<const Frag*>(base + (size_t)qr * row_stride + ks * 4 * N + g * N) : z;
  }
}

// K rows k0 .. k0 + nkeys - 1 -> sK[0 .. nkeys) row-major with pitch KROW: one 16-byte chunk per thread and pass, stored
// whole where the pitch keeps rows 16-byte aligned (KROW % 8 == 0) and as two 8-byte halves otherwise.
template <int HD, int KROW, int NTHR>
__device__ __forceinline__ void stage_k(_Float16* sK, const _Float16* __restrict__ base, size_t row_stride, int hidden, int seq,
                                        int k0, int nkeys, int tid) {
  constexpr int CH = HD / 8;  // 16-byte chunks per key row
  for (int id = tid; id < nkeys * CH; id += NTHR) {
    const int key = id / CH, c = id % CH;
    const int kr = k0 + key;
    f16x8 kv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (kr < seq) kv = *reinterpret_cast<const f16x8*>(base + (size_t)kr * row_stride + c * 8 + hidden);
    if constexpr (KROW % 8 == 0) {
      *reinterpret_cast<f16x8*>(&sK[key * KROW + c * 8]) = kv;
    } else {
      *reinterpret_cast<f16x4*>(&sK[key * KROW + c * 8]) = f16x4{kv[0], kv[1], kv[2], kv[3]};
      *reinterpret_cast<f16x4*>(&sK[key * KROW + c * 8 + 4]) = f16x4{kv[4], kv[5], kv[6], kv[7]};
    }
  }
}

// V rows k0 .. k0 + nkeys - 1 -> sVt[hd][0 .. nkeys) TRANSPOSED with pitch VROW: a thread takes 4 consecutive keys x 8
// head-dim columns and writes eight 8-byte pieces (4 keys of one column) instead of 32 two-byte stores.  PERM32: the
// key order inside every 32-key group that attention_seq32_kernel's 32-deep second product wants (see there).
template <int HD, int VROW, int NTHR, bool PERM32>
__device__ __forceinline__ void stage_vt(_Float16* sVt, const _Float16* __restrict__ base, size_t row_stride, int hidden, int seq,
                                         int k0, int nkeys, int tid) {
  constexpr int CH = HD / 8;
  for (int id = tid; id < (nkeys / 4) * CH; id += NTHR) {
    const int kg = id / CH, c = id % CH;        // keys k0 + 4 kg .. + 3, head-dim elements 8 c .. 8 c + 7
    f16x8 vv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kr = k0 + kg * 4 + j;
      const f16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
      vv[j] = (kr < seq) ? *reinterpret_cast<const f16x8*>(base + (size_t)kr * row_stride + c * 8 + 2 * hidden) : z;
    }
    int pos = kg * 4;
    if constexpr (PERM32) {
      const int kk = pos & 31;
      pos = (pos & ~31) + ((kk & 15) >> 2) * 8 + (kk >> 4) * 4;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e)
      *reinterpret_cast<f16x4*>(&sVt[(c * 8 + e) * VROW + pos]) = f16x4{vv[0][e], vv[1][e], vv[2][e], vv[3][e]};
  }
}

// Scale by inv and store the O^T tiles of query row qr (this lane's column): head-dim columns 16 n + 4 g .. + 4, 8-byte stores.
// (inv: the reciprocal of the row sum; Window mode passes 0 for a row without any allowed key)
// hidden: the width of a ctx row (the causal kernel: query heads x head_dim)
template <int HD>
__device__ __forceinline__ void store_o(const f32x4 (&o)[HD / 16], float inv, _Float16* __restrict__ ctx, int b, int h, int qr,
                                        int seq, int hidden, int g) {
  constexpr int NT = HD / 16;
  if (qr < seq) {
    _Float16* dst = ctx + ((size_t)b * seq + qr) * hidden + h * HD;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const f16x4 v = {(_Float16)(o[n][0] * inv), (_Float16)(o[n][1] * inv), (_Float16)(o[n][2] * inv), (_Float16)(o[n][3] * inv)};
      *reinterpret_cast<f16x4*>(dst + n * 16 + 4 * g) = v;
    }
  }
}

}  // namespace
}  // namespace crs
