// enc_attn.hip -- K3: padding-masked, non-causal self-attention for the encoder (gfx950).
//
//   ctx[b, s, h*hd : (h+1)*hd] = softmax(Q K^T / sqrt(hd) + mask) V        (per batch b, head h)
//
// Flash-style, computed transposed (S^T = K Q^T, O^T = V^T P^T: see the kernel): one 256-thread workgroup per
// (64 query rows, head, batch); wave w owns 16 query rows and keeps their Q fragments, running max / sum and the
// O^T accumulators in registers.
// Keys are visited in blocks of 64: K is staged row-major and V TRANSPOSED in LDS so that both
// MFMA B operands are 8-byte contiguous reads; scores never leave the chip.  S = Q K^T and
// O += P V run on v_mfma_f32_16x16x16_f16 (head_dim 16 / 32 / 64 are whole multiples of its K);
// P goes through a per-wave LDS tile to turn the accumulator layout into the A-operand layout.
// Softmax is fp32 with the usual online rescaling.  Sequences are right-padded: keys >= lens[b]
// get -1e30 before the max (every row sees key 0, so the max is always finite).
// <= 11 % of the encoder's FLOPs at the BASELINE shapes.
// attention_window_kernel: the blocked kernel restricted to the keys with |key - query| <= window (ModernBERT's sliding layers);
// there the claim about key 0 does NOT hold -- see its header for the sentinel and the zero rows.

#include "enc.h"

#include <stdlib.h>

#include <type_traits>

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

// One online-softmax step for this lane's query over the 16 scores it holds of a 64-key block (raw Q.K products of keys
// key0 + 16 ct + i in s).  Works in the base-2 domain with the 1/sqrt(hd) scale folded into one constant c = log2(e) / sqrt(hd).
// Keys >= len (right padding, last block only) are set to -1e30 before the max, so their weight is exp2(-huge) = 0; every
// query sees key 0, so the running max is finite.  The two arms round differently and each keeps its own form:
//   plain  per score a max on the raw product, one fma and one v_exp_f32 (the softmax, not the MFMAs, bounds this kernel: 16
//          scores per lane and block against 16 small MFMAs per wave);
//   BIAS   bias = this lane's window of the staged table (entry 16 ct + i belongs to that key, already times log2(e)):
//          t = s * c + bias first, and the max is taken AFTER the bias is added (the bias can outweigh the product).
template <bool BIAS>
__device__ __forceinline__ void softmax_step(f32x4 (&s)[4], const float* __restrict__ bias, int key0, int len, float c,
                                             float& m_run, float& l_run, float& alpha, f16x4 (&pf)[4]) {
  if constexpr (BIAS) {
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) s[ct][i] = fmaf(s[ct][i], c, bias[ct * 16 + i]);
  }
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
  float mn;
  if constexpr (BIAS) mn = fmaxf(m_run, mx); else mn = fmaxf(m_run, mx * c);
  alpha = __builtin_amdgcn_exp2f(m_run - mn);
  m_run = mn;
  float rs = 0.f;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float p;
      if constexpr (BIAS) p = __builtin_amdgcn_exp2f(s[ct][i] - mn); else p = __builtin_amdgcn_exp2f(fmaf(s[ct][i], c, -mn));
      rs += p;
      pf[ct][i] = (_Float16)p;
    }
  }
  rs += __shfl_xor(rs, 16);
  rs += __shfl_xor(rs, 32);
  l_run = l_run * alpha + rs;
}

// ---- the steps every kernel below is composed from (base = the (batch, head)'s Q column block of qkv; K at + hidden, V at
// + 2 hidden; rows >= seq read as zero)

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

// Normalise and store the O^T tiles of query row qr (this lane's column): head-dim columns 16 n + 4 g .. + 4, 8-byte stores.
// (inv: the reciprocal of the row sum; the windowed kernel passes 0 for a row without any allowed key)
template <int HD>
__device__ __forceinline__ void store_o_scaled(const f32x4 (&o)[HD / 16], float inv, _Float16* __restrict__ ctx, int b, int h, int qr,
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

template <int HD>
__device__ __forceinline__ void store_o(const f32x4 (&o)[HD / 16], float l_run, _Float16* __restrict__ ctx, int b, int h, int qr,
                                        int seq, int hidden, int g) {
  store_o_scaled<HD>(o, 1.0f / l_run, ctx, b, h, qr, seq, hidden, g);
}

// (batch, head) unit of a whole-sequence workgroup.  Workgroups go round-robin over the 8 XCDs (id % 8), and two heads that are
// neighbours in a token's Q / K / V row share 128-byte lines when head_dim is 32: units 2p and 2p + 1 are given to the SAME
// XCD back to back (ids 16 j + x and 16 j + 8 + x), so the second one's K / V come out of that XCD's L2.
__device__ __forceinline__ int xcd_paired_unit(int id, int total) {
  return (total & 15) == 0 ? (((id >> 4) << 3) + (id & 7)) * 2 + ((id >> 3) & 1) : id;
}

// BIAS: an additive relative-position bias on every score,
//   ctx[b, s, h*hd : (h+1)*hd] = softmax(Q K^T / sqrt(hd) + bias[h][key - query] + mask) V
// (what MPNet's layers compute; the bias arrives RESOLVED per offset -- fp32 rel_bias[heads][2 span - 1], entry
// (key - query) + span - 1, span >= seq -- so the bucket rule stays on the host).  The workgroup stages its head's bias
// once: sBias[j] holds log2(e) * bias[h][j - (SP - 1)] for the offsets |j - (SP - 1)| < seq and 0 beyond, SP = seq rounded
// up to 64 -- every (query, key) pair of the padded tiles indexes inside the array, no clamp in the loop.  Everything else,
// the fp16 rounding points included, is the plain kernel; + 4 KB of LDS.  Without BIAS rel_bias and span are not read.
template <int HD, bool BIAS>
__global__ __launch_bounds__(kThreads) void attention_kernel(const _Float16* __restrict__ qkv,
                                                            const int* __restrict__ lens,
                                                            _Float16* __restrict__ ctx, int seq, int hidden,
                                                            const float* __restrict__ rel_bias, int span) {
  constexpr int KS = HD / 16;          // k-steps of the Q K^T contraction
  constexpr int NT = HD / 16;          // 16-row tiles of O^T (head-dim index)
  constexpr int KROW = HD + 4;         // padded K row (halves)
  constexpr int VROW = KB + 4;         // padded V^T row (halves)
  __shared__ __attribute__((aligned(16))) _Float16 sK[KB * KROW];
  __shared__ __attribute__((aligned(16))) _Float16 sVt[HD * VROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int q0 = blockIdx.x * QB + wave * 16;
  const int len = min(max(lens[b], 1), seq);
  const size_t row_stride = (size_t)3 * hidden;
  const _Float16* base = qkv + (size_t)b * seq * row_stride + h * HD;
  const float scale = kLog2e / sqrtf((float)HD);   // log2(e) / sqrt(hd): softmax_step works in base 2

  const float* bias = nullptr;          // BIAS: this lane's window of the staged table at key block 0
  if constexpr (BIAS) {
    // ---- stage the head's bias, times log2(e): offsets -(SP - 1) .. SP - 1, zero where no (query, key) pair of real rows
    // has that offset (|offset| >= seq: rows of the padded tiles only).  Visible to every wave after the first barrier of
    // the key loop (len >= 1: the loop runs at least once).
    __shared__ float sBias[2 * kMaxSeq];
    const int sp = (seq + KB - 1) / KB * KB;         // <= 512: the launcher checks seq
    const float* hb = rel_bias + (size_t)h * (2 * span - 1) + (span - 1);     // offset 0 of this head
    for (int j = tid; j < 2 * sp - 1; j += kThreads) {
      const int d = j - (sp - 1);
      sBias[j] = (d > -seq && d < seq) ? hb[d] * kLog2e : 0.f;
    }
    // this lane's keys of block kb are kb + 4 g + 16 ct + i, its query q0 + lr: staged entry (key - query) + sp - 1.
    // q0 + lr <= sp - 1 and key <= sp - 1, so the entries are within [0, 2 sp - 2]
    bias = sBias + (4 * g - (q0 + lr) + sp - 1);
  }

  // Everything is computed TRANSPOSED: S^T = K Q^T and O^T = V^T P^T.  With the 16x16x16 accumulator layout
  // (column = lane & 15, rows 4 (lane >> 4) + i) a lane then holds the scores of ONE query (lane & 15) for 16
  // keys per block, so the softmax row reductions are 15 register ops + two cross-lane steps instead of four
  // shuffle steps per row, the per-query rescaling is a per-lane scalar, and P^T leaves the accumulators in
  // exactly the B-operand layout of the second product (4 consecutive keys of one query): no LDS round trip
  // for P.
  f16x4 qf[KS];
  load_q_frags<KS>(qf, base, row_stride, q0 + lr, seq, g);
  f32x4 o[NT];                          // O^T tile n: rows = head-dim 16 n + 4 g + i, column = query lr
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;   // of this lane's query

  for (int kb = 0; kb < len; kb += KB) {
    __syncthreads();  // previous block's K / V^T fully consumed
    stage_k<HD, KROW, kThreads>(sK, base, row_stride, hidden, seq, kb, KB, tid);
    stage_vt<HD, VROW, kThreads, false>(sVt, base, row_stride, hidden, seq, kb, KB, tid);
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
    softmax_step<BIAS>(s, BIAS ? bias + kb : nullptr, kb + 4 * g, len, scale, m_run, l_run, alpha, pf);
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
  store_o<HD>(o, l_run, ctx, b, h, q0 + lr, seq, hidden, g);
}

// ---------------------------------------------------------------------------------------------------------------
// Sliding-window variant of the blocked kernel (ModernBERT's local layers): query q attends the keys with |key - q| <= window
// (both ends included) and key < len,
//   ctx[b, q, h*hd : (h+1)*hd] = softmax_{|j - q| <= W, j < len}(Q K^T / sqrt(hd)) V
// Same staging, MFMA shape, fp16 rounding points and online softmax as attention_kernel<HD, false>; a workgroup of 64 queries
// starting at qb walks only the 64-key blocks that meet [max(0, qb - W), min(len, qb + 64 + W)): at most 2 + ceil(2 W / 64) of
// them, whatever the sequence length, and none where that range is empty (qb - W >= len).  Inside a visited block a score outside the window or at key >= len gets the padding
// treatment (-1e30, weight 0); a block that lies wholly inside the window of all 16 queries of the wave and below len skips the test.
// Two things the plain kernel's comments rule out happen here:
//   * a query's FIRST visited block can lie wholly outside its window (W = 8: rows 73 .. 127 of query block 1 against key block 0),
//     so "every row sees key 0, the max is finite" does not hold.  The running maximum then stays at the sentinel -1e30 and that
//     block's weights are exp2(-1e30 - -1e30) = 1, on finite V values; the first block with an allowed key rescales by
//     exp2(-1e30 - finite) = 0 exactly, which wipes the accumulator and the row sum.  That needs the masked score, the maximum and
//     the subtraction to be the SAME fp32 number: the step scales first (t = s c) and masks t, instead of masking the raw product and
//     folding c into an fma as the plain step does -- fma(-1e30, c, fl(1e30 c)) is the product's rounding error, about 2^70, and
//     exp2 of that is infinity.  The sentinel is finite on purpose: with -inf the same subtraction is inf - inf = NaN.
//   * a padding query at q >= len + W has no allowed key at all (and a workgroup whose whole query block is such visits no block).
//     Its row is written as ZEROS: the row sum would be 0 or a count of masked keys, and a NaN there would poison real rows in
//     the next layer's MFMAs (0 x NaN) although their weight for this position is 0.  Every real query allows itself.
__device__ __forceinline__ void softmax_step_window(f32x4 (&s)[4], int key0, int q, int window, int len, bool inside, float c,
                                                    float& m_run, float& l_run, float& alpha, f16x4 (&pf)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) s[ct][i] *= c;
  if (!inside) {                            // wave-uniform
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = key0 + ct * 16 + i, d = key - q;
        if (key >= len || d > window || d < -window) s[ct][i] = -1e30f;
      }
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
__global__ __launch_bounds__(kThreads) void attention_window_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ lens,
                                                                   _Float16* __restrict__ ctx, int seq, int hidden, int window) {
  constexpr int KS = HD / 16, NT = HD / 16;
  constexpr int KROW = HD + 4, VROW = KB + 4;
  __shared__ __attribute__((aligned(16))) _Float16 sK[KB * KROW];
  __shared__ __attribute__((aligned(16))) _Float16 sVt[HD * VROW];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int b = blockIdx.z, h = blockIdx.y;
  const int qb = blockIdx.x * QB, q0 = qb + wave * 16;
  const int len = min(max(lens[b], 1), seq);
  const int w = min(window, seq);                  // (|key - query| < seq anyway; keeps the sums below in range)
  const size_t row_stride = (size_t)3 * hidden;
  const _Float16* base = qkv + (size_t)b * seq * row_stride + h * HD;
  const float scale = kLog2e / sqrtf((float)HD);
  // the workgroup's key blocks (the same for its four waves: the barriers below are uniform)
  // (a query block wholly behind len + w -- qb - w >= len -- has no allowed key at all and walks no block)
  const int k_lo = max(0, qb - w) & ~(KB - 1), k_hi = qb - w >= len ? 0 : min(len, qb + QB + w);

  f16x4 qf[KS];
  load_q_frags<KS>(qf, base, row_stride, q0 + lr, seq, g);
  f32x4 o[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;

  for (int kb = k_lo; kb < k_hi; kb += KB) {
    __syncthreads();
    stage_k<HD, KROW, kThreads>(sK, base, row_stride, hidden, seq, kb, KB, tid);
    stage_vt<HD, VROW, kThreads, false>(sVt, base, row_stride, hidden, seq, kb, KB, tid);
    __syncthreads();
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
    // all 64 keys allowed for all 16 queries of the wave: kb >= (q0 + 15) - w, kb + 63 <= q0 + w, kb + 64 <= len
    const bool inside = kb + w >= q0 + 15 && kb + KB - 1 <= q0 + w && kb + KB <= len;
    float alpha;
    f16x4 pf[4];
    softmax_step_window(s, kb + 4 * g, q0 + lr, w, len, inside, scale, m_run, l_run, alpha, pf);
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
  // a row whose maximum is still the sentinel saw no allowed key (finite scores are far above -1e29): zeros
  store_o_scaled<HD>(o, m_run > -1e29f ? 1.0f / l_run : 0.f, ctx, b, h, q0 + lr, seq, hidden, g);
}

// ---------------------------------------------------------------------------------------------------------------
// Whole-sequence variant (index build): one workgroup per (batch, head) stages K and V^T of the WHOLE sequence once
// (head_dim 32, <= 256 tokens: 18 + 17 KB of LDS, four waves; head_dim 64, <= 512 tokens: 70 + 66 KB, eight waves; one
// barrier) and its waves walk the query tiles (16 queries each: tiles w, w + NW, ...) over all key blocks without
// further barriers.
// The kernel above gives each 64-query block its own workgroup, which re-stages the same K / V per query block and
// pays two barriers and an unprefetched global round trip per 64 keys -- at 256-token sequences four times the loads
// and eight barriers for 16 small MFMAs per block.  Arithmetic, masking and output are identical (same accumulation
// order per query), so the results are bit-equal to the blocked kernel's.
template <int HD, int SMAX, int NW>
__global__ __launch_bounds__(NW * 64) void attention_seq_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ lens,
                                                               _Float16* __restrict__ ctx, int seq, int hidden) {
  constexpr int KS = HD / 16, NT = HD / 16;
  constexpr int KROW = HD + 4, VROW = SMAX + 4;
  constexpr int kThreads = NW * 64;
  extern __shared__ __attribute__((aligned(16))) char attn_smem[];
  _Float16* sK = reinterpret_cast<_Float16*>(attn_smem);                       // [SMAX][KROW]
  _Float16* sVt = sK + SMAX * KROW;                                            // [HD][VROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int heads = hidden / HD;
  const int unit = xcd_paired_unit(blockIdx.x, gridDim.x);
  const int b = unit / heads, h = unit % heads;
  const int len = min(max(lens[b], 1), seq);
  const size_t row_stride = (size_t)3 * hidden;
  const _Float16* base = qkv + (size_t)b * seq * row_stride + h * HD;
  const float scale = kLog2e / sqrtf((float)HD);   // log2(e) / sqrt(hd): softmax_step works in base 2
  const int kend = (len + KB - 1) / KB * KB;       // keys staged: whole 64-key blocks up to len (rows >= seq are zero)

  stage_k<HD, KROW, kThreads>(sK, base, row_stride, hidden, seq, 0, kend, tid);
  stage_vt<HD, VROW, kThreads, false>(sVt, base, row_stride, hidden, seq, 0, kend, tid);
  __syncthreads();

  for (int q0 = wave * 16; q0 < seq; q0 += NW * 16) {
    f16x4 qf[KS];
    load_q_frags<KS>(qf, base, row_stride, q0 + lr, seq, g);
    f32x4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;
    for (int kb = 0; kb < len; kb += KB) {
      f32x4 sc[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        sc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const f16x4 kf = *reinterpret_cast<const f16x4*>(&sK[(kb + ct * 16 + lr) * KROW + ks * 16 + g * 4]);
          sc[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[ks], sc[ct], 0, 0, 0);
        }
      }
      float alpha;
      f16x4 pf[4];
      softmax_step<false>(sc, nullptr, kb + 4 * g, len, scale, m_run, l_run, alpha, pf);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[n][i] *= alpha;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[(n * 16 + lr) * VROW + kb + ct * 16 + g * 4]);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[ct], o[n], 0, 0, 0);
        }
      }
    }
    store_o<HD>(o, l_run, ctx, b, h, q0 + lr, seq, hidden, g);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 3: the whole-sequence kernel on v_mfma_f32_16x16x32_f16 with QT query tiles per wave (index build, head_dim 32 / 64).
// The kernel above reads an 8-byte K or V^T fragment from LDS for EVERY 16x16x16 MFMA and uses it for one 16-query tile:
// 16 flops per LDS byte, i.e. the LDS port bounds it at half the matrix pipe's rate before any latency shows (measured:
// 170 TFLOP/s on bge-base's 512-token sequences, 21 % of the index build).  Here
//   * a wave owns QT = 2 query tiles (32 queries): a fragment is read once (ds_read_b128, 16 bytes per lane) and feeds
//     QT MFMAs of twice the depth -- 4 x fewer LDS instructions per flop;
//   * S^T = K Q^T contracts 32 head-dim elements per MFMA (K rows in natural order: lane = key row, 8 elements of the step);
//   * O^T += V^T P^T contracts 32 KEYS per MFMA.  P^T leaves the score accumulators as 4 consecutive keys of a 16-key tile
//     per lane; two tiles (2 s, 2 s + 1) side by side ARE a lane's 8 k-values of the 32-key step if k is numbered
//     (lane group g, tile, i) instead of key order -- any order works as long as V^T uses the same one, so V^T is STAGED
//     with its keys permuted inside every 32-key group: position = 8 (key % 16 / 4) + 4 (key / 16 % 2) + key % 4.
//     No shuffle, no LDS round trip for P;
//   * row pitches HD + 8 and SMAX + 8 halves: 16-byte aligned rows whose 16 lanes land on 16 distinct 4-bank groups.
// Same masking, scaling and online softmax (softmax_step, per query tile); accumulation ORDER differs from the kernel above
// (32-deep products), so results agree to fp32 rounding, not bit for bit.
template <int HD, int SMAX, int NW, int QT>
__global__ __launch_bounds__(NW * 64) void attention_seq32_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ lens,
                                                                 _Float16* __restrict__ ctx, int seq, int hidden) {
  constexpr int KS = HD / 32, NT = HD / 16;
  constexpr int KROW = HD + 8, VROW = SMAX + 8;
  constexpr int kThr = NW * 64;
  extern __shared__ __attribute__((aligned(16))) char attn_smem[];
  _Float16* sK = reinterpret_cast<_Float16*>(attn_smem);                       // [SMAX][KROW]
  _Float16* sVt = sK + SMAX * KROW;                                            // [HD][VROW], keys permuted per 32-key group
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int heads = hidden / HD;
  const int unit = xcd_paired_unit(blockIdx.x, gridDim.x);
  const int b = unit / heads, h = unit % heads;
  const int len = min(max(lens[b], 1), seq);
  const size_t row_stride = (size_t)3 * hidden;
  const _Float16* base = qkv + (size_t)b * seq * row_stride + h * HD;
  const float scale = kLog2e / sqrtf((float)HD);
  const int kend = (len + KB - 1) / KB * KB;

  stage_k<HD, KROW, kThr>(sK, base, row_stride, hidden, seq, 0, kend, tid);          // (16-byte rows: whole-chunk stores)
  stage_vt<HD, VROW, kThr, true>(sVt, base, row_stride, hidden, seq, 0, kend, tid);  // (keys permuted per 32-key group)
  __syncthreads();

  for (int q0 = wave * (16 * QT); q0 < seq; q0 += NW * 16 * QT) {
    f16x8 qf[QT][KS];
#pragma unroll
    for (int t = 0; t < QT; ++t) load_q_frags<KS>(qf[t], base, row_stride, q0 + t * 16 + lr, seq, g);
    f32x4 o[QT][NT];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      m_run[t] = -1e30f;
      l_run[t] = 0.f;
#pragma unroll
      for (int n = 0; n < NT; ++n) o[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int kb = 0; kb < len; kb += KB) {
      f32x4 sc[QT][4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
        for (int t = 0; t < QT; ++t) sc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const f16x8 kf = *reinterpret_cast<const f16x8*>(&sK[(kb + ct * 16 + lr) * KROW + ks * 32 + g * 8]);
#pragma unroll
          for (int t = 0; t < QT; ++t) sc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[t][ks], sc[t][ct], 0, 0, 0);
        }
      }
      f16x8 pb[QT][2];      // P^T as B operands of the two 32-key steps: (tile 2 s, tile 2 s + 1) side by side
#pragma unroll
      for (int t = 0; t < QT; ++t) {
        float alpha;
        f16x4 pf[4];
        softmax_step<false>(sc[t], nullptr, kb + 4 * g, len, scale, m_run[t], l_run[t], alpha, pf);
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
          pb[t][s2] = f16x8{pf[2 * s2][0], pf[2 * s2][1], pf[2 * s2][2], pf[2 * s2][3],
                            pf[2 * s2 + 1][0], pf[2 * s2 + 1][1], pf[2 * s2 + 1][2], pf[2 * s2 + 1][3]};
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
          for (int i = 0; i < 4; ++i) o[t][n][i] *= alpha;
      }
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          const f16x8 vf = *reinterpret_cast<const f16x8*>(&sVt[(n * 16 + lr) * VROW + kb + s2 * 32 + g * 8]);
#pragma unroll
          for (int t = 0; t < QT; ++t) o[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[t][s2], o[t][n], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) store_o<HD>(o[t], l_run[t], ctx, b, h, q0 + t * 16 + lr, seq, hidden, g);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Round 3: query-length sequences (<= 16 tokens, head_dim 32 / 64): one WAVE per (sequence, head), no workgroup barrier.
// The blocked kernel gives a 64-query block to four waves: at 16 tokens three of them idle through the staging and the barriers
// (bge-base over eight C3 batches: 24 576 (sequence, head) units = 24 576 workgroups; 163 us per layer in the mix).  Here a wave
// loads its unit's Q and K rows as MFMA fragments straight from global memory (16-byte loads), S^T = K Q^T is HD / 32 MFMAs of
// 16x16x32, the softmax over the 16 keys is four values per lane + two cross-lane steps, V goes through a wave-private 2.5 KB
// LDS tile to become V^T fragments, O^T = V^T P^T is HD / 16 MFMAs of 16x16x16 with P^T straight from the score registers.
template <int HD>
__global__ __launch_bounds__(256) void attention_short_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ lens,
                                                             _Float16* __restrict__ ctx, int seq, int hidden, int n_units) {
  constexpr int KS = HD / 32, NT = HD / 16, VROW = 20;        // V^T rows of 16 keys + 4 halves of padding (8-byte aligned rows)
  __shared__ __attribute__((aligned(16))) _Float16 sVt[4][HD * VROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, g = lane >> 4;
  const int unit = blockIdx.x * 4 + wave;
  if (unit >= n_units) return;                                 // (no workgroup barrier below)
  const int heads = hidden / HD;
  const int b = unit / heads, h = unit % heads;
  const int len = min(max(lens[b], 1), seq);
  const size_t row_stride = (size_t)3 * hidden;
  const _Float16* base = qkv + (size_t)b * seq * row_stride + h * HD;
  const float c = 1.44269504088896341f / sqrtf((float)HD);     // log2(e) / sqrt(hd)
  const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 sc = {0.f, 0.f, 0.f, 0.f};                             // S^T: rows = keys 4 g + i, column = query lr
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const _Float16* rowp = base + (size_t)lr * row_stride + ks * 32 + g * 8;
    const f16x8 qf = (lr < seq) ? *reinterpret_cast<const f16x8*>(rowp) : z8;
    const f16x8 kf = (lr < seq) ? *reinterpret_cast<const f16x8*>(rowp + hidden) : z8;
    sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, sc, 0, 0, 0);
  }
  // V rows -> V^T in this wave's LDS tile: lane (key = lane >> 2, quarter = lane & 3) takes HD / 4 head-dim elements of its key
  {
    const int key = lane >> 2, qt = lane & 3;
    constexpr int PER = HD / 4;                                // 16 (head_dim 64) or 8 (32) elements per lane
#pragma unroll
    for (int u = 0; u < PER / 8; ++u) {
      const f16x8 v = (key < seq) ? *reinterpret_cast<const f16x8*>(base + (size_t)key * row_stride + 2 * hidden + qt * PER + u * 8) : z8;
#pragma unroll
      for (int e = 0; e < 8; ++e) sVt[wave][(qt * PER + u * 8 + e) * VROW + key] = v[e];
    }
  }
  // softmax over the keys of query lr (keys >= len masked; key 0 is always real, so the maximum is finite)
  float mx = -1e30f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (4 * g + i >= len) sc[i] = -1e30f;
    mx = fmaxf(mx, sc[i]);
  }
  mx = fmaxf(mx, __shfl_xor(mx, 16));
  mx = fmaxf(mx, __shfl_xor(mx, 32));
  const float mn = mx * c;
  float rs = 0.f;
  f16x4 pf;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float p = __builtin_amdgcn_exp2f(fmaf(sc[i], c, -mn));
    rs += p;
    pf[i] = (_Float16)p;
  }
  rs += __shfl_xor(rs, 16);
  rs += __shfl_xor(rs, 32);
  __builtin_amdgcn_wave_barrier();                             // the wave's V^T stores precede its fragment reads (LDS ops of one wave stay in order)
  const float inv = 1.0f / rs;
  // (every lane multiplies: as A operand lane lr is head-dim row 16 n + lr of V^T, whatever the sequence length; only the store
  // -- column = query lr -- depends on it)
  _Float16* dst = ctx + ((size_t)b * seq + (lr < seq ? lr : 0)) * hidden + h * HD;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[wave][(n * 16 + lr) * VROW + 4 * g]);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    o = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf, o, 0, 0, 0);
    const f16x4 ov = {(_Float16)(o[0] * inv), (_Float16)(o[1] * inv), (_Float16)(o[2] * inv), (_Float16)(o[3] * inv)};
    if (lr < seq) *reinterpret_cast<f16x4*>(dst + n * 16 + 4 * g) = ov;
  }
}

}  // namespace

int attention_launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int batch, int seq, int hidden, int heads,
                     const float* rel_bias, int span, hipStream_t stream) {
  const dim3 grid(p.d.gx, p.d.gy, p.d.gz);
  auto blocked = [&](auto with_bias) -> int {
    constexpr bool BIAS = decltype(with_bias)::value;
    switch (p.hd) {
      case 16: hipLaunchKernelGGL((attention_kernel<16, BIAS>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, rel_bias, span); break;
      case 32: hipLaunchKernelGGL((attention_kernel<32, BIAS>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, rel_bias, span); break;
      case 64: hipLaunchKernelGGL((attention_kernel<64, BIAS>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, rel_bias, span); break;
      default: return -1;
    }
    return (int)hipGetLastError();
  };
  auto whole = [&](auto kernel) -> int {   // whole sequence per workgroup
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, p.d.lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, grid, dim3(p.d.threads), p.d.lds, stream, qkv, lens, ctx, seq, hidden);
    return (int)hipGetLastError();
  };
  const auto is = [&](int hd, int smax, int qt) { return p.hd == hd && p.smax == smax && p.qt == qt; };   // the instantiations
  switch (p.form) {
    case AttnForm::Blocked:
      if (!p.bias) return blocked(std::false_type{});
      if (!rel_bias || seq < 1 || seq > kMaxSeq || span < seq || batch < 1 || batch > 65535) return -1;
      return blocked(std::true_type{});
    case AttnForm::Short: {
      const int units = heads * batch;
      if (p.hd == 32) hipLaunchKernelGGL((attention_short_kernel<32>), grid, dim3(256), 0, stream, qkv, lens, ctx, seq, hidden, units);
      else hipLaunchKernelGGL((attention_short_kernel<64>), grid, dim3(256), 0, stream, qkv, lens, ctx, seq, hidden, units);
      return (int)hipGetLastError();
    }
    case AttnForm::Seq32:
      if (is(32, 256, 4)) return whole(&attention_seq32_kernel<32, 256, 4, 4>);
      if (is(64, 512, 4)) return whole(&attention_seq32_kernel<64, 512, 8, 4>);
      if (is(32, 256, 2)) return whole(&attention_seq32_kernel<32, 256, 4, 2>);
      if (is(64, 512, 2)) return whole(&attention_seq32_kernel<64, 512, 8, 2>);
      if (is(64, 256, 2)) return whole(&attention_seq32_kernel<64, 256, 4, 2>);
      return -1;
    case AttnForm::Seq:
      if (is(32, 256, 0)) return whole(&attention_seq_kernel<32, 256, 4>);
      if (is(16, 256, 0)) return whole(&attention_seq_kernel<16, 256, 4>);
      if (is(64, 512, 0)) return whole(&attention_seq_kernel<64, 512, 8>);
      if (is(64, 256, 0)) return whole(&attention_seq_kernel<64, 256, 4>);
      return -1;
    default: return -1;
  }
}

int attention_window_launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int seq, int hidden, hipStream_t stream) {
  if (p.form != AttnForm::Window || p.window < 1) return -1;
  const dim3 grid(p.d.gx, p.d.gy, p.d.gz);
  switch (p.hd) {
    case 16: hipLaunchKernelGGL((attention_window_kernel<16>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, p.window); break;
    case 32: hipLaunchKernelGGL((attention_window_kernel<32>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, p.window); break;
    case 64: hipLaunchKernelGGL((attention_window_kernel<64>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, p.window); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace crs
