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
//
// The steps the five kernels are composed from exist once: softmax_step<Score> (the online-softmax step in its three score modes:
// Plain -- padding mask only, Bias -- MPNet's relative-position bias, Window -- ModernBERT's sliding layers, only the keys with
// |key - query| <= window; in Window mode the claim about key 0 does NOT hold, see the step for the sentinel and the zero rows),
// make_unit (a (batch, head)'s setup), load_q_frags, stage_k, stage_vt and store_o.
// The 64-key block step on the 16-deep MFMA (S^T MFMAs, softmax_step, rescale, O^T MFMAs) is still written out in attention_kernel,
// attention_window_kernel and attention_seq_kernel: sharing it, or the blocked body, moved s_waitcnt counts in the compiled
// kernels (profiles/attn_refactor_resources.txt has the lines), so each keeps its copy and the bit-equality of the three rests on
// tests/test_attn_forms_gpu.py and tools/encoder_digest.py.

#include "enc.h"
#include "enc_attn_steps.h"

#include <stdlib.h>

#include <type_traits>

namespace crs {
namespace {

// softmax_step, load_q_frags, stage_k, stage_vt, store_o and the constants: enc_attn_steps.h (shared with enc_attn_causal.hip)

// (batch, head) unit of a whole-sequence workgroup.  Workgroups go round-robin over the 8 XCDs (id % 8), and two heads that are
// neighbours in a token's Q / K / V row share 128-byte lines when head_dim is 32: units 2p and 2p + 1 are given to the SAME
// XCD back to back (ids 16 j + x and 16 j + 8 + x), so the second one's K / V come out of that XCD's L2.
__device__ __forceinline__ int xcd_paired_unit(int id, int total) {
  return (total & 15) == 0 ? (((id >> 4) << 3) + (id & 7)) * 2 + ((id >> 3) & 1) : id;
}

// What a workgroup (or, in the short kernel, a wave) knows about its (batch, head) unit and its own lanes.
struct Unit {
  int tid, wave, lr, g;        // thread, wave of the workgroup; lane = 16 g + lr
  int b, h, len;               // len: the real tokens, clamped to [1, seq]
  size_t row_stride;           // of qkv, in halves
  const _Float16* base;        // the unit's Q column block (K at + hidden, V at + 2 hidden)
  float scale;                 // log2(e) / sqrt(hd): softmax_step works in base 2
};

template <int HD>
__device__ __forceinline__ Unit make_unit(const _Float16* qkv, const int* lens, int b, int h, int seq, int hidden) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int len = min(max(lens[b], 1), seq);
  const size_t row_stride = (size_t)3 * hidden;
  return Unit{tid, tid >> 6, lane & 15, lane >> 4, b, h, len, row_stride, qkv + (size_t)b * seq * row_stride + h * HD,
              kLog2e / sqrtf((float)HD)};
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

  const Unit u = make_unit<HD>(qkv, lens, blockIdx.z, blockIdx.y, seq, hidden);
  const int q0 = blockIdx.x * QB + u.wave * 16;

  const float* bias = nullptr;          // BIAS: this lane's window of the staged table at key block 0
  if constexpr (BIAS) {
    // ---- stage the head's bias, times log2(e): offsets -(SP - 1) .. SP - 1, zero where no (query, key) pair of real rows
    // has that offset (|offset| >= seq: rows of the padded tiles only).  Visible to every wave after the first barrier of
    // the key loop (len >= 1: the loop runs at least once).
    __shared__ float sBias[2 * kMaxSeq];
    const int sp = (seq + KB - 1) / KB * KB;         // <= 512: the launcher checks seq
    const float* hb = rel_bias + (size_t)u.h * (2 * span - 1) + (span - 1);     // offset 0 of this head
    for (int j = u.tid; j < 2 * sp - 1; j += kThreads) {
      const int d = j - (sp - 1);
      sBias[j] = (d > -seq && d < seq) ? hb[d] * kLog2e : 0.f;
    }
    // this lane's keys of block kb are kb + 4 g + 16 ct + i, its query q0 + lr: staged entry (key - query) + sp - 1.
    // q0 + lr <= sp - 1 and key <= sp - 1, so the entries are within [0, 2 sp - 2]
    bias = sBias + (4 * u.g - (q0 + u.lr) + sp - 1);
  }

  // Everything is computed TRANSPOSED: S^T = K Q^T and O^T = V^T P^T.  With the 16x16x16 accumulator layout
  // (column = lane & 15, rows 4 (lane >> 4) + i) a lane then holds the scores of ONE query (lane & 15) for 16
  // keys per block, so the softmax row reductions are 15 register ops + two cross-lane steps instead of four
  // shuffle steps per row, the per-query rescaling is a per-lane scalar, and P^T leaves the accumulators in
  // exactly the B-operand layout of the second product (4 consecutive keys of one query): no LDS round trip
  // for P.
  f16x4 qf[KS];
  load_q_frags<KS>(qf, u.base, u.row_stride, q0 + u.lr, seq, u.g);
  f32x4 o[NT];                          // O^T tile n: rows = head-dim 16 n + 4 g + i, column = query lr
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;   // of this lane's query

  for (int kb = 0; kb < u.len; kb += KB) {
    __syncthreads();  // previous block's K / V^T fully consumed
    stage_k<HD, KROW, kThreads>(sK, u.base, u.row_stride, hidden, seq, kb, KB, u.tid);
    stage_vt<HD, VROW, kThreads, false>(sVt, u.base, u.row_stride, hidden, seq, kb, KB, u.tid);
    __syncthreads();

    // ---- S^T = K Q^T for 4 tiles of 16 keys: lane holds keys kb + 16 ct + 4 g + i of query lr
    f32x4 s[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      s[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x4 kf = *reinterpret_cast<const f16x4*>(&sK[(ct * 16 + u.lr) * KROW + ks * 16 + u.g * 4]);
        s[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[ks], s[ct], 0, 0, 0);
      }
    }
    float alpha;
    f16x4 pf[4];
    softmax_step<BIAS ? Score::Bias : Score::Plain>(s, KeyMask{u.len, BIAS ? bias + kb : nullptr, 0, 0, false}, kb + 4 * u.g, u.scale, m_run, l_run, alpha, pf);
    // ---- O^T = O^T alpha + V^T P^T   (A = V^T[hd 16 n + lr][key 16 ct + 4 g + j], B = P^T from the registers)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[n][i] *= alpha;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[(n * 16 + u.lr) * VROW + ct * 16 + u.g * 4]);
        o[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[ct], o[n], 0, 0, 0);
      }
    }
  }
  store_o<HD>(o, 1.0f / l_run, ctx, u.b, u.h, q0 + u.lr, seq, hidden, u.g);
}

// ---------------------------------------------------------------------------------------------------------------
// Sliding-window variant of the blocked kernel (ModernBERT's local layers): query q attends the keys with |key - q| <= window
// (both ends included) and key < len,
//   ctx[b, q, h*hd : (h+1)*hd] = softmax_{|j - q| <= W, j < len}(Q K^T / sqrt(hd)) V
// Same staging, MFMA shape and fp16 rounding points as attention_kernel<HD, false>, softmax_step in Window mode; a workgroup of 64
// queries starting at qb walks only the 64-key blocks that meet [max(0, qb - W), min(len, qb + 64 + W)): at most 2 + ceil(2 W / 64)
// of them, whatever the sequence length, and none where that range is empty (qb - W >= len).  Inside a visited block a score outside
// the window or at key >= len gets the padding treatment (-1e30, weight 0); a block that lies wholly inside the window of all 16
// queries of the wave and below len skips the test.  A query's first visited block can lie wholly outside its window, and a padding
// query at q >= len + W has no allowed key at all and is stored as a ZERO row: softmax_step's Window arm has the reasons.
template <int HD>
__global__ __launch_bounds__(kThreads) void attention_window_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ lens,
                                                                   _Float16* __restrict__ ctx, int seq, int hidden, int window) {
  constexpr int KS = HD / 16, NT = HD / 16;
  constexpr int KROW = HD + 4, VROW = KB + 4;
  __shared__ __attribute__((aligned(16))) _Float16 sK[KB * KROW];
  __shared__ __attribute__((aligned(16))) _Float16 sVt[HD * VROW];

  const Unit u = make_unit<HD>(qkv, lens, blockIdx.z, blockIdx.y, seq, hidden);
  const int qb = blockIdx.x * QB, q0 = qb + u.wave * 16;
  const int w = min(window, seq);                  // (|key - query| < seq anyway; keeps the sums below in range)
  // the workgroup's key blocks (the same for its four waves: the barriers below are uniform)
  // (a query block wholly behind len + w -- qb - w >= len -- has no allowed key at all and walks no block)
  const int k_lo = max(0, qb - w) & ~(KB - 1), k_hi = qb - w >= u.len ? 0 : min(u.len, qb + QB + w);

  f16x4 qf[KS];
  load_q_frags<KS>(qf, u.base, u.row_stride, q0 + u.lr, seq, u.g);
  f32x4 o[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -1e30f, l_run = 0.f;

  for (int kb = k_lo; kb < k_hi; kb += KB) {
    __syncthreads();
    stage_k<HD, KROW, kThreads>(sK, u.base, u.row_stride, hidden, seq, kb, KB, u.tid);
    stage_vt<HD, VROW, kThreads, false>(sVt, u.base, u.row_stride, hidden, seq, kb, KB, u.tid);
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      s[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x4 kf = *reinterpret_cast<const f16x4*>(&sK[(ct * 16 + u.lr) * KROW + ks * 16 + u.g * 4]);
        s[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[ks], s[ct], 0, 0, 0);
      }
    }
    // all 64 keys allowed for all 16 queries of the wave: kb >= (q0 + 15) - w, kb + 63 <= q0 + w, kb + 64 <= len
    const bool inside = kb + w >= q0 + 15 && kb + KB - 1 <= q0 + w && kb + KB <= u.len;
    float alpha;
    f16x4 pf[4];
    softmax_step<Score::Window>(s, KeyMask{u.len, nullptr, q0 + u.lr, w, inside}, kb + 4 * u.g, u.scale, m_run, l_run, alpha, pf);
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int i = 0; i < 4; ++i) o[n][i] *= alpha;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[(n * 16 + u.lr) * VROW + ct * 16 + u.g * 4]);
        o[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[ct], o[n], 0, 0, 0);
      }
    }
  }
  // a row whose maximum is still the sentinel saw no allowed key (finite scores are far above -1e29): zeros
  store_o<HD>(o, m_run > -1e29f ? 1.0f / l_run : 0.f, ctx, u.b, u.h, q0 + u.lr, seq, hidden, u.g);
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
  const int heads = hidden / HD;
  const int unit = xcd_paired_unit(blockIdx.x, gridDim.x);
  const Unit u = make_unit<HD>(qkv, lens, unit / heads, unit % heads, seq, hidden);
  const int kend = (u.len + KB - 1) / KB * KB;     // keys staged: whole 64-key blocks up to len (rows >= seq are zero)

  stage_k<HD, KROW, kThreads>(sK, u.base, u.row_stride, hidden, seq, 0, kend, u.tid);
  stage_vt<HD, VROW, kThreads, false>(sVt, u.base, u.row_stride, hidden, seq, 0, kend, u.tid);
  __syncthreads();

  for (int q0 = u.wave * 16; q0 < seq; q0 += NW * 16) {
    f16x4 qf[KS];
    load_q_frags<KS>(qf, u.base, u.row_stride, q0 + u.lr, seq, u.g);
    f32x4 o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) o[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -1e30f, l_run = 0.f;
    for (int kb = 0; kb < u.len; kb += KB) {
      f32x4 sc[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        sc[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
          const f16x4 kf = *reinterpret_cast<const f16x4*>(&sK[(kb + ct * 16 + u.lr) * KROW + ks * 16 + u.g * 4]);
          sc[ct] = __builtin_amdgcn_mfma_f32_16x16x16f16(kf, qf[ks], sc[ct], 0, 0, 0);
        }
      }
      float alpha;
      f16x4 pf[4];
      softmax_step<Score::Plain>(sc, KeyMask{u.len, nullptr, 0, 0, false}, kb + 4 * u.g, u.scale, m_run, l_run, alpha, pf);
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[n][i] *= alpha;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[(n * 16 + u.lr) * VROW + kb + ct * 16 + u.g * 4]);
          o[n] = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf[ct], o[n], 0, 0, 0);
        }
      }
    }
    store_o<HD>(o, 1.0f / l_run, ctx, u.b, u.h, q0 + u.lr, seq, hidden, u.g);
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
  const int heads = hidden / HD;
  const int unit = xcd_paired_unit(blockIdx.x, gridDim.x);
  const Unit u = make_unit<HD>(qkv, lens, unit / heads, unit % heads, seq, hidden);
  const int lr = u.lr, g = u.g;
  const int kend = (u.len + KB - 1) / KB * KB;

  stage_k<HD, KROW, kThr>(sK, u.base, u.row_stride, hidden, seq, 0, kend, u.tid);          // (16-byte rows: whole-chunk stores)
  stage_vt<HD, VROW, kThr, true>(sVt, u.base, u.row_stride, hidden, seq, 0, kend, u.tid);  // (keys permuted per 32-key group)
  __syncthreads();

  for (int q0 = u.wave * (16 * QT); q0 < seq; q0 += NW * 16 * QT) {
    f16x8 qf[QT][KS];
#pragma unroll
    for (int t = 0; t < QT; ++t) load_q_frags<KS>(qf[t], u.base, u.row_stride, q0 + t * 16 + lr, seq, g);
    f32x4 o[QT][NT];
    float m_run[QT], l_run[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      m_run[t] = -1e30f;
      l_run[t] = 0.f;
#pragma unroll
      for (int n = 0; n < NT; ++n) o[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int kb = 0; kb < u.len; kb += KB) {
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
        softmax_step<Score::Plain>(sc[t], KeyMask{u.len, nullptr, 0, 0, false}, kb + 4 * g, u.scale, m_run[t], l_run[t], alpha, pf);
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
    for (int t = 0; t < QT; ++t) store_o<HD>(o[t], 1.0f / l_run[t], ctx, u.b, u.h, q0 + t * 16 + lr, seq, hidden, g);
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
  const int unit = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (unit >= n_units) return;                                 // (no workgroup barrier below)
  const int heads = hidden / HD;
  const Unit u = make_unit<HD>(qkv, lens, unit / heads, unit % heads, seq, hidden);
  const int lane = u.tid & 63, lr = u.lr, g = u.g;
  const float c = u.scale;
  const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 sc = {0.f, 0.f, 0.f, 0.f};                             // S^T: rows = keys 4 g + i, column = query lr
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const _Float16* rowp = u.base + (size_t)lr * u.row_stride + ks * 32 + g * 8;
    const f16x8 qf = (lr < seq) ? *reinterpret_cast<const f16x8*>(rowp) : z8;
    const f16x8 kf = (lr < seq) ? *reinterpret_cast<const f16x8*>(rowp + hidden) : z8;
    sc = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, sc, 0, 0, 0);
  }
  // V rows -> V^T in this wave's LDS tile: lane (key = lane >> 2, quarter = lane & 3) takes HD / 4 head-dim elements of its key
  {
    const int key = lane >> 2, qt = lane & 3;
    constexpr int PER = HD / 4;                                // 16 (head_dim 64) or 8 (32) elements per lane
#pragma unroll
    for (int i = 0; i < PER / 8; ++i) {
      const f16x8 v = (key < seq) ? *reinterpret_cast<const f16x8*>(u.base + (size_t)key * u.row_stride + 2 * hidden + qt * PER + i * 8) : z8;
#pragma unroll
      for (int e = 0; e < 8; ++e) sVt[u.wave][(qt * PER + i * 8 + e) * VROW + key] = v[e];
    }
  }
  // softmax over the keys of query lr (keys >= len masked; key 0 is always real, so the maximum is finite)
  float mx = -1e30f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (4 * g + i >= u.len) sc[i] = -1e30f;
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
  _Float16* dst = ctx + ((size_t)u.b * seq + (lr < seq ? lr : 0)) * hidden + u.h * HD;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const f16x4 vf = *reinterpret_cast<const f16x4*>(&sVt[u.wave][(n * 16 + lr) * VROW + 4 * g]);
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    o = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf, o, 0, 0, 0);
    const f16x4 ov = {(_Float16)(o[0] * inv), (_Float16)(o[1] * inv), (_Float16)(o[2] * inv), (_Float16)(o[3] * inv)};
    if (lr < seq) *reinterpret_cast<f16x4*>(dst + n * 16 + 4 * g) = ov;
  }
}

// The head_dim dispatch of the blocked, bias, window and short launches: f(std::integral_constant<int, HD>) launches its instantiation.
template <typename F>
int with_head_dim(int hd, F f) {
  switch (hd) {
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    default: return -1;
  }
  return (int)hipGetLastError();
}

}  // namespace

int attention_launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int batch, int seq, int hidden, int heads,
                     const float* rel_bias, int span, hipStream_t stream) {
  const dim3 grid(p.d.gx, p.d.gy, p.d.gz);
  auto blocked = [&](auto with_bias) -> int {
    return with_head_dim(p.hd, [&](auto hd) {
      hipLaunchKernelGGL((attention_kernel<decltype(hd)::value, decltype(with_bias)::value>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, rel_bias, span);
    });
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
    case AttnForm::Window:
      if (p.window < 1) return -1;
      return with_head_dim(p.hd, [&](auto hd) {
        hipLaunchKernelGGL((attention_window_kernel<decltype(hd)::value>), grid, dim3(kThreads), 0, stream, qkv, lens, ctx, seq, hidden, p.window);
      });
    case AttnForm::Short:
      if (p.hd == 16) return -1;             // (the short kernel's first product is 32 deep)
      return with_head_dim(p.hd, [&](auto hd) {
        if constexpr (decltype(hd)::value != 16) hipLaunchKernelGGL((attention_short_kernel<decltype(hd)::value>), grid, dim3(256), 0, stream, qkv, lens, ctx, seq, hidden, heads * batch);
      });
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

}  // namespace crs
