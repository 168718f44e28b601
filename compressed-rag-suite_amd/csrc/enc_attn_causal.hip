// enc_attn_causal.hip -- causal grouped-query attention for decoder-style embedders (Qwen3-Embedding, CRS_ENC_CAUSAL), gfx950.
//
//   ctx[b, q, h*hd : (h+1)*hd] = softmax_{key <= q, key < len_b}(Q_h K_{h / G}^T / sqrt(hd)) V_{h / G}       G = Hq / Hkv
//
// qkv is fp16 [T, (Hq + 2 Hkv) hd]: the Q block (Hq heads), then the K block and the V block (Hkv heads each); ctx is [T, Hq hd].
// Flash-style and TRANSPOSED like every kernel of enc_attn.hip (S^T = K Q^T, O^T = V^T P^T; a lane owns ONE query, so the softmax
// reductions are per lane + two cross-lane steps), on v_mfma_f32_16x16x32_f16 for both products, composed from the shared steps of
// enc_attn_steps.h.  What is its own:
//
//   * The work split.  A 256-thread workgroup owns a 64-query block of ONE key / value head of one sequence for ALL G query heads of
//     that group: wave w holds query rows qb + 16 w .. + 15 of each of the G heads (G query tiles per wave, as attention_seq32_kernel's
//     QT).  A K or V^T fragment is read from LDS once (ds_read_b128) and feeds G MFMAs, and each 64-key block of K / V is fetched
//     from memory and staged ONCE for G x 64 query rows: half the K / V traffic of a workgroup per query head at G = 2.
//   * Masked key blocks are never visited.  A query block at qb walks key blocks 0 .. min(qb, len - 1) / 64.  The causal test is
//     softmax_step's Plain padding test with a key limit PER LANE, lim = min(query + 1, len): only the block with kb + 64 > lim
//     (the diagonal block, or the block that holds len) compares keys; every earlier block is passed lim = INT_MAX and skips the
//     test.  Every walked block starts at a key kb <= qb <= query and kb < len, so each lane sees at least one key in every block it
//     walks and the Plain step's finite-maximum argument holds.  A padding query (q >= len) attends the real keys: finite, unread.
//   * Two K / V^T images in LDS (HD 128: 2 x (17 + 18) KB, HD 64: 2 x (9 + 9) KB).  Block i + 1 is staged into the other image
//     right after the barrier that publishes block i, so there is ONE barrier per key block, and a wave that waits for its staging
//     loads does not hold the other waves' MFMAs back (they meet again only at the next barrier).  Two workgroups fit a CU at HD 128.
//   * Longest first.  Work per workgroup grows with qb; blockIdx.y counts query blocks from the LAST one down and the (batch, kv
//     head) units run along x, so every unit's longest block is dispatched before any shorter one.
//
// Registers at <128, 2> (the largest): 32 VGPRs of Q fragments, 64 of O^T accumulators, 32 of scores, 16 of P^T operands.  Pitches
// HD + 8 and 64 + 8 halves: 16-byte aligned rows whose 16 lanes land on distinct 4-bank groups (attention_seq32_kernel's).
// A short form for query-length sequences (one wave per unit, no barrier) is not written: every length runs this kernel.

#include "enc.h"
#include "enc_attn_steps.h"

#include <limits.h>

namespace crs {
namespace {

template <int HD, int G>
__global__ __launch_bounds__(kThreads) void attention_causal_kernel(const _Float16* __restrict__ qkv, const int* __restrict__ lens,
                                                                   _Float16* __restrict__ ctx, int seq, int kv_heads) {
  constexpr int KS = HD / 32, NT = HD / 16;
  constexpr int KROW = forms::causal_krow(HD), VROW = forms::kCausalVRow;
  constexpr int IMG = forms::causal_image_halves(HD);       // one K + V^T image
  extern __shared__ __attribute__((aligned(16))) char attn_smem[];
  _Float16* smem = reinterpret_cast<_Float16*>(attn_smem);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / kv_heads, kvh = blockIdx.x % kv_heads;
  const int qb = ((int)gridDim.y - 1 - (int)blockIdx.y) * QB;          // the last query block first
  const int q = qb + wave * 16 + lr;                                   // this lane's query, in all G heads
  const int len = min(max(lens[b], 1), seq);
  const int q_heads = kv_heads * G;
  const size_t row_stride = (size_t)(q_heads + 2 * kv_heads) * HD;
  const _Float16* row0 = qkv + (size_t)b * seq * row_stride;
  const _Float16* kbase = row0 + (size_t)q_heads * HD + kvh * HD;      // K head: stage_k's base with hidden = 0
  const _Float16* vbase = kbase + (size_t)kv_heads * HD;               // V head: stage_vt's base with hidden = 0
  const float scale = kLog2e / sqrtf((float)HD);
  const int lim = min(q + 1, len);                                     // this lane's keys: [0, lim)
  const int kend = min(qb + QB, len);                                  // the workgroup's keys: blocks 0 .. (kend - 1) / 64

  f16x8 qf[G][KS];
  f32x4 o[G][NT];
  float m_run[G], l_run[G];
#pragma unroll
  for (int t = 0; t < G; ++t) {
    load_q_frags<KS>(qf[t], row0 + (size_t)(kvh * G + t) * HD, row_stride, q, seq, g);
    m_run[t] = -1e30f;
    l_run[t] = 0.f;
#pragma unroll
    for (int n = 0; n < NT; ++n) o[t][n] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  stage_k<HD, KROW, kThreads>(smem, kbase, row_stride, 0, seq, 0, KB, tid);
  stage_vt<HD, VROW, kThreads, true>(smem + KB * KROW, vbase, row_stride, 0, seq, 0, KB, tid);
  for (int kb = 0, cur = 0; kb < kend; kb += KB, cur ^= 1) {
    __syncthreads();   // image cur is staged; every wave is done with the other one
    const _Float16* sK = smem + cur * IMG;
    const _Float16* sVt = sK + KB * KROW;
    if (kb + KB < kend) {
      _Float16* nK = smem + (cur ^ 1) * IMG;
      stage_k<HD, KROW, kThreads>(nK, kbase, row_stride, 0, seq, kb + KB, KB, tid);
      stage_vt<HD, VROW, kThreads, true>(nK + KB * KROW, vbase, row_stride, 0, seq, kb + KB, KB, tid);
    }
    // ---- S^T = K Q^T: 4 tiles of 16 keys, each K fragment feeds the G heads
    f32x4 sc[G][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
#pragma unroll
      for (int t = 0; t < G; ++t) sc[t][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const f16x8 kf = *reinterpret_cast<const f16x8*>(&sK[(ct * 16 + lr) * KROW + ks * 32 + g * 8]);
#pragma unroll
        for (int t = 0; t < G; ++t) sc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[t][ks], sc[t][ct], 0, 0, 0);
      }
    }
    // the block that holds a lane's limit tests its keys; every earlier one does not (kb + 64 <= lim)
    const int lim_here = kb + KB > lim ? lim : INT_MAX;
    f16x8 pb[G][2];      // P^T as B operands of the two 32-key steps (attention_seq32_kernel's key order)
#pragma unroll
    for (int t = 0; t < G; ++t) {
      float alpha;
      f16x4 pf[4];
      softmax_step<Score::Plain>(sc[t], KeyMask{lim_here, nullptr, 0, 0, false}, kb + 4 * g, scale, m_run[t], l_run[t], alpha, pf);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2)
        pb[t][s2] = f16x8{pf[2 * s2][0], pf[2 * s2][1], pf[2 * s2][2], pf[2 * s2][3],
                          pf[2 * s2 + 1][0], pf[2 * s2 + 1][1], pf[2 * s2 + 1][2], pf[2 * s2 + 1][3]};
#pragma unroll
      for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[t][n][i] *= alpha;
    }
    // ---- O^T += V^T P^T: each V^T fragment feeds the G heads
#pragma unroll
    for (int n = 0; n < NT; ++n) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const f16x8 vf = *reinterpret_cast<const f16x8*>(&sVt[(n * 16 + lr) * VROW + s2 * 32 + g * 8]);
#pragma unroll
        for (int t = 0; t < G; ++t) o[t][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[t][s2], o[t][n], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < G; ++t) store_o<HD>(o[t], 1.0f / l_run[t], ctx, b, kvh * G + t, q, seq, q_heads * HD, g);
}

template <int HD, int G>
int launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int seq, int kv_heads, hipStream_t stream) {
  auto kernel = &attention_causal_kernel<HD, G>;
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, p.d.lds);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(kernel, dim3(p.d.gx, p.d.gy, p.d.gz), dim3(p.d.threads), p.d.lds, stream, qkv, lens, ctx, seq, kv_heads);
  return (int)hipGetLastError();
}

}  // namespace

int attention_causal_launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int seq, int kv_heads,
                            hipStream_t stream) {
  if (p.form != AttnForm::Causal) return -1;
  if (p.hd == 128 && p.group == 2) return launch<128, 2>(p, qkv, lens, ctx, seq, kv_heads, stream);
  if (p.hd == 128 && p.group == 1) return launch<128, 1>(p, qkv, lens, ctx, seq, kv_heads, stream);
  if (p.hd == 64 && p.group == 2) return launch<64, 2>(p, qkv, lens, ctx, seq, kv_heads, stream);
  if (p.hd == 64 && p.group == 1) return launch<64, 1>(p, qkv, lens, ctx, seq, kv_heads, stream);
  return -1;
}

}  // namespace crs
