// maxsim.hip -- late-interaction (ColBERT) scoring of candidate lists on the device (gfx950): crs_maxsim.
//
//     out[q][c] = sum_{i < q_len[q]} max_{j in doc} <q_i, d_j>         doc = tokens [offsets[r], offsets[r + 1]) of r = rows[q][c]
//
// One wave per (query, candidate); the four waves of a workgroup share one query (its 8 KB at most stay hot in L1 / L2) and take
// four neighbouring candidates.  A wave:
//
//   1. loads the query as the A operand of v_mfma_f32_16x16x32_f16 and KEEPS it in registers for the whole document: row block b
//      (16 query tokens), k-step s (32 coordinates), lane (r = lane & 15, h = lane >> 4) holds coordinates 32 s + 8 h .. + 7 of
//      query token 16 b + r -- one 16-byte load.  At most 4 x 4 fragments = 64 VGPRs.  Rows at or past q_len are zeros and are
//      never read; row blocks at or past ceil(q_len / 16) are skipped (a wave-uniform branch), so the work follows q_len, not
//      lq_max.
//   2. streams the document 16 tokens at a time straight from global memory into B fragments: lane (r, h) reads coordinates
//      32 s + 8 h .. + 7 of token t + r, 16 bytes per lane per k-step, no LDS -- a token is used by this wave alone, so staging
//      would only add a round trip.  The loads of group g + 1 are issued before the MFMAs of group g.  A token at or past the
//      document's end is read from the document's LAST token instead (an address inside the document, so nothing outside
//      [t0, t1) is touched) and its column is masked to -inf below -- not to 0: every similarity may be negative.
//   3. accumulator register e of lane (c = lane & 15, g = lane >> 4) is <query token 16 b + 4 g + e, token t + c>: each lane keeps a
//      running maximum per (b, e), 16 registers, and the columns meet only once, at the end, in one xor butterfly over the 16
//      lanes of a row per register.
//   4. adds the row maxima in a fixed order: each 16-lane group adds its rows 16 b + 4 g + e in (b, e) order, rows at or past
//      q_len skipped, then the four groups' sums are added as ((g0 + g1) + g2) + g3.
//
// Nothing in a pair's arithmetic depends on nq, m_max, lq_max, blockIdx or the other pairs: its score is bitwise independent of
// the launch it shares.  A row < 0 or >= n_rows is never dereferenced and scores -inf (whatever q_len is); an empty document and an
// empty query score 0.  Offsets are clamped into [0, n_tokens].  No scratch, no LDS, no atomics, no workgroup waits for another.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"

namespace crs {
namespace {

typedef _Float16 ms_f16x8 __attribute__((ext_vector_type(8)));
typedef float ms_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kMsThreads = 256;      // four waves: four candidates of one query
constexpr int kMsRowBlocks = 4;      // lq_max <= 64

template <int KS>   // k-steps of 32: dimp = 32 KS
__global__ __launch_bounds__(kMsThreads) void maxsim_kernel(const _Float16* __restrict__ q16, const int* __restrict__ q_len, int lq_max,
                                                            const _Float16* __restrict__ tok16, const long long* __restrict__ offsets,
                                                            long long n_rows, long long n_tokens, const long long* __restrict__ rows,
                                                            int m_max, float* __restrict__ out) {
  constexpr int kDimp = 32 * KS;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int q = blockIdx.y;
  const int c = (int)blockIdx.x * 4 + wave;
  if (c >= m_max) return;                                   // (wave-uniform)
  const size_t cell = (size_t)q * m_max + c;
  const float ninf = -__builtin_huge_valf();

  const long long row = rows[cell];
  if (row < 0 || row >= n_rows) {
    if (lane == 0) out[cell] = ninf;
    return;
  }
  int lq = q_len[q];
  lq = lq < 0 ? 0 : (lq > lq_max ? lq_max : lq);
  lq = __builtin_amdgcn_readfirstlane(lq);
  long long t0 = offsets[row], t1 = offsets[row + 1];
  t0 = t0 < 0 ? 0 : (t0 > n_tokens ? n_tokens : t0);
  t1 = t1 < 0 ? 0 : (t1 > n_tokens ? n_tokens : t1);
  if (lq == 0 || t1 <= t0) {
    if (lane == 0) out[cell] = 0.f;
    return;
  }
  const int nrb = (lq + 15) >> 4;                           // live row blocks (uniform)
  const int r = lane & 15, h = lane >> 4;

  // ---- 1. the query's fragments
  ms_f16x8 af[kMsRowBlocks][KS];
  const _Float16* qb = q16 + (size_t)q * lq_max * kDimp + 8 * h;
#pragma unroll
  for (int b = 0; b < kMsRowBlocks; ++b)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      af[b][s] = ms_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (16 * b + r < lq) af[b][s] = *reinterpret_cast<const ms_f16x8*>(qb + (size_t)(16 * b + r) * kDimp + 32 * s);
    }

  float best[kMsRowBlocks][4];
#pragma unroll
  for (int b = 0; b < kMsRowBlocks; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) best[b][e] = ninf;

  // ---- 2 + 3. the document, 16 tokens at a time
  const long long last = t1 - 1;
  auto load = [&](long long t, ms_f16x8 (&bf)[KS]) {
    long long tr = t + r;
    tr = tr > last ? last : tr;
    const _Float16* src = tok16 + (size_t)tr * kDimp + 8 * h;
#pragma unroll
    for (int s = 0; s < KS; ++s) bf[s] = *reinterpret_cast<const ms_f16x8*>(src + 32 * s);
  };
  ms_f16x8 cur[KS], nxt[KS];
  load(t0, cur);
#pragma unroll
  for (int s = 0; s < KS; ++s) nxt[s] = cur[s];
  for (long long t = t0; t < t1; t += 16) {
    if (t + 16 < t1) load(t + 16, nxt);                     // (uniform) the next group, ahead of this group's MFMAs
    const bool live = t + r < t1;                           // this lane's column
#pragma unroll
    for (int b = 0; b < kMsRowBlocks; ++b) {
      if (b < nrb) {                                        // (uniform)
        ms_f32x4 acc = ms_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[b][s], cur[s], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) best[b][e] = fmaxf(best[b][e], live ? acc[e] : ninf);
      }
    }
#pragma unroll
    for (int s = 0; s < KS; ++s) cur[s] = nxt[s];
  }

  // ---- 4. row maxima over the 16 columns, then the sum over the query's rows in a fixed order
  float sum = 0.f;
#pragma unroll
  for (int b = 0; b < kMsRowBlocks; ++b) {
    if (b < nrb) {                                          // (uniform)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float m = best[b][e];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (16 * b + 4 * h + e < lq) sum += m;
      }
    }
  }
  const float g1 = __shfl(sum, 16), g2 = __shfl(sum, 32), g3 = __shfl(sum, 48);
  if (lane == 0) out[cell] = ((sum + g1) + g2) + g3;
}

}  // namespace

int maxsim_launch(const void* q16, const int* q_len, int nq, int lq_max, const void* tok16, const int64_t* offsets, int64_t n_rows,
                  int64_t n_tokens, const int64_t* rows, int m_max, int dimp, float* out, hipStream_t stream) {
  const dim3 grid((unsigned)((m_max + 3) / 4), (unsigned)nq), block(kMsThreads);
#define CRS_MS_LAUNCH(KS)                                                                                                          \
  hipLaunchKernelGGL(maxsim_kernel<KS>, grid, block, 0, stream, static_cast<const _Float16*>(q16), q_len, lq_max,                  \
                     static_cast<const _Float16*>(tok16), reinterpret_cast<const long long*>(offsets), (long long)n_rows,          \
                     (long long)n_tokens, reinterpret_cast<const long long*>(rows), m_max, out)
  switch (dimp) {
    case 32: CRS_MS_LAUNCH(1); break;
    case 64: CRS_MS_LAUNCH(2); break;
    case 96: CRS_MS_LAUNCH(3); break;
    case 128: CRS_MS_LAUNCH(4); break;
    default: return -1;
  }
#undef CRS_MS_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace crs
