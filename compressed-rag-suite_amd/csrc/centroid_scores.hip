// centroid_scores.hip -- the first step of the pruned centroid-interaction first stage over a 2-bit residual token index (gfx950;
// DESIGN 3.25): every query token against every CENTROID of the codec, once per query, and the bitmap of the centroids that some
// query token likes.  Declared in include/crs_hip.h: crs_centroid_scores.
//
//     S[q][c][i]   = fp16(<Q_qi, C_c>)      exact products, fp32 accumulation from zero, k-steps ascending, one rounding (RNE);
//                                           +0 for q_len[q] <= i < lqp, lqp = lq_max rounded up to a multiple of 8
//     keep[q] bit c = q_len[q] > 0 and max_{i < q_len[q]} float(S[q][c][i]) >= t        (of the STORED values; bits past K are 0)
//
// Split.  A wave owns 64 consecutive centroids of one query, as four groups of 16, and all of the query's row blocks: the query's
// A fragments stay in registers (maxsim_rc.h's layout: lane (r, h) holds coordinates [8 KS h, 8 KS (h + 1)) of token r) and are
// reused for kCsChunks such sets of 64.  The centroid rows are read as rc_gather reads them -- lane (r, h) loads its KS 16-byte
// pieces of row c0 + r, 16 rows of one group are one contiguous 512 KS bytes -- and never pass through LDS: every centroid byte is
// used by exactly one wave, so there is nothing to share.  D's lane (r, h) holds S for centroid r and query tokens 16 b + 4 h + {0..3}:
// four consecutive fp16, one 8-byte store.  The maximum over i is a maximum over a lane's registers and then over the four h
// (two shuffles); the 16 keep bits of a group are the low 16 bits of one ballot, and four groups make the two words lane 0 writes.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "maxsim_rc.h"
#include "scan.h"

namespace crs {
namespace {

constexpr int kCsScoreThreads = 256;
constexpr int kCsChunks = 4;                                  // sets of 64 centroids a wave serves with one load of the query
constexpr int kCsBlockCentroids = (kCsScoreThreads / 64) * kCsChunks * 64;

struct CsScoreArgs {
  const _Float16* q16;          // [nq, lq_max, dimp]
  const int* q_len;             // [nq]
  const _Float16* centroids;    // [K, dimp]
  _Float16* s16;                // [nq, K, lqp]
  unsigned* keep;               // [nq, words]
  float t;
  int lq_max, lqp, K, words;
};

typedef _Float16 cs_f16x4 __attribute__((ext_vector_type(4)));

template <int KS>
__global__ __launch_bounds__(kCsScoreThreads) void centroid_scores_kernel(const CsScoreArgs a) {
  constexpr int kDimp = 32 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, h = lane >> 4;
  const int q = blockIdx.y;
  int lq = a.q_len[q];
  lq = lq < 0 ? 0 : (lq > a.lq_max ? a.lq_max : lq);
  const _Float16* qb = a.q16 + (size_t)q * a.lq_max * kDimp;
  RcFrag<KS> af[4];
#pragma unroll
  for (int b = 0; b < 4; ++b) af[b] = 16 * b + r < lq ? rc_load_query<KS>(qb + (size_t)(16 * b + r) * kDimp, h) : rc_zero<KS>();
  const RcCodec codec{a.centroids, nullptr, a.K};
  const float ninf = -__builtin_huge_valf();

  for (int chunk = 0; chunk < kCsChunks; ++chunk) {
    const int c0 = (int)blockIdx.x * kCsBlockCentroids + (wave * kCsChunks + chunk) * 64;      // (uniform)
    if (c0 >= a.K) break;
    unsigned long long bits = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = c0 + 16 * g + r;
      const bool in = c < a.K;
      RcRaw<KS> raw;
      rc_gather<KS>(raw, codec, in ? c : a.K - 1, h);          // past the table: its last row again, never stored
      RcFrag<KS> bf;
#pragma unroll
      for (int s = 0; s < KS; ++s) bf.v[s] = __builtin_bit_cast(rc_f16x8, raw.cent[s]);
      _Float16* out = a.s16 + ((size_t)q * a.K + (in ? c : 0)) * a.lqp;
      float best = ninf;
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i0 = 16 * b + 4 * h;                         // lqp is a multiple of 8: the four columns are inside a row or outside
        if (16 * b < a.lqp) {                                  // (uniform)
          const f8_f32x4 acc = rc_mfma<KS>(af[b], bf);
          cs_f16x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            v[e] = i0 + e < lq ? (_Float16)acc[e] : (_Float16)0.f;
            best = fmaxf(best, i0 + e < lq ? (float)v[e] : ninf);
          }
          if (in && i0 < a.lqp) *reinterpret_cast<cs_f16x4*>(out + i0) = v;
        }
      }
      best = fmaxf(best, __shfl_xor(best, 16));
      best = fmaxf(best, __shfl_xor(best, 32));
      const unsigned long long m = __ballot(in && lq > 0 && best >= a.t);
      bits |= (m & 0xffffull) << (16 * g);
    }
    if (lane == 0) {
      const int w = c0 >> 5;                                   // c0 is a multiple of 64: two whole words
      unsigned* kq = a.keep + (size_t)q * a.words;
      kq[w] = (unsigned)bits;
      if (w + 1 < a.words) kq[w + 1] = (unsigned)(bits >> 32);
    }
  }
}

using CsScoreKernel = void (*)(const CsScoreArgs);
CsScoreKernel score_kernel(int ksteps) {
  switch (ksteps) {
    case 1: return centroid_scores_kernel<1>;
    case 2: return centroid_scores_kernel<2>;
    case 3: return centroid_scores_kernel<3>;
    default: return centroid_scores_kernel<4>;
  }
}

}  // namespace
}  // namespace crs

extern "C" int crs_centroid_scores(const void* q16_dev, const int32_t* q_len_dev, int nq, int lq_max, const void* centroids_dev,
                                   int n_centroids, int dimp, float threshold, void* s16_dev, uint32_t* keep_dev, void* stream) {
  using namespace crs;
  if (lq_max < 1 || lq_max > CRS_MAXSIM_MAX_QUERY) return set_error(CRS_EINVAL, "lq_max must be in 1..CRS_MAXSIM_MAX_QUERY");
  if (dimp != 32 && dimp != 64 && dimp != 96 && dimp != 128) return set_error(CRS_EINVAL, "dimp must be 32, 64, 96 or 128");
  if (nq < 0 || nq > 65535) return set_error(CRS_EINVAL, "nq must be in 0..65535");
  if (n_centroids < CRS_RC_MIN_CENTROIDS || n_centroids > CRS_RC_MAX_CENTROIDS)
    return set_error(CRS_EINVAL, "n_centroids must be in CRS_RC_MIN_CENTROIDS..CRS_RC_MAX_CENTROIDS");
  if (threshold != threshold) return set_error(CRS_EINVAL, "threshold is NaN");
  if (!q16_dev || !q_len_dev || !centroids_dev) return set_error(CRS_EINVAL, "q16_dev / q_len_dev / centroids_dev is null");
  if (!s16_dev || !keep_dev) return set_error(CRS_EINVAL, "s16_dev / keep_dev is null");
  if (((uintptr_t)q16_dev | (uintptr_t)centroids_dev | (uintptr_t)s16_dev) & 15)
    return set_error(CRS_EINVAL, "q16_dev / centroids_dev / s16_dev must be 16-byte aligned");
  if ((uintptr_t)keep_dev & 3) return set_error(CRS_EINVAL, "keep_dev must be 4-byte aligned");
  if (nq == 0) return CRS_OK;
  const CsScoreArgs a{static_cast<const _Float16*>(q16_dev), q_len_dev, static_cast<const _Float16*>(centroids_dev),
                      static_cast<_Float16*>(s16_dev), keep_dev, threshold, lq_max, (lq_max + 7) & ~7, n_centroids, (n_centroids + 31) / 32};
  const unsigned blocks = (unsigned)((n_centroids + kCsBlockCentroids - 1) / kCsBlockCentroids);
  hipLaunchKernelGGL(score_kernel(dimp / 32), dim3(blocks, (unsigned)nq), dim3(kCsScoreThreads), 0, (hipStream_t)stream, a);
  return launch_status("centroid_scores");
}
