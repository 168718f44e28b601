// maxsim_rc.hip -- late-interaction scoring of candidate lists over a 2-bit residual token index (gfx950): crs_maxsim_rc
// (DESIGN 3.24).
//
//     out[q][c] = sum_{i < q_len[q]} max_{j in doc} <Q_i, V_j>     V_j the decoded token (maxsim_rc.h), doc = tokens
//                                                                  [offsets[r], offsets[r + 1]) of r = rows[q][c]
//
// maxsim_f8.hip's kernel on compressed rows: one wave per (query, candidate), the four waves of a workgroup share a query.  A
// group of 16 document tokens is, per lane, one cid, one scale, 2 KS code bytes and KS 16-byte loads of the token's centroid row;
// the lane decodes its 8 KS coordinates in registers (packed fp16, maxsim_rc.h) and the group is multiplied against the resident
// fp16 query by v_mfma_f32_16x16x32_f16 from a zero accumulator.  The next group's three plane reads and its gathers are issued
// ahead of this group's decode.  What does not change is everything DESIGN 3.15 fixes: a token at or past the document's end is
// read from the document's last token and its column masked to -inf by a select, a running fmaxf per (row block, register), and
// step 4's sum order.  A row < 0 or >= n_rows is never dereferenced and scores -inf; an empty document and an empty query score
// 0; a cid outside the table is never used as an index.  No scratch, no LDS, no atomics.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "maxsim_rc.h"
#include "scan.h"

namespace crs {
namespace {

constexpr int kMsRcThreads = 256;     // four waves: four candidates of one query
constexpr int kMsRcRowBlocks = 4;     // lq_max <= 64

template <int KS>   // dimp = 32 KS
__global__ __launch_bounds__(kMsRcThreads) void maxsim_rc_kernel(const _Float16* __restrict__ q16, const int* __restrict__ q_len, int lq_max,
                                                                 const RcPlanes tok, const RcCodec codec,
                                                                 const long long* __restrict__ offsets, long long n_rows,
                                                                 long long n_tokens, const long long* __restrict__ rows, int m_max,
                                                                 float* __restrict__ out) {
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
  const RcWeights w = rc_weights(codec.weights);

  // ---- 1. the query's fragments: rows at or past q_len are zeros and are never read
  RcFrag<KS> af[kMsRcRowBlocks];
  const _Float16* qb = q16 + (size_t)q * lq_max * kDimp;
#pragma unroll
  for (int b = 0; b < kMsRcRowBlocks; ++b)
    af[b] = 16 * b + r < lq ? rc_load_query<KS>(qb + (size_t)(16 * b + r) * kDimp, h) : rc_zero<KS>();

  float best[kMsRcRowBlocks][4];
#pragma unroll
  for (int b = 0; b < kMsRcRowBlocks; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) best[b][e] = ninf;

  // ---- 2 + 3. the document, 16 tokens at a time, the next group's loads ahead of this group's decode and MFMAs
  const long long last = t1 - 1;
  auto load = [&](long long t) {
    long long tr = t + r;
    tr = tr > last ? last : tr;                             // t0 <= tr < t1 <= n_tokens
    RcRaw<KS> raw;
    int cid = tok.cid[tr];
    unsigned sc = tok.scale[tr];
    rc_checked(cid, sc, codec.n_centroids);
    raw.scale2 = sc | (sc << 16);
    raw.codes = rc_load_codes<KS>(tok.codes + (size_t)tr * (8 * KS), h);
    rc_gather<KS>(raw, codec, cid, h);
    return raw;
  };
  RcRaw<KS> cur = load(t0), nxt = cur;
  for (long long t = t0; t < t1; t += 16) {
    if (t + 16 < t1) nxt = load(t + 16);                    // (uniform)
    const bool live = t + r < t1;                           // this lane's column
    const RcFrag<KS> bd = rc_decode<KS>(cur, w);
#pragma unroll
    for (int b = 0; b < kMsRcRowBlocks; ++b) {
      if (b < nrb) {                                        // (uniform)
        const f8_f32x4 acc = rc_mfma<KS>(af[b], bd);
#pragma unroll
        for (int e = 0; e < 4; ++e) best[b][e] = fmaxf(best[b][e], live ? acc[e] : ninf);
      }
    }
    cur = nxt;
  }

  // ---- 4. row maxima over the 16 columns, then the sum over the query's rows in a fixed order
  const float score = f8_row_sum(best, nrb, lq, h);
  if (lane == 0) out[cell] = score;
}

}  // namespace
}  // namespace crs

extern "C" int crs_maxsim_rc(const void* q16_dev, const int32_t* q_len_dev, int nq, int lq_max, const int32_t* cid_dev, const void* codes_dev,
                             const void* scale_dev, const void* centroids_dev, int n_centroids, const float* weights_dev,
                             const int64_t* offsets_dev, int64_t n_rows, int64_t n_tokens, const int64_t* rows_dev, int m_max, int dimp,
                             float* out_dev, void* stream) {
  using namespace crs;
  if (lq_max < 1 || lq_max > CRS_MAXSIM_MAX_QUERY) return set_error(CRS_EINVAL, "lq_max must be in 1..CRS_MAXSIM_MAX_QUERY");
  if (dimp != 32 && dimp != 64 && dimp != 96 && dimp != 128) return set_error(CRS_EINVAL, "dimp must be 32, 64, 96 or 128");
  if (nq < 0 || nq > 65535) return set_error(CRS_EINVAL, "nq must be in 0..65535");
  if (m_max < 1) return set_error(CRS_EINVAL, "bad m_max (m_max >= 1)");
  if (n_rows < 0 || n_tokens < 0) return set_error(CRS_EINVAL, "bad n_rows/n_tokens");
  if (n_centroids < CRS_RC_MIN_CENTROIDS || n_centroids > CRS_RC_MAX_CENTROIDS)
    return set_error(CRS_EINVAL, "n_centroids must be in CRS_RC_MIN_CENTROIDS..CRS_RC_MAX_CENTROIDS");
  if (!q16_dev) return set_error(CRS_EINVAL, "q16_dev is null");
  if (!q_len_dev) return set_error(CRS_EINVAL, "q_len_dev is null");
  if (!centroids_dev || !weights_dev) return set_error(CRS_EINVAL, "centroids_dev / weights_dev is null");
  if (!offsets_dev) return set_error(CRS_EINVAL, "offsets_dev is null");
  if (!rows_dev) return set_error(CRS_EINVAL, "rows_dev is null");
  if (!out_dev) return set_error(CRS_EINVAL, "out_dev is null");
  if (n_tokens > 0 && (!cid_dev || !codes_dev || !scale_dev)) return set_error(CRS_EINVAL, "cid_dev / codes_dev / scale_dev is null");
  if (((uintptr_t)q16_dev | (uintptr_t)codes_dev | (uintptr_t)centroids_dev) & 15)
    return set_error(CRS_EINVAL, "q16_dev / codes_dev / centroids_dev must be 16-byte aligned");
  if (nq == 0) return CRS_OK;
  const RcPlanes tok{cid_dev, static_cast<const unsigned char*>(codes_dev), static_cast<const unsigned short*>(scale_dev)};
  const RcCodec codec{static_cast<const _Float16*>(centroids_dev), weights_dev, n_centroids};
  const dim3 grid((unsigned)((m_max + 3) / 4), (unsigned)nq), block(kMsRcThreads);
#define CRS_MSRC_LAUNCH(KS)                                                                                                        \
  hipLaunchKernelGGL(maxsim_rc_kernel<KS>, grid, block, 0, (hipStream_t)stream, static_cast<const _Float16*>(q16_dev), q_len_dev,   \
                     lq_max, tok, codec, reinterpret_cast<const long long*>(offsets_dev), (long long)n_rows, (long long)n_tokens,  \
                     reinterpret_cast<const long long*>(rows_dev), m_max, out_dev)
  switch (dimp) {
    case 32: CRS_MSRC_LAUNCH(1); break;
    case 64: CRS_MSRC_LAUNCH(2); break;
    case 96: CRS_MSRC_LAUNCH(3); break;
    default: CRS_MSRC_LAUNCH(4); break;
  }
#undef CRS_MSRC_LAUNCH
  return launch_status("maxsim_rc");
}
