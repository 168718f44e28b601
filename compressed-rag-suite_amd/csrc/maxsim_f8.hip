// maxsim_f8.hip -- late-interaction scoring of candidate lists over an fp8 (e4m3) token index (gfx950): crs_maxsim_f8.
//
//     out[q][c] = 2^(-2 S) sum_{i < q_len[q]} max_{j in doc} <Q_i, D_j>     over the stored e4m3 values (e4m3.h), doc = tokens
//                                                                           [offsets[r], offsets[r + 1]) of r = rows[q][c]
//
// maxsim.hip's kernel on byte rows: one wave per (query, candidate), the four waves of a workgroup share a query.  A group of 16
// document tokens is two 16-byte loads per lane instead of four; the fragments are decoded to fp16 in registers, exactly, and
// multiplied by v_mfma_f32_16x16x32_f16 from a zero accumulator (maxsim_f8.h says why not by the fp8 matrix instructions), so
// products are exact and the accumulation is fp32.  The query is decoded once and kept (64 VGPRs at dimp 128, as in fp16).  What
// does not change is everything DESIGN 3.15 fixes: a token at or past the document's end is read from the document's last token
// and its column masked to -inf by a select, a running fmaxf per (row block, register), and step 4's sum order.
// A row < 0 or >= n_rows is never dereferenced and scores -inf; an empty document and an empty query score 0.  No scratch, no LDS,
// no atomics.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "maxsim_f8.h"
#include "scan.h"

namespace crs {
namespace {

constexpr int kMs8Threads = 256;      // four waves: four candidates of one query
constexpr int kMs8RowBlocks = 4;      // lq_max <= 64

template <int KS>   // dimp = 32 KS bytes
__global__ __launch_bounds__(kMs8Threads) void maxsim_f8_kernel(const unsigned char* __restrict__ q8, const int* __restrict__ q_len,
                                                                int lq_max, const unsigned char* __restrict__ tok8,
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

  // ---- 1. the query's fragments: rows at or past q_len are zeros and are never read
  F8Frag16<KS> af[kMs8RowBlocks];
  const unsigned char* qb = q8 + (size_t)q * lq_max * kDimp;
#pragma unroll
  for (int b = 0; b < kMs8RowBlocks; ++b) {
    f8x32 raw = f8x32{0, 0, 0, 0, 0, 0, 0, 0};
    if (16 * b + r < lq) raw = f8_load_frag<KS>(qb + (size_t)(16 * b + r) * kDimp, h);
    af[b] = f8_decode<KS>(raw);
  }

  float best[kMs8RowBlocks][4];
#pragma unroll
  for (int b = 0; b < kMs8RowBlocks; ++b)
#pragma unroll
    for (int e = 0; e < 4; ++e) best[b][e] = ninf;

  // ---- 2 + 3. the document, 16 tokens at a time, the next group's loads ahead of this group's MFMAs
  const long long last = t1 - 1;
  auto load = [&](long long t) {
    long long tr = t + r;
    tr = tr > last ? last : tr;
    return f8_load_frag<KS>(tok8 + (size_t)tr * kDimp, h);
  };
  f8x32 cur = load(t0), nxt = cur;
  for (long long t = t0; t < t1; t += 16) {
    if (t + 16 < t1) nxt = load(t + 16);                    // (uniform)
    const bool live = t + r < t1;                           // this lane's column
    const F8Frag16<KS> bd = f8_decode<KS>(cur);
#pragma unroll
    for (int b = 0; b < kMs8RowBlocks; ++b) {
      if (b < nrb) {                                        // (uniform)
        const f8_f32x4 acc = f8_mfma<KS>(af[b], bd);
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

int maxsim_f8_launch(const void* q8, const int* q_len, int nq, int lq_max, const void* tok8, const int64_t* offsets, int64_t n_rows,
                     int64_t n_tokens, const int64_t* rows, int m_max, int dimp, float* out, hipStream_t stream) {
  const dim3 grid((unsigned)((m_max + 3) / 4), (unsigned)nq), block(kMs8Threads);
#define CRS_MS8_LAUNCH(KS)                                                                                                         \
  hipLaunchKernelGGL(maxsim_f8_kernel<KS>, grid, block, 0, stream, static_cast<const unsigned char*>(q8), q_len, lq_max,           \
                     static_cast<const unsigned char*>(tok8), reinterpret_cast<const long long*>(offsets), (long long)n_rows,      \
                     (long long)n_tokens, reinterpret_cast<const long long*>(rows), m_max, out)
  switch (dimp) {
    case 32: CRS_MS8_LAUNCH(1); break;
    case 64: CRS_MS8_LAUNCH(2); break;
    case 96: CRS_MS8_LAUNCH(3); break;
    case 128: CRS_MS8_LAUNCH(4); break;
    default: return -1;
  }
#undef CRS_MS8_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace crs
