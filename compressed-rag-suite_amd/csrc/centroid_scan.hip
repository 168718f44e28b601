// centroid_scan.hip -- the pruned centroid-interaction sweep over a 2-bit residual token index (gfx950): PLAID's
// candidate stage.  Declared in include/crs_hip.h: crs_centroid_maxsim_topk, _workspace_bytes, _plan_describe.  Plan: maxsim_scan.h.
//
//     A[q][r] = sum_{i < q_len[q]} float(max(+0, max_{j in row r, 0 <= cid_j < K, keep[q] bit cid_j} S[q][cid_j][i]))
//     out[q]  = the k largest (A, r) over the rows that hold a token, A descending, ties by lower row; missing slots (-inf, -1)
//
// with S and keep what crs_centroid_scores wrote.  The maximum is an fp16 maximum (exact).  The sum is fp32 in this fixed order:
// within each chunk of 8 query tokens [8 c, 8 c + 8) ascending i from +0 (tokens at or past q_len add +0), then the chunk sums
// ascending c from +0.  Nothing is multiplied and nothing is decoded: no matrix instruction appears here.
//
// The bitmap lives in LDS.  A workgroup of 16 waves serves qg queries and copies their keep bits (K / 8 bytes a query) into LDS
// once; qg = min(8, 128 KB / bitmap bytes) is the plan's.  Every WAVE then walks items of 64 rows on its own, for all qg queries
// (wave v of the grid takes items v, v + waves, ...): row ends one per lane, clamped and made non-decreasing as in maxsim_scan.hip.
//
// The cid plane is the only thing streamed.  A step is at most 64 consecutive tokens of one row, one coalesced 4-byte load a lane;
// the next step's load is issued before this step's work (the next step starts where this one ends, whatever row that is).
// Per query: a lane tests its token's bit, one ballot counts the kept tokens, and ds_permute moves their cids to lanes 0..n - 1.
//
// Gathers.  A score row is lqp * 2 bytes, CH = lqp / 8 rounded up to a power of two 16-byte chunks.  Lane = (slot s = lane / CH,
// chunk c = lane % CH): the CH lanes of a slot read one kept token's row as one contiguous access, 64 / CH tokens per pass.  A lane
// keeps four packed-fp16 running maxima (v_pk_max_f16) for its 8 query tokens, per query, from +0.  At a row's end they are
// reduced over the slots (log2(64 / CH) shuffle steps on four registers) and summed in the order above.
//
// Selection: key lists with the row in the key, one per (wave, query), as the other sweeps keep them; at the end the waves sort
// theirs (wave_sort.h), leave them in LDS where the bitmaps were, and wave j sorts the 16 lists of query j into the workgroup's
// one: the workspace is [G][nq][kp] and merge.hip reduces the G lists to k.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "maxsim_scan.h"
#include "scan.h"
#include "scan_common.h"
#include "wave_sort.h"

namespace crs {
namespace {

constexpr int kItem = CRS_MAXSIM_SCAN_ITEM_ROWS;
static_assert(kItem == 64, "one lane per row of an item");
static_assert(kCsWaves == 16, "the final sort holds one list per wave in 16 registers");

struct CsScanArgs {
  const _Float16* s16;          // [nq, K, lqp]
  const unsigned* keep;         // [nq, words]
  const int* q_len;             // [nq]
  const int* cid;               // [n_tokens]
  const long long* offsets;     // [n_rows + 1]
  long long n_tokens, row_first, row_count, items;
  float* part_s;                // [G][nq][kp]
  long long* part_r;
  int nq, lq_max, lqp, K, words, qg, kp;
};

typedef _Float16 cs_f16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ long long cs_uniform_ll(long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long cs_lane_ll(long long v, int l) { return cs_uniform_ll(__shfl(v, l)); }
__device__ __forceinline__ long long cs_clamp_ll(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned cs_pk_max(unsigned x, unsigned y) {
  return __builtin_bit_cast(unsigned, __builtin_elementwise_max(__builtin_bit_cast(cs_f16x2, x), __builtin_bit_cast(cs_f16x2, y)));
}

// QG: the queries a wave keeps state for (qg rounded up to a power of two); CH: lanes of a token slot
template <int QG, int CH>
__global__ __launch_bounds__(kCsThreads) void centroid_scan_kernel(const CsScanArgs a) {
  constexpr int kSlots = 64 / CH;
  extern __shared__ __attribute__((aligned(16))) unsigned cs_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slot = lane / CH, chunk = lane % CH;
  const int nch = a.lqp >> 3;                                         // chunks a score row really has (<= CH)
  const int q0 = (int)blockIdx.y * a.qg;
  const int nqh = a.nq - q0 < a.qg ? a.nq - q0 : a.qg;                // queries of this workgroup, 1..qg
  const float ninf = -__builtin_huge_valf();

  // ---- the queries' bitmaps, once
  for (int j = 0; j < nqh; ++j)
    for (int w = tid; w < a.words; w += kCsThreads) cs_lds[j * a.words + w] = a.keep[(size_t)(q0 + j) * a.words + w];
  __syncthreads();

  int lq[QG];
  u64 key[QG], minkey[QG];
  unsigned vmax[QG][4];
#pragma unroll
  for (int j = 0; j < QG; ++j) {
    int l = j < nqh ? a.q_len[q0 + j] : 0;
    l = l < 0 ? 0 : (l > a.lq_max ? a.lq_max : l);
    lq[j] = __builtin_amdgcn_readfirstlane(l);
    key[j] = lane < a.kp ? 0ull : ~0ull;                              // lane < kp holds one key, 0 = empty; the others are never the minimum
    minkey[j] = 0ull;
#pragma unroll
    for (int e = 0; e < 4; ++e) vmax[j][e] = 0u;                      // +0: the formula's max(+0, .)
  }
  auto offer = [&](u64& mine, u64& least, float score, unsigned rel) {
    const u64 cand = ((u64)ord_of(score) << 32) | (u64)(0xffffffffu - rel);
    if (cand > least) {                                               // (every lane holds the same two values)
      const u64 at = __ballot(mine == least);
      if (lane == (int)__builtin_ctzll(at)) mine = cand;
      u64 m = mine;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = umin64(m, __shfl_xor(m, o));
      least = m;
    }
  };

  const long long walkers = (long long)gridDim.x * kCsWaves;
  for (long long item = (long long)blockIdx.x * kCsWaves + wave; item < a.items; item += walkers) {
    const long long r0 = a.row_first + item * kItem;
    const long long left = a.row_first + a.row_count - r0;
    const int nr = left < kItem ? (int)left : kItem;
    // ---- row ends of the item, one per lane, clamped and non-decreasing
    const long long T0 = cs_uniform_ll(cs_clamp_ll(a.offsets[r0], a.n_tokens));
    long long e = cs_clamp_ll(a.offsets[r0 + 1 + (lane < nr ? lane : nr - 1)], a.n_tokens);
    e = e < T0 ? T0 : e;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long v = __shfl_up(e, o);
      if (lane >= o && v > e) e = v;
    }
    const long long T1 = cs_lane_ll(e, 63);
    if (T1 <= T0) continue;                                           // (uniform) no tokens in the item

    long long cur = T0;
    int row = (int)__popcll(__ballot(lane < nr && e <= cur));         // the first row that holds a token: T1 > T0, there is one
    auto load_cid = [&](long long at) {                               // token at + lane, kept inside [T0, T1), a sub-range of [0, n_tokens)
      const long long t = at + lane;
      return a.cid[t < T1 ? t : T1 - 1];
    };
    int cidv = load_cid(cur);
    while (row < nr) {                                                // (uniform)
      const long long t1 = cs_lane_ll(e, row);                        // > cur
      const int n_here = t1 - cur < 64 ? (int)(t1 - cur) : 64;
      const long long nxt = cur + n_here;
      const int cid_next = load_cid(nxt < T1 ? nxt : T1 - 1);
      const bool in = lane < n_here && (unsigned)cidv < (unsigned)a.K;        // a cid outside the table is skipped, never an index
      const unsigned c = in ? (unsigned)cidv : 0u;
#pragma unroll
      for (int j = 0; j < QG; ++j) {
        if (j < nqh && lq[j] > 0) {                                   // (uniform)
          const bool kept = in && ((cs_lds[j * a.words + (c >> 5)] >> (c & 31u)) & 1u);
          const u64 m = __ballot(kept);
          const int n = (int)__popcll(m);
          if (n) {                                                    // (uniform)
            const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            // lane p < n receives the p-th kept cid; the others go behind them in order, so no two lanes send to one
            const int comp = __builtin_amdgcn_ds_permute((kept ? rank : n + lane - rank) << 2, (int)c);
            const _Float16* sq = a.s16 + (size_t)(q0 + j) * a.K * a.lqp + 8 * chunk;
            for (int base = 0; base < n; base += kSlots) {            // (uniform)
              const int p = base + slot;                              // <= 63
              const int cp = __shfl(comp, p);
              if (p < n && chunk < nch) {                             // cp is a kept cid: inside [0, K)
                const uint4 v = *reinterpret_cast<const uint4*>(sq + (size_t)cp * a.lqp);
                vmax[j][0] = cs_pk_max(vmax[j][0], v.x);
                vmax[j][1] = cs_pk_max(vmax[j][1], v.y);
                vmax[j][2] = cs_pk_max(vmax[j][2], v.z);
                vmax[j][3] = cs_pk_max(vmax[j][3], v.w);
              }
            }
          }
        }
      }
      if (nxt == t1) {                                                // (uniform) the row ends here: reduce, sum, offer
        const unsigned rel = (unsigned)(item * kItem + row);
#pragma unroll
        for (int j = 0; j < QG; ++j) {
          if (j < nqh && lq[j] > 0) {                                 // (uniform) an empty query keeps nothing
            float part = 0.f;
#pragma unroll
            for (int x = 0; x < 4; ++x) {
              unsigned v = vmax[j][x];
#pragma unroll
              for (int o = CH; o < 64; o <<= 1) v = cs_pk_max(v, (unsigned)__shfl_xor((int)v, o));
              const cs_f16x2 h2 = __builtin_bit_cast(cs_f16x2, v);
              part += 8 * chunk + 2 * x < lq[j] ? (float)h2[0] : 0.f;
              part += 8 * chunk + 2 * x + 1 < lq[j] ? (float)h2[1] : 0.f;
              vmax[j][x] = 0u;
            }
            float sum = 0.f;
#pragma unroll
            for (int cc = 0; cc < CH; ++cc) {
              const float pc = __shfl(part, cc);                      // slot 0's lane of chunk cc
              if (cc < nch) sum += pc;                                // (uniform)
            }
            offer(key[j], minkey[j], sum, rel);
          }
        }
        row += 1;
        row += (int)__popcll(__ballot(lane >= row && lane < nr && e <= nxt));      // rows without tokens are never offered
      }
      cur = nxt;
      cidv = cid_next;
    }
  }

  // ---- every wave's lists, sorted, into LDS (the bitmaps are dead); wave j sorts query j's 16 lists into the workgroup's one
#pragma unroll
  for (int j = 0; j < QG; ++j) {
    u64 k1[1] = {lane < a.kp ? key[j] : 0ull};
    wave_sort_keys<1>(k1, lane);
    key[j] = k1[0];
  }
  __syncthreads();                                                    // everybody is done with the bitmaps
  u64* lists = reinterpret_cast<u64*>(cs_lds);                        // [qg][16][64]
#pragma unroll
  for (int j = 0; j < QG; ++j)
    if (j < nqh) lists[(j * kCsWaves + wave) * 64 + lane] = key[j];
  __syncthreads();
  if (wave < nqh) {
    u64 all[kCsWaves];
#pragma unroll
    for (int u = 0; u < kCsWaves; ++u) all[u] = lists[(wave * kCsWaves + u) * 64 + lane];
    wave_sort_keys<kCsWaves>(all, lane);                              // element lane + 64 u, descending: the best 64 are all[0]
    if (lane < a.kp) {
      const size_t o = ((size_t)blockIdx.x * a.nq + (q0 + wave)) * a.kp + lane;
      const bool in = all[0] != 0;
      a.part_s[o] = in ? float_of_ord((unsigned)(all[0] >> 32)) : ninf;
      a.part_r[o] = in ? a.row_first + (long long)(0xffffffffu - (unsigned)all[0]) : -1;
    }
  }
}

__global__ void centroid_scan_fill_kernel(float* out_s, long long* out_r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { out_s[i] = -__builtin_huge_valf(); out_r[i] = -1; }
}

using CsScanKernel = void (*)(const CsScanArgs);
template <int QG>
CsScanKernel scan_kernel_ch(int ch) {
  switch (ch) {
    case 1: return centroid_scan_kernel<QG, 1>;
    case 2: return centroid_scan_kernel<QG, 2>;
    case 4: return centroid_scan_kernel<QG, 4>;
    default: return centroid_scan_kernel<QG, 8>;
  }
}
CsScanKernel scan_kernel(int qg, int ch) {
  if (qg <= 1) return scan_kernel_ch<1>(ch);
  if (qg <= 2) return scan_kernel_ch<2>(ch);
  if (qg <= 4) return scan_kernel_ch<4>(ch);
  return scan_kernel_ch<8>(ch);
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_centroid_maxsim_topk_workspace_bytes(int nq, int k, int64_t row_count, size_t* bytes) {
  crs::CentroidScanPlan p;
  const char* why = "";
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer (bytes)");
  if (crs::centroid_scan_make_plan(nq, 1, CRS_RC_MIN_CENTROIDS, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  *bytes = crs::centroid_scan_workspace_bound(nq, k, row_count);
  return CRS_OK;
}

int crs_centroid_maxsim_topk_plan_describe(int nq, int lq_max, int n_centroids, int k, int64_t row_count, char* buf, size_t cap) {
  crs::CentroidScanPlan p;
  const char* why = "";
  if (!buf || cap == 0) return crs::set_error(CRS_EINVAL, "null buffer");
  if (crs::centroid_scan_make_plan(nq, lq_max, n_centroids, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  crs::centroid_scan_plan_describe(p, buf, cap);
  return CRS_OK;
}

int crs_centroid_maxsim_topk(const void* s16_dev, const uint32_t* keep_dev, const int32_t* q_len_dev, int nq, int lq_max, int n_centroids,
                             const int32_t* cid_dev, const int64_t* offsets_dev, int64_t n_rows, int64_t n_tokens, int64_t row_first,
                             int64_t row_count, int k, void* workspace_dev, size_t workspace_bytes, float* out_scores_dev,
                             int64_t* out_rows_dev, void* stream) {
  using namespace crs;
  CentroidScanPlan p;
  const char* why = "";
  if (n_rows < 0 || n_tokens < 0) return set_error(CRS_EINVAL, "bad n_rows/n_tokens");
  if (row_first < 0 || row_count < 0 || row_first > n_rows || row_count > n_rows - row_first)
    return set_error(CRS_EINVAL, "row range leaves [0, n_rows)");
  if (centroid_scan_make_plan(nq, lq_max, n_centroids, k, row_count, &p, &why)) return set_error(CRS_EINVAL, why);
  if (!s16_dev || !keep_dev) return set_error(CRS_EINVAL, "s16_dev / keep_dev is null");
  if (!q_len_dev) return set_error(CRS_EINVAL, "q_len_dev is null");
  if (!offsets_dev) return set_error(CRS_EINVAL, "offsets_dev is null");
  if (n_tokens > 0 && !cid_dev) return set_error(CRS_EINVAL, "cid_dev is null");
  if (!workspace_dev) return set_error(CRS_EINVAL, "workspace_dev is null");
  if (!out_scores_dev || !out_rows_dev) return set_error(CRS_EINVAL, "out_scores_dev / out_rows_dev is null");
  if (((uintptr_t)s16_dev | (uintptr_t)workspace_dev) & 15) return set_error(CRS_EINVAL, "s16_dev / workspace_dev must be 16-byte aligned");
  if ((uintptr_t)keep_dev & 3) return set_error(CRS_EINVAL, "keep_dev must be 4-byte aligned");
  if (workspace_bytes < p.bytes) return set_error(CRS_EINVAL, "workspace too small (crs_centroid_maxsim_topk_workspace_bytes)");
  if (nq == 0) return CRS_OK;
  hipStream_t st = (hipStream_t)stream;
  if (row_count == 0) {
    const int n = nq * k;
    hipLaunchKernelGGL(centroid_scan_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out_scores_dev,
                       reinterpret_cast<long long*>(out_rows_dev), n);
    return launch_status("centroid_maxsim_topk (empty range)");
  }
  char* ws = static_cast<char*>(workspace_dev);
  float* part_s = reinterpret_cast<float*>(ws + p.part_s);
  int64_t* part_r = reinterpret_cast<int64_t*>(ws + p.part_r);
  const CsScanArgs a{static_cast<const _Float16*>(s16_dev), keep_dev, q_len_dev, cid_dev, reinterpret_cast<const long long*>(offsets_dev),
                     (long long)n_tokens, (long long)row_first, (long long)row_count, (long long)p.items, part_s,
                     reinterpret_cast<long long*>(part_r), nq, lq_max, p.lqp, n_centroids, p.words, p.qg, p.kp};
  const CsScanKernel kern = scan_kernel(p.qg, p.ch);
  if (p.lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes) != hipSuccess)
    return launch_status("centroid_maxsim_topk (LDS size)");
  hipLaunchKernelGGL(kern, dim3((unsigned)p.g, (unsigned)p.qgroups), dim3(kCsThreads), (size_t)p.lds_bytes, st, a);
  merge_launch_i64(part_s, part_r, p.g, nq, p.kp, k, out_scores_dev, out_rows_dev, st);
  return launch_status("centroid_maxsim_topk");
}

}  // extern "C"
