// csr_scan.h -- what the flat doc-at-a-time CSR scans share (bm25.hip: crs_bm25_topk, sparse_scan.hip: crs_sparse_topk): the
// sorted (token, query, weight) pair table of a launch, the per-tile list insertion and the launch geometry.  The two scans differ
// in the term a matching token adds and in the per-row inputs it needs, nothing else.  Everything here sits in an anonymous
// namespace: each of the two files gets its own copy of the pair kernel.
#pragma once
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

namespace crs {
namespace {

constexpr int kLanes = 64;                     // rows per tile: one lane per row
constexpr int kMaxPairs = CRS_BM25_MAX_PAIRS;  // (query, token) pairs per launch
constexpr int kChunk = 2048;                   // tokens staged per round
constexpr int kMinTiles = 4;                   // tiles per workgroup at least (short collections: fewer lists to merge)
constexpr int kMaxWg = 2048;                   // workgroups at most
constexpr int kSortThreads = 256;
constexpr unsigned long long kNoPair = ~0ull;
constexpr float kNegInf = -__builtin_huge_valf();
static_assert((kMaxPairs & (kMaxPairs - 1)) == 0 && kMaxPairs <= 4096, "pair index fits the 12 low bits of a sort key");
static_assert(CRS_MAX_K <= kLanes, "one lane per list slot");

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---- the pair table: (token, query, weight) sorted by token, then query ----------------------------------------------------------
// Pair p IS entry p of q_tok / q_w (n_pairs = their length <= kMaxPairs); its query is the one whose clamped offsets hold p.  An
// entry no query holds sorts last as (0xffffffff, query 0, weight 0).
__global__ __launch_bounds__(kSortThreads) void csr_pairs_kernel(const int64_t* __restrict__ q_off, const int* __restrict__ q_tok,
                                                                const float* __restrict__ q_w, int nq, int n_pairs,
                                                                unsigned* __restrict__ pt_tok, float* __restrict__ pt_w,
                                                                int* __restrict__ pt_q) {
  __shared__ unsigned long long key[kMaxPairs];
  __shared__ int off[kLanes + 1];
  const int tid = threadIdx.x;
  for (int q = tid; q <= nq; q += kSortThreads) off[q] = (int)clamp_i64(q_off[q], 0, n_pairs);
  __syncthreads();
  int n2 = 1;
  while (n2 < n_pairs) n2 <<= 1;
  for (int p = tid; p < n2; p += kSortThreads) {
    unsigned long long kk = kNoPair;
    if (p < n_pairs) {
      int lo = 0, hi = nq;                     // the last q in [0, nq) with off[q] <= p
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
      }
      if (off[lo] <= p && p < off[lo + 1]) kk = ((unsigned long long)(unsigned)q_tok[p] << 12) | (unsigned)p;
    }
    key[p] = kk;
  }
  __syncthreads();
  for (int size = 2; size <= n2; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < (n2 >> 1); i += kSortThreads) {
        const int a = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), b = a | stride;
        const bool up = (a & size) == 0;
        const unsigned long long x = key[a], y = key[b];
        if ((x > y) == up) { key[a] = y; key[b] = x; }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < n_pairs; i += kSortThreads) {
    const unsigned long long kk = key[i];
    if (kk == kNoPair) {
      pt_tok[i] = 0xffffffffu; pt_w[i] = 0.0f; pt_q[i] = 0;
    } else {
      const int p = (int)(kk & 4095ull);
      int lo = 0, hi = nq;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p) lo = mid; else hi = mid;
      }
      pt_tok[i] = (unsigned)(kk >> 12); pt_w[i] = q_w[p]; pt_q[i] = lo;
    }
  }
}

// dynamic LDS of a scan: [pair tokens u32 [n_pairs] | pair weights f32 [n_pairs] | acc f32 [nq, 64] | list scores f32 [nq, k] |
//                         list rows i32 [nq, k] | staged tokens u32 [kChunk] | pair queries u8 [n_pairs]]
__host__ __device__ inline size_t csr_scan_lds_bytes(int nq, int k, int n_pairs) {
  return (size_t)n_pairs * 8 + (size_t)nq * kLanes * 4 + (size_t)nq * k * 8 + (size_t)kChunk * 4 + (((size_t)n_pairs + 3) & ~(size_t)3);
}

// ---- selection: the rows of a tile that enter a query's list, in row order ----
// Lane d holds row tile * 64 + d: `mine` the queries it hit, acc[q * 64 + d] its scores.  A query's sorted list is held one slot
// per lane while it is updated and kept in LDS between tiles.  Rows only ascend inside a workgroup, so an equal score never
// displaces an earlier row: ties by lower row.
__device__ __forceinline__ void csr_select_tile(const float* acc, unsigned long long mine, int nq, int k, int tile, int lane,
                                                float* ls_s, int* ls_r) {
  for (int q = 0; q < nq; ++q) {
    const bool hit = (mine >> q) & 1ull;
    if (!__ballot(hit)) continue;                    // (uniform)
    const float s = acc[q * kLanes + lane];
    float my_s = lane < k ? ls_s[q * k + lane] : kNegInf;     // slot `lane` of the query's list
    int my_r = lane < k ? ls_r[q * k + lane] : -1;
    float kth_s = __shfl(my_s, k - 1);
    int kth_r = __shfl(my_r, k - 1);
    unsigned long long todo = __ballot(hit && (kth_r < 0 || s > kth_s));
    bool changed = false;
    while (todo) {
      const int src = __ffsll((long long)todo) - 1;
      todo &= todo - 1ull;
      const float cs = __shfl(s, src);
      if (!(kth_r < 0 || cs > kth_s)) continue;
      const int pos = __popcll(__ballot(lane < k && my_r >= 0 && my_s >= cs));   // entries that stay ahead: an equal score is an earlier row
      const float up_s = __shfl_up(my_s, 1);
      const int up_r = __shfl_up(my_r, 1);
      if (pos >= k) continue;
      if (lane == pos) { my_s = cs; my_r = tile * kLanes + src; }
      else if (lane > pos && lane < k) { my_s = up_s; my_r = up_r; }
      kth_s = __shfl(my_s, k - 1);
      kth_r = __shfl(my_r, k - 1);
      changed = true;
    }
    if (changed && lane < k) { ls_s[q * k + lane] = my_s; ls_r[q * k + lane] = my_r; }
  }
}

// geometry of a launch: workgroups and tiles per workgroup for n_rows rows
inline void csr_scan_plan(int64_t n_rows, int* n_wg, int* tiles_per_wg) {
  const int64_t n_tiles = (n_rows + kLanes - 1) / kLanes;
  int64_t per = (n_tiles + kMaxWg - 1) / kMaxWg;
  if (per < kMinTiles) per = kMinTiles;
  *tiles_per_wg = (int)per;
  *n_wg = (int)((n_tiles + per - 1) / per);
  if (*n_wg < 1) *n_wg = 1;
}

inline size_t csr_scan_align(size_t x) { return (x + 255) / 256 * 256; }

// workspace: [pair tokens | pair weights | pair queries (kMaxPairs each) | partial scores f32 [n_wg, nq, k] | partial rows i64 [n_wg, nq, k]]
inline size_t csr_scan_workspace_bytes(int nq, int k, int64_t n_rows) {
  int n_wg, per;
  csr_scan_plan(n_rows, &n_wg, &per);
  const size_t cells = (size_t)n_wg * nq * k;
  return 3 * csr_scan_align((size_t)kMaxPairs * 4) + csr_scan_align(cells * 4) + csr_scan_align(cells * 8);
}

struct CsrScanWs {
  unsigned* pt_tok;
  float* pt_w;
  int* pt_q;
  float* part_s;
  int64_t* part_i;
};
inline CsrScanWs csr_scan_ws(void* workspace, int n_wg, int nq, int k) {
  const size_t cells = (size_t)n_wg * nq * k;
  char* w = reinterpret_cast<char*>(workspace);
  CsrScanWs s;
  s.pt_tok = reinterpret_cast<unsigned*>(w);
  s.pt_w = reinterpret_cast<float*>(w + csr_scan_align((size_t)kMaxPairs * 4));
  s.pt_q = reinterpret_cast<int*>(w + 2 * csr_scan_align((size_t)kMaxPairs * 4));
  s.part_s = reinterpret_cast<float*>(w + 3 * csr_scan_align((size_t)kMaxPairs * 4));
  s.part_i = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(s.part_s) + csr_scan_align(cells * 4));
  return s;
}

}  // namespace
}  // namespace crs
