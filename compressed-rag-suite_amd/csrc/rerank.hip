// rerank.hip -- score, threshold and lexically re-rank retrieved lists on the device (gfx950): crs_rerank_lexical.
//
// The post-search half of ContextRetriever.retrieve_batch (rag/retrieval.py: the cosine score, similarity_threshold, _rerank and
// its stable sort) for the <= 64 candidates of one query, restated operation for operation in fp64 so that the results carry the
// host's bits:
//     dist = (double)(1.0f - score)                       fp32 subtraction, as search_batch / retrieve_batch take the distance
//     d    = min(max(dist, 0), 2);   sim = min(max(1 - d * d / 2, 0), 1)          a NaN stays a NaN (numpy's minimum / maximum)
//     keep = sim >= threshold                                                     (a NaN drops)
//     kept > k:  hits = |query ids & row ids|,  rr = sim * 0.7 + (hits / q_norm) * 0.3,  order by rr descending, ties by list
//                position ascending (Python's stable sort(reverse=True)), cut to k
//     else:      the first min(kept, k) kept positions in list order
// Every product, quotient, sum and difference above is rounded on its own: the file is compiled with fp contraction off and the
// expressions are written as plain operators (the __dmul_rn family is `x * y` in a header that is compiled with contraction on).
//
// One wave per query, lane c owning candidate c.  The tokens of a chunk are a sorted segment of an int32 CSR (rag/indexing.py:
// SlabCollection._token_csr), the known tokens of the query another; the query's ids are staged in LDS kQC at a time (any number
// of them: the chunk loop runs until they are through) and each lane counts its row's hits against the staged ids either by
// walking its row and searching the staged ids, or by walking the staged ids and searching its row -- whichever reads less global
// memory (a 5000-token chunk against a 6-token query: 6 x 13 reads instead of 5000).  The stable order is a rank count: the rank
// of lane i is the number of kept lanes j with rr_j > rr_i, or rr_j == rr_i and j < i.
//
// A row id outside [0, n_rows) is never dereferenced (such a candidate has no hits), and every CSR offset is clamped into its
// token array before it becomes an address.  No atomics, no scratch, no workgroup depends on another.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"

#pragma clang fp contract(off)

namespace crs {
namespace {

constexpr int kM = CRS_MAX_K;        // longest list: one lane per candidate
constexpr int kQC = 128;             // query ids staged per round
static_assert(kM == 64, "one lane per candidate");

// is `t` among the n ascending distinct ints at a?
template <typename Index>
__device__ __forceinline__ bool contains(const int* a, Index n, int t) {
  Index lo = 0, hi = n;
  while (lo < hi) {
    const Index mid = lo + ((hi - lo) >> 1);
    if (a[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo < n && a[lo] == t;
}

__device__ __forceinline__ int64_t clamp_i64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kM) void rerank_lexical_kernel(const float* __restrict__ scores, const int64_t* __restrict__ rows, int m_max,
                                                           const int64_t* __restrict__ doc_off, const int* __restrict__ doc_tok,
                                                           int64_t n_rows, int64_t n_doc_tok, const int64_t* __restrict__ q_off,
                                                           const int* __restrict__ q_tok, int64_t n_q_tok,
                                                           const int* __restrict__ q_norm, int k, double threshold,
                                                           int* __restrict__ order, int* __restrict__ out_count,
                                                           double* __restrict__ sim_out, double* __restrict__ rr_out,
                                                           int* __restrict__ reranked) {
  __shared__ int sh_q[kQC];
  const int q = blockIdx.x, lane = threadIdx.x;
  const size_t base = (size_t)q * m_max;
  const bool slot = lane < m_max;
  const int64_t row = slot ? rows[base + lane] : (int64_t)-1;

  // ---- score and threshold ----
  double sim = 0.0;
  bool keep = false;
  if (row >= 0) {
    const double dist = (double)(1.0f - scores[base + lane]);
    if (dist != dist) {
      sim = __longlong_as_double(0x7ff8000000000000ll);
    } else {
      const double d = fmin(fmax(dist, 0.0), 2.0);
      const double half = d * d / 2.0;
      sim = fmin(fmax(1.0 - half, 0.0), 1.0);
    }
    keep = sim >= threshold;
  }
  const unsigned long long kept_mask = __ballot(keep);
  const int kept = __popcll(kept_mask);
  const bool rerank = kept > k;                         // uniform: the block is one wave
  const int count = kept < k ? kept : k;
  int rank = __popcll(kept_mask & ((1ull << lane) - 1ull));   // list order among the kept
  double rr = 0.0;

  if (rerank) {
    // ---- hits: |query ids & row ids| ----
    int64_t q_lo = clamp_i64(q_off[q], 0, n_q_tok), q_hi = clamp_i64(q_off[q + 1], q_lo, n_q_tok);
    int64_t d_lo = 0, d_hi = 0;
    if (keep && row < n_rows) {
      d_lo = clamp_i64(doc_off[row], 0, n_doc_tok);
      d_hi = clamp_i64(doc_off[row + 1], d_lo, n_doc_tok);
    }
    const int64_t d_len = d_hi - d_lo;
    const int steps = 64 - __clzll((unsigned long long)d_len);         // reads of one search of the row
    int hits = 0;
    for (int64_t c0 = q_lo; c0 < q_hi; c0 += kQC) {
      const int n = (int)(q_hi - c0 < kQC ? q_hi - c0 : kQC);
      if (c0 > q_lo) __syncthreads();                   // the previous ids have been read
      for (int i = lane; i < n; i += kM) sh_q[i] = q_tok[c0 + i];
      __syncthreads();
      if (d_len > 0) {
        if (d_len <= (int64_t)n * steps) {
          for (int64_t t = d_lo; t < d_hi; ++t) hits += contains(sh_q, n, doc_tok[t]) ? 1 : 0;
        } else {
          for (int i = 0; i < n; ++i) hits += contains(doc_tok + d_lo, d_len, sh_q[i]) ? 1 : 0;
        }
      }
    }
    if (keep) {
      int norm = q_norm[q];
      norm = norm < 1 ? 1 : norm;
      const double frac = (double)hits / (double)norm;
      const double a = sim * 0.7, b = frac * 0.3;
      rr = a + b;
    }
    // ---- stable descending order by rank count ----
    rank = 0;
    for (int j = 0; j < kM; ++j) {
      const double rj = __shfl(rr, j);
      if (((kept_mask >> j) & 1ull) && (rj > rr || (rj == rr && j < lane))) ++rank;
    }
  }

  if (slot) {
    sim_out[base + lane] = sim;
    rr_out[base + lane] = rr;
    if (lane >= count) order[base + lane] = -1;
  }
  if (keep && rank < count) order[base + rank] = lane;
  if (lane == 0) {
    out_count[q] = count;
    reranked[q] = rerank ? 1 : 0;
  }
}

}  // namespace

int rerank_lexical_launch(const float* scores, const int64_t* rows, int nq, int m_max, const int64_t* doc_off, const int* doc_tok,
                          int64_t n_rows, int64_t n_doc_tok, const int64_t* q_off, const int* q_tok, int64_t n_q_tok, const int* q_norm,
                          int k, double threshold, int* order, int* out_count, double* sim, double* rr, int* reranked, hipStream_t stream) {
  hipLaunchKernelGGL(rerank_lexical_kernel, dim3((unsigned)nq), dim3(kM), 0, stream, scores, rows, m_max, doc_off, doc_tok, n_rows,
                     n_doc_tok, q_off, q_tok, n_q_tok, q_norm, k, threshold, order, out_count, sim, rr, reranked);
  return (int)hipGetLastError();
}

}  // namespace crs
