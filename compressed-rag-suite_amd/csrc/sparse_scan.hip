// sparse_scan.hip -- exact, flat, doc-at-a-time impact top-k over a weighted token CSR (gfx950): crs_sparse_topk.
//
// The weighted twin of bm25.hip for learned sparse retrieval (SPLADE): a row is the ascending token ids of a document's sparse
// vector with one fp32 weight each (rag/indexing.py: _SparseIndex), a query the same, and the relevance is their dot product.
//
// Arithmetic (fp32, every operation rounded on its own: the file is compiled with fp contraction off), for a row d and a query q,
// over the tokens t both hold, in ascending token id:
//     term  = q_w[t] * d_w[t]
//     score = (((0 + term_1) + term_2) + ...)
// A row with no token in common with the query is no hit and never enters a list, whatever its score would round to.
//
// The pair table, the tile walk, the list insertion, the geometry and the merge are bm25.hip's (csr_scan.h): one wave per
// workgroup, lane d owns row d of a 64-row tile, the tile's token segment is staged into LDS in chunks of 2048, a match reads the
// row's weight and adds the product into acc[q * 64 + d].  Every CSR offset is clamped into its array before it becomes an
// address; a malformed CSR or query table can give wrong scores, never an access outside the buffers.  No atomics, no scratch, no
// workgroup waits on another.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "csr_scan.h"
#include "scan.h"

#pragma clang fp contract(off)

namespace crs {
namespace {

// dynamic LDS: csr_scan.h's csr_scan_lds_bytes
__global__ __launch_bounds__(kLanes) void sparse_scan_kernel(const int64_t* __restrict__ doc_off, const int* __restrict__ doc_tok,
                                                            const float* __restrict__ doc_w, int n_rows, int64_t n_doc_tok,
                                                            const unsigned* __restrict__ pt_tok, const float* __restrict__ pt_w,
                                                            const int* __restrict__ pt_q, int n_pairs, int nq, int k, int tiles_per_wg,
                                                            float* __restrict__ part_s, int64_t* __restrict__ part_i) {
  extern __shared__ __attribute__((aligned(16))) char sparse_smem[];
  unsigned* s_tok = reinterpret_cast<unsigned*>(sparse_smem);
  float* s_w = reinterpret_cast<float*>(s_tok + n_pairs);
  float* acc = s_w + n_pairs;
  float* ls_s = acc + (size_t)nq * kLanes;
  int* ls_r = reinterpret_cast<int*>(ls_s + (size_t)nq * k);
  unsigned* stage = reinterpret_cast<unsigned*>(ls_r + (size_t)nq * k);
  unsigned char* s_q = reinterpret_cast<unsigned char*>(stage + kChunk);

  const int lane = threadIdx.x;
  for (int i = lane; i < n_pairs; i += kLanes) { s_tok[i] = pt_tok[i]; s_w[i] = pt_w[i]; s_q[i] = (unsigned char)pt_q[i]; }
  for (int i = lane; i < nq * k; i += kLanes) { ls_s[i] = kNegInf; ls_r[i] = -1; }
  __syncthreads();

  const int n_tiles = (n_rows + kLanes - 1) / kLanes;
  const int tile0 = blockIdx.x * tiles_per_wg;
  const int tile1 = (n_tiles - tile0 < tiles_per_wg) ? n_tiles : tile0 + tiles_per_wg;
  for (int tile = tile0; tile < tile1 && n_pairs > 0; ++tile) {
    const int row = tile * kLanes + lane;
    int64_t lo = 0, hi = 0;
    if (row < n_rows) {
      lo = clamp_i64(doc_off[row], 0, n_doc_tok);
      hi = clamp_i64(doc_off[row + 1], lo, n_doc_tok);
    }
    // the tile's segment of the token array: [smallest lo, largest hi) over the rows that hold tokens
    int64_t seg_lo = lo < hi ? lo : n_doc_tok, seg_hi = lo < hi ? hi : 0;
    for (int s = 32; s > 0; s >>= 1) {
      const int64_t a = __shfl_xor(seg_lo, s), b = __shfl_xor(seg_hi, s);
      seg_lo = a < seg_lo ? a : seg_lo;
      seg_hi = b > seg_hi ? b : seg_hi;
    }
    if (seg_lo >= seg_hi) continue;                    // (uniform) a tile of empty rows
    for (int q = 0; q < nq; ++q) acc[q * kLanes + lane] = 0.0f;
    unsigned long long mine = 0ull;                    // the queries this row hit
    for (int64_t base = seg_lo; base < seg_hi; base += kChunk) {
      const int n = (int)(seg_hi - base < kChunk ? seg_hi - base : kChunk);
      __syncthreads();                                 // the previous chunk has been read
      for (int i = lane; i < n; i += kLanes) stage[i] = (unsigned)doc_tok[base + i];
      __syncthreads();
      const int64_t a = lo > base ? lo : base, b = hi < base + n ? hi : base + n;
      for (int64_t t = a; t < b; ++t) {
        const unsigned tok = stage[t - base];
        int i = 0, j = n_pairs;
        while (i < j) {
          const int mid = (i + j) >> 1;
          if (s_tok[mid] < tok) i = mid + 1; else j = mid;
        }
        if (i < n_pairs && s_tok[i] == tok) {
          const float dw = doc_w[t];
          do {
            const int q = s_q[i];
            const float term = s_w[i] * dw;
            acc[q * kLanes + lane] = acc[q * kLanes + lane] + term;
            mine |= 1ull << q;
            ++i;
          } while (i < n_pairs && s_tok[i] == tok);
        }
      }
    }
    csr_select_tile(acc, mine, nq, k, tile, lane, ls_s, ls_r);
  }
  __syncthreads();
  const size_t out0 = (size_t)blockIdx.x * nq * k;
  for (int i = lane; i < nq * k; i += kLanes) { part_s[out0 + i] = ls_s[i]; part_i[out0 + i] = (int64_t)ls_r[i]; }
}

}  // namespace

size_t sparse_workspace_bytes(int nq, int k, int64_t n_rows) { return csr_scan_workspace_bytes(nq, k, n_rows); }

int sparse_topk_launch(const int64_t* doc_off, const int* doc_tok, const float* doc_w, int64_t n_rows, int64_t n_doc_tok,
                       const int64_t* q_off, const int* q_tok, const float* q_w, int nq, int n_pairs, int k, void* workspace, float* out_s,
                       int64_t* out_i, hipStream_t stream) {
  int n_wg, per;
  csr_scan_plan(n_rows, &n_wg, &per);
  const CsrScanWs ws = csr_scan_ws(workspace, n_wg, nq, k);
  if (n_pairs > 0)
    hipLaunchKernelGGL(csr_pairs_kernel, dim3(1), dim3(kSortThreads), 0, stream, q_off, q_tok, q_w, nq, n_pairs, ws.pt_tok, ws.pt_w, ws.pt_q);
  const size_t lds = csr_scan_lds_bytes(nq, k, n_pairs);
  if (lds > 48 * 1024) {     // beyond the default dynamic-LDS limit (at most ~100 KiB of the CU's 160: 4096 pairs, 64 queries, k = 64)
    const hipError_t ae = hipFuncSetAttribute(reinterpret_cast<const void*>(&sparse_scan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (ae != hipSuccess) return (int)ae;
  }
  hipLaunchKernelGGL(sparse_scan_kernel, dim3((unsigned)n_wg), dim3(kLanes), lds, stream, doc_off, doc_tok, doc_w, (int)n_rows, n_doc_tok,
                     ws.pt_tok, ws.pt_w, ws.pt_q, n_pairs, nq, k, per, ws.part_s, ws.part_i);
  const int e = (int)hipGetLastError();
  if (e) return e;
  return merge_launch_i64(ws.part_s, ws.part_i, n_wg, nq, k, k, out_s, out_i, stream);
}

}  // namespace crs
