// finish.hip -- the search tail of a tile-best fp16 scan in ONE kernel: merge + tile re-score + fp32 re-rank + certificate.
//
// crs_cosine_topk_cert used to finish a tile-best scan with three launches, each a latency-bound chain of dependent global
// round trips on one workgroup per query with HBM idle: merge_kernel (merge.hip: the k' best tile representatives out of the
// scan's [nq, nwg, kp] partial lists), refine_kernel (scan_refine.hip: those tiles' rows re-scored with the scan's MFMA
// arithmetic, the k' best rows ranked) and refine_cert_kernel (exact.hip: fp32 re-rank against the shadow + the exactness
// certificate).  This kernel runs the same three steps as phases of one 16-wave workgroup per query, with the lists between
// them in LDS.  Each phase issues its loads before it waits for any of them: three dependent round trips in all (partial
// lists, tile rows, shadow rows).  Every phase calls the same step functions as its kernel of the chain (tail_steps.h), so the
// outputs are bit for bit those of the three-kernel chain (tests/test_fused_tail_gpu.py compares the two):
//   1. merge: bucket maxima (1024 buckets of <= 16 register-held entries, slot rotation as merge.hip: MergePasses) -> tau = the k'-th
//      largest maximum -> entries >= tau in an LDS list -> rank by counting.  The selection is exact for any tau that is a
//      lower bound of the k'-th best, so the list size is the only thing the bucket count changes.  Overflow (thousands of
//      exact ties): k' rounds of workgroup arg-max over the register-held entries, exact as merge.hip's fallback.
//   2. tile re-score: refine_kernel's v_mfma_f32_16x16x32_f16 products in the same k-chunk order, the same admission bar
//      (k'-th representative - 1e-5 |.|), rank by counting -> the k' best rows with their slab scores, which also go to the
//      caller's candidate buffers (nothing in the kernel reads them back).
//   3. certificate: the fp32 scores through score_candidates4, the norms over the padded query in refine_cert_kernel's
//      256-thread order (cert_query_partials), the same rank rule and status / ws_thr / ws_cnt / ws_done, so that
//      escalate_kernel runs after it unchanged.

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

constexpr int kFinThreads = 1024;
constexpr int kFinWaves = kFinThreads / 64;
constexpr int kFinRegE = 16;     // partial-list entries a thread holds (16 passes of >= 961 entries)
constexpr int kFinCap = 1024;    // phase-1 LDS list
constexpr int kFinRows = 2048;   // phase-2 LDS list: k' * tile_rows <= 2048

template <int D>
__global__ __launch_bounds__(kFinThreads) void finish_cert_kernel(
    const float* __restrict__ part_s, const int* __restrict__ part_r, int nlists, int kp, const _Float16* __restrict__ q16,
    const _Float16* __restrict__ slab, int n_rows, int tile_rows, const float* __restrict__ q32, int dim,
    const float* __restrict__ shadow, int64_t id_base, int kc, int k_out, float err_rows, float err_arith,
    float* __restrict__ cand_s, int64_t* __restrict__ cand_i, float* __restrict__ out_s, int64_t* __restrict__ out_i,
    int* __restrict__ status, ExactWs ws) {
  __shared__ float sh_sorted[2][kFinWaves][64];    // sorted bucket maxima of every wave, then the merge tree (two buffers)
  __shared__ float l_s[kFinCap];                   // phase 1: entries >= tau
  __shared__ int l_i[kFinCap];
  __shared__ float r_s[kFinRows];                  // phase 2: rows >= the admission bar
  __shared__ int r_i[kFinRows];
  __shared__ float win_s[64];                      // the k' best tile representatives (local rows)
  __shared__ int win_i[64];
  __shared__ float fin_s[64];                      // the k' best rows (slab score, global id)
  __shared__ int64_t fin_i[64];
  __shared__ float cer_s[64];                      // their fp32 scores
  __shared__ int64_t cer_i[64];
  __shared__ float arg_s[2][kFinWaves];
  __shared__ int arg_i[2][kFinWaves];
  __shared__ float red[4][3];
  __shared__ float kth_s;
  __shared__ int cnt1, cnt2;

  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { cnt1 = 0; cnt2 = 0; kth_s = kNegInf; }
  if (tid < kc) { win_s[tid] = kNegInf; win_i[tid] = -1; fin_s[tid] = kNegInf; fin_i[tid] = -1; }

  // ---- phase 1: merge -> win (the k' best tile representatives) ------------------------------------------------
  {
    const MergePasses<kFinThreads> g(tid, nlists, kp);    // n_pass <= kFinRegE (finish_fits)
    float cs[kFinRegE];
    int ci[kFinRegE];
    const float best = merge_load_entries<kFinRegE>(g, part_s + (size_t)q * g.m, part_r + (size_t)q * g.m, cs, ci);
    const float tau = __shfl(top64_of_sorted<kFinWaves>(sh_sorted, wave_sort_desc(best, lane), wave, lane), kc - 1);
#pragma unroll
    for (int u = 0; u < kFinRegE; ++u) merge_append(cs[u], ci[u], tau, &cnt1, kFinCap, l_s, l_i);
    __syncthreads();
    const int n1 = cnt1;
    if (n1 <= kFinCap) {
      rank_by_count<kFinThreads>(l_s, l_i, n1, kc, tid, [&](int rank, float s, int id) { win_s[rank] = s; win_i[rank] = id; });
    } else {   // the list overflowed: k' rounds of workgroup arg-max over the register-held entries
      float last_s = __builtin_huge_valf();
      int last_i = -1;
      for (int r = 0; r < kc; ++r) {
        float bs = kNegInf;
        int bi = -1;
#pragma unroll
        for (int u = 0; u < kFinRegE; ++u)
          if (argmax_after(cs[u], ci[u], last_s, last_i) && argmax_take(cs[u], ci[u], bs, bi)) { bs = cs[u]; bi = ci[u]; }
        wg_argmax<kFinWaves>(bs, bi, r, arg_s, arg_i, wave, lane);
        if (bi < 0) break;   // exhausted (uniform); the tail keeps (-inf, -1)
        if (tid == 0) { win_s[r] = bs; win_i[r] = bi; }
        last_s = bs;
        last_i = bi;
      }
    }
  }
  __syncthreads();

  // ---- phase 2: re-score the k' tiles -> fin (the k' best rows, also the caller's candidate buffers) ------------
  {
    f16x8 qf[D / 32];
    tile_query_frags<D>(q16 + (size_t)q * D, lane, qf);
    tile_rescore_f16<D, kFinWaves>(qf, slab, n_rows, tile_rows, kc, [&](int j) { return win_i[j]; },
                                   tile_bar(win_s[kc - 1], win_i[kc - 1] >= 0), wave, lane, &cnt2, r_s, r_i);   // cnt2 <= kFinRows (finish_fits)
  }
  __syncthreads();
  rank_by_count<kFinThreads>(r_s, r_i, cnt2, kc, tid, [&](int rank, float s, int id) { fin_s[rank] = s; fin_i[rank] = (int64_t)id + id_base; });
  __syncthreads();
  if (tid < kc) { cand_s[(size_t)q * kc + tid] = fin_s[tid]; cand_i[(size_t)q * kc + tid] = fin_i[tid]; }

  // ---- phase 3: fp32 re-rank + certificate ----------------------------------------------------------------------
  const float* a = q32 + (size_t)q * dim;
  if (tid < 256) cert_query_partials(a, q16 + (size_t)q * D, dim, D, tid, red);
  // candidate c is scored by wave c % 16, up to four per wave: one round trip for k' <= 64
  score_candidates4(a, shadow, dim, n_rows, id_base, wave, kFinWaves, kc, [&](int c) { return fin_i[c]; }, (int64_t)-1, lane, cer_s, cer_i);
  __syncthreads();
  rank_rescored(cer_s, cer_i, kc, k_out, tid, out_s + (size_t)q * k_out, out_i + (size_t)q * k_out, &kth_s);
  __syncthreads();
  if (tid == 0) {
    const float eps = cert_query_eps(red, D, 0, err_rows, err_arith), kth = kth_s;
    const int st = cert_verdict(kc, [&](int c) { return fin_i[c]; }, [&](int c) { return fin_s[c]; }, id_base, n_rows, kth, eps);
    cert_publish(q, st, kth, eps, status, ws.thr, ws.cnt, ws.done);
  }
}

}  // namespace

// the fused tail takes a plan when its lists fit the kernel: k' <= 64 rows from k' tiles of 16 / 32 / 64 rows (<= 2048 rows),
// <= 16 register-held partial-list entries per thread (<= 16 384 per query), rows of <= 640 elements (768: 12 bytes per lane of
// scratch at 16 waves; those plans keep the three-kernel chain)
bool finish_fits(int nlists, int kp, int kc, int tile_rows, int pdim) {
  if (kc < 1 || kc > 64 || kp < 1 || nlists < 1) return false;
  if ((tile_rows != 16 && tile_rows != 32 && tile_rows != 64) || kc * tile_rows > kFinRows) return false;
  const long m = (long)nlists * kp;
  if (m > 16384 || (m + merge_entries_per_pass<kFinThreads>(kp) - 1) / merge_entries_per_pass<kFinThreads>(kp) > kFinRegE) return false;
  return pdim == 128 || pdim == 256 || pdim == 384 || pdim == 512 || pdim == 640;
}

int finish_cert_launch(const float* part_s, const int* part_r, int nlists, int kp, const _Float16* q16, int nq, int pdim,
                       const _Float16* slab, int n_rows, int tile_rows, const float* q32, int dim, const float* shadow, int64_t id_base,
                       int kc, int k_out, float err_rows, float* cand_s, int64_t* cand_i, float* out_s, int64_t* out_i, int* status,
                       const ExactWs& ws, hipStream_t stream) {
  if (!finish_fits(nlists, kp, kc, tile_rows, pdim)) return -1;
  const float err_arith = exact_err_arith(dim, pdim);
#define CRS_FINISH(DD) hipLaunchKernelGGL((finish_cert_kernel<DD>), dim3(nq), dim3(kFinThreads), 0, stream, part_s, part_r, nlists, kp, q16, \
                                          slab, n_rows, tile_rows, q32, dim, shadow, id_base, kc, k_out, err_rows, err_arith, cand_s, cand_i, \
                                          out_s, out_i, status, ws)
  switch (pdim) {
    case 128: CRS_FINISH(128); break;
    case 256: CRS_FINISH(256); break;
    case 384: CRS_FINISH(384); break;
    case 512: CRS_FINISH(512); break;
    case 640: CRS_FINISH(640); break;
    default: return -1;
  }
#undef CRS_FINISH
  return (int)hipGetLastError();
}

}  // namespace crs
