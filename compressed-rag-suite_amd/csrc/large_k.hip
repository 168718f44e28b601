// large_k.hip -- the exactness certificate for CRS_MAX_K < k_out <= CRS_MAX_K_CERT (crs_cosine_topk_large_cert).
//
// One scan keeps at most CRS_MAX_K = 64 candidates per query, too few to over-fetch a top-1000.  A partition can: the shard's
// n_rows rows are cut into P contiguous chunks (crs_large_k_plan: chunk_rows a multiple of 16, P <= 64) and each chunk is scanned
// with k = 64 (crs_cosine_topk, id_base = the chunk's first row).  That gives P x 64 <= 4096 candidates per query with exact slab
// scores; t_c = the 64th slab score of chunk c.  This kernel re-scores every candidate in fp32 against the shadow (dot4_f32: the
// bits of the k <= 64 path), orders them (score desc, id asc) with a bitonic sort in LDS and keeps the best k_out.
//
// Certificate (tail_steps.h has the derivation of eps_q and the bound): a row missing from chunk c's list has slab score
// <= t_c, so its fp32 score is <= t_c + 2e-5 |t_c| + eps_q.  The list is the fp32 top-k_out of all n_rows rows when
//     k_out-th fp32 score > max over the chunks c that do not list every one of their rows of (t_c + eps_q + 2e-5 |t_c|)
// with the rules of refine_cert_kernel, per chunk: a chunk proves without a bound only when its list holds every row of the chunk;
// a -1 slot on a larger chunk, or an id outside the chunk, proves nothing (status 1).  Fewer than k_out valid candidates, unless
// every chunk is listed whole, cannot pass (the k_out-th score is -inf).  Status 1 also writes the escalation workspace the way
// refine_cert_kernel does (ws_thr = k_out-th fp32 score - eps_q): any k_out distinct rows bound the true k-th fp32 score from
// below, so crs_escalate_exact's sweep lists a superset of the true top-k_out and re-ranks it exactly.
//
// Sizing (crs_large_k_plan): P = clamp(ceil(k_out / 16), 2, 64) chunks, fewer on small shards, so each chunk's 64-deep list is
// about 4 x its expected share of the top-k_out (k_out / P <= 16).

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

constexpr int kLkThreads = 1024;           // 16 waves per query
constexpr int kLkSlots = 64;               // candidates per chunk (the scan's k)
constexpr int kLkMaxCand = 4096;           // 64 chunks x 64
constexpr int64_t kNoId = 0x7fffffffffffffffLL;   // empty slot while sorting: after every real row on a -inf tie

// One 1024-thread workgroup per query.  cand / cand_s: [parts, nq, 64] (chunk p of query qi at (p * nq + qi) * 64).
// LDS: 4096 x (4 + 8) B = 48 KB for the list, plus the per-chunk verdicts.
__global__ __launch_bounds__(kLkThreads) void large_cert_kernel(const float* __restrict__ q32, const _Float16* __restrict__ q16, int nq, int dim,
                                                               int pdim, int is_i8, const float* __restrict__ shadow, int64_t n_rows,
                                                               int64_t id_base, const int64_t* __restrict__ cand, const float* __restrict__ cand_s,
                                                               int parts, int64_t chunk_rows, int k_out, float err_rows, float err_arith,
                                                               float* __restrict__ out_s, int64_t* __restrict__ out_i, int* __restrict__ status,
                                                               ExactWs ws) {
  __shared__ float sh_s[kLkMaxCand];
  __shared__ int64_t sh_i[kLkMaxCand];
  __shared__ float red[4][3];
  __shared__ float ch_bound[kLkMaxCand / kLkSlots];
  __shared__ int ch_state[kLkMaxCand / kLkSlots];     // 0: the chunk lists every one of its rows, 1: bounded by ch_bound, 2: no proof
  __shared__ float eps_s;
  const int qi = blockIdx.x;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int n_c = parts * kLkSlots;
  int npow = kLkSlots;
  while (npow < n_c) npow <<= 1;
  const float* a = q32 + (size_t)qi * dim;
  if (t < 256) cert_query_partials(a, q16 + (size_t)qi * pdim, dim, pdim, t, red);

  // fp32 re-score: candidate c = chunk c / 64, slot c % 64; wave w takes c = w + 64 r + 16 u, four rows per dot4_f32
  for (int c0 = wave; c0 < n_c; c0 += 64)
    score_candidates4(a, shadow, dim, n_rows, id_base, c0, 16, n_c,
                      [&](int c) { return cand[((size_t)(c / kLkSlots) * nq + qi) * kLkSlots + (c % kLkSlots)]; }, kNoId, lane, sh_s, sh_i);
  for (int c = n_c + t; c < npow; c += kLkThreads) { sh_s[c] = kNegInf; sh_i[c] = kNoId; }
  __syncthreads();
  if (t == 0) eps_s = cert_query_eps(red, pdim, is_i8, err_rows, err_arith);

  // bitonic sort of npow (<= 4096) entries into (score desc, id asc)
  for (int k = 2; k <= npow; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = t; i < npow; i += kLkThreads) {
        const int ix = i ^ j;
        if (ix > i) {
          const float si = sh_s[i], sx = sh_s[ix];
          const int64_t ii = sh_i[i], ixx = sh_i[ix];
          const bool swap = ((i & k) == 0) ? before(sx, ixx, si, ii) : before(si, ii, sx, ixx);
          if (swap) { sh_s[i] = sx; sh_s[ix] = si; sh_i[i] = ixx; sh_i[ix] = ii; }
        }
      }
      __syncthreads();
    }
  }

  for (int o = t; o < k_out; o += kLkThreads) {
    const bool v = o < npow && sh_i[o] != kNoId;
    out_s[(size_t)qi * k_out + o] = v ? sh_s[o] : kNegInf;
    out_i[(size_t)qi * k_out + o] = v ? sh_i[o] : (int64_t)-1;
  }

  // per chunk (one wave, one slot per lane): the chunk's verdict and its bound t_c + eps_q + 2e-5 |t_c|
  const float eps = eps_s;
  for (int p = wave; p < parts; p += kLkThreads / 64) {
    const int64_t lo = (int64_t)p * chunk_rows;
    const int64_t rows_c = (n_rows - lo < chunk_rows) ? n_rows - lo : chunk_rows;
    const size_t at = ((size_t)p * nq + qi) * kLkSlots + lane;
    const int64_t id = cand[at];
    const int64_t rel = id - id_base - lo;
    const bool in_chunk = id >= 0 && rel >= 0 && rel < rows_c;
    const bool outside = id >= 0 && !in_chunk;
    const int valid = __popcll(__ballot(in_chunk));
    const bool any_out = __ballot(outside) != 0ull;
    const float tmin = wmin(in_chunk ? cand_s[at] : __builtin_huge_valf());
    if (lane == 0) {
      ch_state[p] = any_out ? 2 : (int64_t)valid >= rows_c ? 0 : valid == kLkSlots ? 1 : 2;   // (2 after "valid < 64": a -1 slot)
      ch_bound[p] = cert_bound(tmin, eps);
    }
  }
  __syncthreads();
  if (t == 0) {
    const float kth = (k_out <= npow && sh_i[k_out - 1] != kNoId) ? sh_s[k_out - 1] : kNegInf;
    int bad = 0, whole = 1;
    float bound = kNegInf;
    for (int p = 0; p < parts; ++p) {
      bad |= ch_state[p] == 2;
      if (ch_state[p] == 1) { whole = 0; bound = fmaxf(bound, ch_bound[p]); }
    }
    int st = 1;
    if (!bad) st = (whole || kth > bound) ? 0 : 1;     // (kth == -inf, fewer than k_out candidates, passes only when whole)
    cert_publish(qi, st, kth, eps, status, ws.thr, ws.cnt, ws.done);
  }
}

}  // namespace

int large_k_max_parts() { return kLkMaxCand / kLkSlots; }

int large_cert_launch(const float* q32, const _Float16* q16, int nq, int dim, int pdim, int slab_type, const float* shadow, int64_t n_rows,
                      int64_t id_base, const int64_t* cand, const float* cand_s, int parts, int64_t chunk_rows, int k_out, float err_rows,
                      float* out_s, int64_t* out_i, int* status, const ExactWs& ws, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (parts <= 0 || parts > large_k_max_parts()) return -1;
  hipLaunchKernelGGL(large_cert_kernel, dim3(nq), dim3(kLkThreads), 0, stream, q32, q16, nq, dim, pdim, slab_type == 1 ? 1 : 0, shadow, n_rows,
                     id_base, cand, cand_s, parts, chunk_rows, k_out, err_rows, exact_err_arith(dim, pdim), out_s, out_i, status, ws);
  return (int)hipGetLastError();
}

}  // namespace crs
