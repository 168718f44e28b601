// convert.hip -- exact re-score kernels (gfx950, HBM-bound).
//
//   rescore     : exact fp32 <q, shadow[id]> for over-fetched candidates + per-row re-sort.
//   refine      : the over-fetch re-rank of one query per workgroup.
//
// One wave64 per candidate row.

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

// one wave per (query, slot)
__global__ __launch_bounds__(256) void rescore_dot_kernel(const float* __restrict__ q32, int nq,
                                                         int dim, const float* __restrict__ shadow,
                                                         int64_t n_rows, int64_t id_base, int k,
                                                         float* __restrict__ scores,
                                                         const int64_t* __restrict__ ids) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= (int64_t)nq * k) return;
  const int qi = (int)(e / k);
  const int64_t id = ids[e];
  if (id < 0) {
    if (lane == 0) scores[e] = kNegInf;
    return;
  }
  const int64_t row = id - id_base;
  if (row < 0 || row >= n_rows) return;  // foreign shard: leave untouched (the caller pre-fills)
  const float* a = q32 + (size_t)qi * dim;
  const float* b = shadow + (size_t)row * dim;
  const float acc = dot_f32(a, b, dim, lane);
  if (lane == 0) scores[e] = acc;
}

// one wave per query, k <= 64: rank-by-counting sort on (score desc, id asc); empty slots last
__global__ __launch_bounds__(64) void sort_rows_kernel(int nq, int k, float* __restrict__ scores,
                                                      int64_t* __restrict__ ids) {
  const int lane = threadIdx.x;
  const int qi = blockIdx.x;
  const bool in = lane < k;
  float s = in ? scores[(size_t)qi * k + lane] : kNegInf;
  int64_t id = in ? ids[(size_t)qi * k + lane] : -1;
  if (id < 0) s = kNegInf;
  int rank = 0;
  for (int j = 0; j < k; ++j) {
    const float sj = __shfl(s, j);
    const int64_t ij = __shfl(id, j);
    bool first;  // does entry j precede this lane's entry?
    if (ij < 0) first = (id < 0) && (j < lane);
    else if (id < 0) first = true;
    else first = before(sj, ij, s, id);
    rank += first ? 1 : 0;
  }
  if (in) {
    scores[(size_t)qi * k + rank] = s;
    ids[(size_t)qi * k + rank] = id;
  }
}

// Over-fetch re-rank (crs_refine_f32): one 256-thread workgroup per query.  Wave w re-scores candidates
// w, w+4, ... (fp32 FMA over the lane's strided elements, butterfly sum), the scores meet in LDS, and the
// first k_in threads rank themselves by counting (score desc, id asc, empties last); ranks < k_out leave.
__global__ __launch_bounds__(256) void refine_f32_kernel(const float* __restrict__ q32, int dim,
                                                        const float* __restrict__ shadow, int64_t n_rows,
                                                        int64_t id_base, const int64_t* __restrict__ cand,
                                                        int k_in, int k_out, float* __restrict__ out_s,
                                                        int64_t* __restrict__ out_i) {
  __shared__ float sh_s[64];
  __shared__ int64_t sh_i[64];
  const int qi = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* a = q32 + (size_t)qi * dim;
  for (int c = wave; c < k_in; c += 4) {
    int64_t id = cand[(size_t)qi * k_in + c];
    const int64_t row = id - id_base;
    const bool ok = id >= 0 && row >= 0 && row < n_rows;
    const float acc = ok ? dot_f32(a, shadow + (size_t)row * dim, dim, lane) : 0.f;   // (ok is wave-uniform)
    if (lane == 0) { sh_s[c] = ok ? acc : kNegInf; sh_i[c] = ok ? id : (int64_t)-1; }
  }
  __syncthreads();
  rank_rescored(sh_s, sh_i, k_in, k_out, threadIdx.x, out_s + (size_t)qi * k_out, out_i + (size_t)qi * k_out, nullptr);
}

}  // namespace

int refine_f32_launch(const float* q32, int nq, int dim, const float* shadow, int64_t n_rows, int64_t id_base,
                      const int64_t* cand, int k_in, int k_out, float* out_s, int64_t* out_i, hipStream_t stream) {
  if (nq <= 0) return 0;
  hipLaunchKernelGGL(refine_f32_kernel, dim3(nq), dim3(256), 0, stream, q32, dim, shadow, n_rows, id_base, cand,
                     k_in, k_out, out_s, out_i);
  return (int)hipGetLastError();
}

// fp32 scores of arbitrary candidate lists (any k): out[e] = <q32[e / k], shadow[ids[e] - id_base]>, -inf for ids < 0
int score_rows_launch(const float* q32, int nq, int dim, const float* shadow, int64_t n_rows, int64_t id_base, int k, const int64_t* ids,
                      float* scores, hipStream_t stream) {
  const int64_t e = (int64_t)nq * k;
  if (e <= 0) return 0;
  hipLaunchKernelGGL(rescore_dot_kernel, dim3((unsigned)((e + 3) / 4)), dim3(256), 0, stream, q32, nq, dim, shadow, n_rows, id_base, k,
                     scores, ids);
  return (int)hipGetLastError();
}

int rescore_launch(const float* q32, int nq, int dim, const float* shadow, int64_t n_rows,
                   int64_t id_base, int k, float* scores, int64_t* ids, hipStream_t stream) {
  const int64_t e = (int64_t)nq * k;
  if (e <= 0) return 0;
  hipLaunchKernelGGL(rescore_dot_kernel, dim3((unsigned)((e + 3) / 4)), dim3(256), 0, stream, q32,
                     nq, dim, shadow, n_rows, id_base, k, scores, ids);
  hipLaunchKernelGGL(sort_rows_kernel, dim3(nq), dim3(64), 0, stream, nq, k, scores, ids);
  return (int)hipGetLastError();
}

}  // namespace crs
