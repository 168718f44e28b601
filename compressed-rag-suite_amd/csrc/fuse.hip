// fuse.hip -- weighted reciprocal rank fusion of a dense and a lexical result list per query, on the device (gfx950): crs_fuse_rrf.
//
// The host rule (tests/_bm25_ref.py: fuse_rrf_ref; ContextRetriever's hybrid step), restated operation for operation in fp64 so
// that the results carry the host's bits.  For a row at 0-based position i of the dense list and j of the lexical list:
//     fused = w_dense / ((c + i) + 1)  +  w_lex / ((c + j) + 1)          each quotient rounded, then the sum, dense term first;
//     a row only one list holds gets that list's term alone.
// Order: fused descending, ties by the smaller dense position (absent = infinite), then by the smaller lexical position -- a total
// order, so the output slot of a candidate is the number of candidates ahead of it (a rank count, as rerank.hip orders its lists).
// The file is compiled with fp contraction off and the expressions are plain operators.
//
// One wave per query.  Lane l owns dense slot l and lexical slot l (both lists <= CRS_MAX_K long); the <= 128 candidates are the
// dense entries and the lexical entries no dense entry repeats.  A negative row is an empty slot.  Rows are only compared, never
// dereferenced.  No atomics, no scratch, no workgroup depends on another.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"

#pragma clang fp contract(off)

namespace crs {
namespace {

constexpr int kM = CRS_MAX_K;
constexpr int kAbsent = 0x7fffffff;            // "position" of a row a list does not hold
static_assert(kM == 64, "one lane per list slot");

__device__ __forceinline__ bool ahead(double fa, int da, int la, double fb, int db, int lb) {   // a before b
  if (fa != fb) return fa > fb;
  if (da != db) return da < db;
  return la < lb;
}

__global__ __launch_bounds__(kM) void fuse_rrf_kernel(const int64_t* __restrict__ dense, int m_dense, const int64_t* __restrict__ lex,
                                                     int m_lex, double c, double w_dense, double w_lex, int k_out,
                                                     int64_t* __restrict__ out_rows, double* __restrict__ out_fused,
                                                     int* __restrict__ out_dpos, int* __restrict__ out_lpos, int* __restrict__ out_count) {
  __shared__ int64_t sh_row[2 * kM];
  __shared__ double sh_f[2 * kM];
  __shared__ int sh_d[2 * kM], sh_l[2 * kM];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int64_t d_row = lane < m_dense ? dense[(size_t)q * m_dense + lane] : (int64_t)-1;
  const int64_t l_row = lane < m_lex ? lex[(size_t)q * m_lex + lane] : (int64_t)-1;

  // where the other list holds this lane's rows (the first such slot)
  int d_in_lex = kAbsent, l_in_dense = kAbsent;
  for (int j = kM - 1; j >= 0; --j) {
    const int64_t lj = __shfl(l_row, j), dj = __shfl(d_row, j);
    if (lj >= 0 && lj == d_row) d_in_lex = j;
    if (dj >= 0 && dj == l_row) l_in_dense = j;
  }
  const double pd = (c + (double)lane) + 1.0;            // the same expression serves either list: the slot is the rank
  const double term_d = w_dense / pd, term_l = w_lex / pd;
  // candidate `lane`: the dense entry; candidate kM + lane: the lexical entry, when no dense entry repeats it
  const bool has_d = d_row >= 0, has_l = l_row >= 0 && l_in_dense == kAbsent;
  double f_d = term_d;
  if (has_d && d_in_lex != kAbsent) {
    const double pl = (c + (double)d_in_lex) + 1.0;
    const double other = w_lex / pl;
    f_d = term_d + other;
  }
  sh_row[lane] = has_d ? d_row : (int64_t)-1;
  sh_f[lane] = f_d;
  sh_d[lane] = lane;
  sh_l[lane] = d_in_lex;
  sh_row[kM + lane] = has_l ? l_row : (int64_t)-1;
  sh_f[kM + lane] = term_l;
  sh_d[kM + lane] = kAbsent;
  sh_l[kM + lane] = lane;
  __syncthreads();

  const int total = __popcll(__ballot(has_d)) + __popcll(__ballot(has_l));
  const int count = total < k_out ? total : k_out;
  const size_t base = (size_t)q * k_out;
  for (int r = count + lane; r < k_out; r += kM) { out_rows[base + r] = -1; out_fused[base + r] = 0.0; out_dpos[base + r] = -1; out_lpos[base + r] = -1; }
  if (lane == 0) out_count[q] = count;
  for (int mine = lane; mine < 2 * kM; mine += kM) {
    if (sh_row[mine] < 0) continue;
    const double f = sh_f[mine];
    const int dp = sh_d[mine], lp = sh_l[mine];
    int rank = 0;
    for (int o = 0; o < 2 * kM; ++o)
      if (sh_row[o] >= 0 && o != mine && ahead(sh_f[o], sh_d[o], sh_l[o], f, dp, lp)) ++rank;
    if (rank < count) {
      out_rows[base + rank] = sh_row[mine];
      out_fused[base + rank] = f;
      out_dpos[base + rank] = dp == kAbsent ? -1 : dp;
      out_lpos[base + rank] = lp == kAbsent ? -1 : lp;
    }
  }
}

}  // namespace

int fuse_rrf_launch(const int64_t* dense, int m_dense, const int64_t* lex, int m_lex, int nq, double c, double w_dense, double w_lex,
                    int k_out, int64_t* out_rows, double* out_fused, int* out_dpos, int* out_lpos, int* out_count, hipStream_t stream) {
  hipLaunchKernelGGL(fuse_rrf_kernel, dim3((unsigned)nq), dim3(kM), 0, stream, dense, m_dense, lex, m_lex, c, w_dense, w_lex, k_out,
                     out_rows, out_fused, out_dpos, out_lpos, out_count);
  return (int)hipGetLastError();
}

}  // namespace crs
