// scan_refine.hip -- second stage of the "tile best" scan variants (scan.hip dump mode, scan_wide.hip).
//
// Those kernels keep, per query and tile, only the tile's BEST SCORE, filed under the tile's first row; tail_steps.h
// (tile_rescore_f16) has the proof that this is exact.  This kernel re-opens the k best tiles per query, re-scores their rows
// with the scan's own arithmetic and ranks the (<= 2048, typically ~k) candidates by counting: one workgroup per query, the
// final sorted (score desc, row asc) top-k comes out directly.

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

// 16 waves per query: wave u re-scores 16-row block u (and u + 16) of the k winning tiles, so the whole
// re-score is at most two dependent global round trips; every load is unconditional (rows past the
// end are clamped and masked afterwards) so that the D/32 loads of a block are all in flight at once.
constexpr int kRefThreads = 1024;

// TH threads per workgroup: 1024 (16 waves x <= 128 registers) up to 768-element rows; 896 / 1024-element rows keep their
// query fragments (D / 8 registers) in 8 waves x <= 256 registers instead of spilling
template <int D, int TH>
__global__ __launch_bounds__(TH) void refine_kernel(const _Float16* __restrict__ q16, const _Float16* __restrict__ slab,
                                                            int n_rows, const float* __restrict__ win_s,
                                                            const int64_t* __restrict__ win, int k, int tile_rows, int64_t id_base, float* __restrict__ out_s,
                                                            int64_t* __restrict__ out_i) {
  __shared__ float cs[2048];   // k * tile_rows <= 16 * 64 (chain kernels) or 64 * 32 (dump mode, k <= 64)
  __shared__ int ci[2048];
  __shared__ int cnt;
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  float* os = out_s + (size_t)q * k;
  int64_t* oi = out_i + (size_t)q * k;
  const int64_t* qw = win + (size_t)q * k;
  if (tid == 0) cnt = 0;
  for (int r = tid; r < k; r += TH) { os[r] = kNegInf; oi[r] = -1; }
  const float bar = tile_bar(win_s[(size_t)q * k + k - 1], qw[k - 1] >= 0);
  f16x8 qf[D / 32];
  tile_query_frags<D>(q16 + (size_t)q * D, lane, qf);
  __syncthreads();
  tile_rescore_f16<D, TH / 64>(qf, slab, n_rows, tile_rows, k, [&](int j) { return (int)qw[j]; }, bar, wave, lane, &cnt, cs, ci);
  __syncthreads();
  rank_by_count<TH>(cs, ci, cnt, k, tid, [&](int rank, float s, int id) { os[rank] = s; oi[rank] = (int64_t)id + id_base; });
}

// ---- int8 slabs (scan_i8.hip, tile-best modes).  The scan's score is exact integer arithmetic up to the final
// scaling: q16 = rint(q / sq), sq = max|q| / 32512, q16 = 256 hi + lo, score = (256 S_hi + S_lo) * sq * s_row
// with S_x = sum_k row[k] x[k] in int32.  This kernel forms the same integers with plain VALU dot products (one
// wave per row, D/64 bytes per lane) and applies the same float operations in the same order, so a re-scored
// row carries bit for bit the score the scan gave it.
template <int D>
__global__ __launch_bounds__(kRefThreads) void refine_i8_kernel(const _Float16* __restrict__ q16, const signed char* __restrict__ slab,
                                                               const float* __restrict__ scales, int n_rows,
                                                               const float* __restrict__ win_s, const int64_t* __restrict__ win,
                                                               int k, int tile_rows, int64_t id_base,
                                                               float* __restrict__ out_s, int64_t* __restrict__ out_i) {
  constexpr int BPL = D / 64;                  // bytes of a row per lane (4, 8, 12 or 16)
  __shared__ float cs[2048];
  __shared__ int ci[2048];
  __shared__ int cnt;
  __shared__ float red[16];
  __shared__ short qhi[D], qlo[D];
  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) cnt = 0;
  for (int r = tid; r < k; r += kRefThreads) { out_s[(size_t)q * k + r] = kNegInf; out_i[(size_t)q * k + r] = -1; }
  // query scale: max |q| over the row (a max is order-independent, so this equals the scan's value)
  const _Float16* qrow = q16 + (size_t)q * D;
  float amax = 0.f;
  for (int c = tid; c < D; c += kRefThreads) amax = fmaxf(amax, fabsf((float)qrow[c]));
  amax = wmax(amax);
  if (lane == 0) red[wave] = amax;
  __syncthreads();
  amax = red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) amax = fmaxf(amax, red[w]);
  const float qscale = amax > 0.f ? amax / 32512.0f : 1.0f;
  for (int c = tid; c < D; c += kRefThreads) {
    const int v = (int)rintf((float)qrow[c] / qscale);
    const int lo = ((v + 128) & 255) - 128;
    qlo[c] = (short)lo;
    qhi[c] = (short)((v - lo) >> 8);
  }
  const float t1 = win_s[(size_t)q * k + k - 1];
  const float tau = (win[(size_t)q * k + k - 1] >= 0) ? t1 : kNegInf;   // identical arithmetic: no margin needed
  __syncthreads();

  int myhi[BPL], mylo[BPL];                    // this lane's columns lane * BPL .. + BPL - 1, the same for every row
#pragma unroll
  for (int j = 0; j < BPL; ++j) { myhi[j] = qhi[lane * BPL + j]; mylo[j] = qlo[lane * BPL + j]; }
  const int nrows = k * tile_rows;             // <= 64 * 32
  for (int u = wave; u < nrows; u += kRefThreads / 64) {
    const int64_t w = win[(size_t)q * k + u / tile_rows];
    if (w < 0) continue;                        // wave-uniform
    const int row = (int)w + (u % tile_rows);
    if (row >= n_rows) continue;
    const signed char* src = slab + (size_t)row * D + lane * BPL;
    int shi = 0, slo = 0;
#pragma unroll
    for (int wd = 0; wd < BPL / 4; ++wd) {
      const int bits = *reinterpret_cast<const int*>(src + wd * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int x = (bits << (24 - 8 * e)) >> 24;     // sign-extended byte e
        shi += x * myhi[wd * 4 + e];
        slo += x * mylo[wd * 4 + e];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { shi += __shfl_xor(shi, o); slo += __shfl_xor(slo, o); }
    if (lane == 0) {
      const float sc = ((float)shi * 256.0f + (float)slo) * qscale * scales[row];
      if (sc >= tau) {
        const int p = atomicAdd(&cnt, 1);
        cs[p] = sc;
        ci[p] = row;
      }
    }
  }
  __syncthreads();
  rank_by_count<kRefThreads>(cs, ci, cnt, k, tid, [&](int rank, float s, int id) {
    out_s[(size_t)q * k + rank] = s;
    out_i[(size_t)q * k + rank] = (int64_t)id + id_base;
  });
}

}  // namespace

int refine_i8_launch(const _Float16* q16, int nq, int pdim, const void* slab, const float* scales, int n_rows, const float* win_s,
                     const int64_t* win, int k, int tile_rows, int64_t id_base, float* out_s, int64_t* out_i, hipStream_t stream) {
  if (k > 64 || tile_rows != 32) return -1;
#define CRS_REFINE8(DD) hipLaunchKernelGGL((refine_i8_kernel<DD>), dim3(nq), dim3(kRefThreads), 0, stream, q16, \
                                          reinterpret_cast<const signed char*>(slab), scales, n_rows, win_s, win, k, tile_rows, id_base, out_s, out_i)
  switch (pdim) {
    case 256: CRS_REFINE8(256); break;
    case 512: CRS_REFINE8(512); break;
    case 768: CRS_REFINE8(768); break;
    case 1024: CRS_REFINE8(1024); break;
    default: return -1;
  }
#undef CRS_REFINE8
  return (int)hipGetLastError();
}

int refine_launch(const _Float16* q16, int nq, int pdim, const _Float16* slab, int n_rows, const float* win_s,
                  const int64_t* win, int k, int tile_rows, int64_t id_base, float* out_s, int64_t* out_i, hipStream_t stream) {
  if (k > 64 || (tile_rows != 16 && tile_rows != 32 && tile_rows != 64) || k * tile_rows > 2048) return -1;
#define CRS_REFINE(DD) hipLaunchKernelGGL((refine_kernel<DD, (DD >= 896 ? 512 : 1024)>), dim3(nq), dim3(DD >= 896 ? 512 : 1024), 0, stream, q16, slab, \
                                         n_rows, win_s, win, k, tile_rows, id_base, out_s, out_i)
  switch (pdim) {
    case 128: CRS_REFINE(128); break;
    case 256: CRS_REFINE(256); break;
    case 384: CRS_REFINE(384); break;
    case 512: CRS_REFINE(512); break;
    case 640: CRS_REFINE(640); break;
    case 768: CRS_REFINE(768); break;
    case 896: CRS_REFINE(896); break;
    case 1024: CRS_REFINE(1024); break;
    default: return -1;
  }
#undef CRS_REFINE
  return (int)hipGetLastError();
}

}  // namespace crs
