// finish.hip -- the search tail of a tile-best fp16 scan in ONE kernel: merge + tile re-score + fp32 re-rank + certificate.
//
// crs_cosine_topk_cert used to finish a tile-best scan with three launches, each a latency-bound chain of dependent global
// round trips on one workgroup per query with HBM idle: merge_kernel (merge.hip: the k' best tile representatives out of the
// scan's [nq, nwg, kp] partial lists), refine_kernel (scan_refine.hip: those tiles' rows re-scored with the scan's MFMA
// arithmetic, the k' best rows ranked) and refine_cert_kernel (exact.hip: fp32 re-rank against the shadow + the exactness
// certificate).  This kernel runs the same three steps as phases of one 16-wave workgroup per query, with the lists between
// them in LDS.  Each phase issues its loads before it waits for any of them: three dependent round trips in all (partial
// lists, tile rows, shadow rows).  Every phase repeats its kernel's arithmetic and its ordering rules, so the outputs are
// bit for bit those of the three-kernel chain (tests/test_fused_tail_gpu.py compares the two):
//   1. merge: bucket maxima (1024 buckets of <= 16 register-held entries, slot rotation as merge.hip) -> tau = the k'-th
//      largest maximum -> entries >= tau in an LDS list -> rank by counting.  The selection is exact for any tau that is a
//      lower bound of the k'-th best, so the list size is the only thing the bucket count changes.  Overflow (thousands of
//      exact ties): k' rounds of workgroup arg-max over the register-held entries, exact as merge.hip's fallback.
//   2. tile re-score: refine_kernel's v_mfma_f32_16x16x32_f16 products in the same k-chunk order, the same admission bar
//      (k'-th representative - 1e-5 |.|), rank by counting -> the k' best rows with their slab scores, which also go to the
//      caller's candidate buffers (nothing in the kernel reads them back).
//   3. certificate: the fp32 scores through dot4_f32 (dot_f32.h, shared with exact.hip), the norms over the padded query
//      in refine_cert_kernel's 256-thread order, the same rank rule and status / ws_thr / ws_cnt / ws_done, so that
//      escalate_kernel runs after it unchanged.

#include "dot_f32.h"
#include "scan.h"
#include "wave_sort.h"

namespace crs {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kNegInfF = -__builtin_huge_valf();
constexpr int kFinThreads = 1024;
constexpr int kFinWaves = kFinThreads / 64;
constexpr int kFinRegE = 16;     // partial-list entries a thread holds (16 passes of >= 961 entries)
constexpr int kFinCap = 1024;    // phase-1 LDS list
constexpr int kFinRows = 2048;   // phase-2 LDS list: k' * tile_rows <= 2048

// the pass geometry of phase 1 (merge.hip): a pass covers whole lists and the slot rotates with the pass number
__host__ __device__ inline int fin_entries_per_pass(int kp) { return (kp > 1 && kp <= kFinThreads) ? (kFinThreads / kp) * kp : kFinThreads; }

template <int D>
__global__ __launch_bounds__(kFinThreads) void finish_cert_kernel(
    const float* __restrict__ part_s, const int* __restrict__ part_r, int nlists, int kp, const _Float16* __restrict__ q16,
    const _Float16* __restrict__ slab, int n_rows, int tile_rows, const float* __restrict__ q32, int dim,
    const float* __restrict__ shadow, int64_t id_base, int kc, int k_out, float err_rows, float err_arith,
    float* __restrict__ cand_s, int64_t* __restrict__ cand_i, float* __restrict__ out_s, int64_t* __restrict__ out_i,
    int* __restrict__ status, float* __restrict__ ws_thr, int* __restrict__ ws_cnt, int* __restrict__ ws_done) {
  constexpr int kKs = D / 32;
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
  const int lr = lane & 15, kq = lane >> 4;
  if (tid == 0) { cnt1 = 0; cnt2 = 0; kth_s = kNegInfF; }
  if (tid < kc) { win_s[tid] = kNegInfF; win_i[tid] = -1; fin_s[tid] = kNegInfF; fin_i[tid] = -1; }

  // ---- phase 1: merge ------------------------------------------------------------------------------------------
  const int m = nlists * kp;
  const float* qs = part_s + (size_t)q * m;
  const int* qr = part_r + (size_t)q * m;
  const bool rotate = kp > 1 && kp <= kFinThreads;
  const int C = fin_entries_per_pass(kp);
  const int lpp = rotate ? kFinThreads / kp : 0;
  const int list0 = rotate ? tid / kp : 0, slot0 = rotate ? tid - list0 * kp : 0;
  const int n_pass = (m + C - 1) / C;    // <= kFinRegE (finish_fits)
  float cs[kFinRegE];
  int ci[kFinRegE];
  {
    int sl = slot0;
#pragma unroll
    for (int u = 0; u < kFinRegE; ++u) {
      int e = -1;
      if (u < n_pass && tid < C) {
        const int li = list0 + u * lpp;
        e = rotate ? li * kp + sl : u * kFinThreads + tid;
        if (e >= m || (rotate && li >= nlists)) e = -1;
      }
      sl = (sl + 1 == kp) ? 0 : sl + 1;
      cs[u] = e >= 0 ? qs[e] : kNegInfF;
      ci[u] = e >= 0 ? qr[e] : -1;
    }
  }
  float best = kNegInfF;
#pragma unroll
  for (int u = 0; u < kFinRegE; ++u) best = fmaxf(best, (ci[u] >= 0) ? cs[u] : kNegInfF);
  sh_sorted[0][wave][lane] = wave_sort_desc(best, lane);
  __syncthreads();
  // top 64 of the 1024 maxima: "top 64 of two sorted lists" merges, 16 -> 8 -> 4 -> 2 lists, then every wave the last one
  int src = 0;
  for (int n = kFinWaves; n > 2; n >>= 1) {
    if (wave < n / 2)
      sh_sorted[src ^ 1][wave][lane] = wave_clean_desc(fmaxf(sh_sorted[src][2 * wave][lane], sh_sorted[src][2 * wave + 1][63 - lane]), lane);
    __syncthreads();
    src ^= 1;
  }
  const float top = wave_clean_desc(fmaxf(sh_sorted[src][0][lane], sh_sorted[src][1][63 - lane]), lane);
  const float tau = __shfl(top, kc - 1);
#pragma unroll
  for (int u = 0; u < kFinRegE; ++u) {
    if (ci[u] >= 0 && cs[u] >= tau) {
      const int p = atomicAdd(&cnt1, 1);
      if (p < kFinCap) { l_s[p] = cs[u]; l_i[p] = ci[u]; }
    }
  }
  __syncthreads();
  const int n1 = cnt1;
  if (n1 <= kFinCap) {
    for (int c = tid; c < n1; c += kFinThreads) {   // rank = slot (score desc, row asc)
      const float s = l_s[c];
      const int id = l_i[c];
      int rank = 0;
      for (int o = 0; o < n1; ++o) {
        const float so = l_s[o];
        const int io = l_i[o];
        rank += (so > s || (so == s && io < id)) ? 1 : 0;
      }
      if (rank < kc) { win_s[rank] = s; win_i[rank] = id; }
    }
  } else {   // the list overflowed (exact ties by the thousand): k' rounds of "best entry strictly after the previous winner"
    float last_s = __builtin_huge_valf();
    int last_i = -1;
    for (int r = 0; r < kc; ++r) {
      float bs = kNegInfF;
      int bi = -1;
#pragma unroll
      for (int u = 0; u < kFinRegE; ++u) {
        const float s = cs[u];
        const int id = ci[u];
        const bool after = (s < last_s) || (s == last_s && id > last_i);
        if (id >= 0 && after && (bi < 0 || s > bs || (s == bs && id < bi))) { bs = s; bi = id; }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const float os2 = __shfl_xor(bs, off);
        const int oi2 = __shfl_xor(bi, off);
        const bool take = (oi2 >= 0) && (bi < 0 || os2 > bs || (os2 == bs && oi2 < bi));
        bs = take ? os2 : bs;
        bi = take ? oi2 : bi;
      }
      const int pp = r & 1;
      if (lane == 0) { arg_s[pp][wave] = bs; arg_i[pp][wave] = bi; }
      __syncthreads();
      bs = arg_s[pp][0];
      bi = arg_i[pp][0];
      for (int w = 1; w < kFinWaves; ++w) {
        const float os2 = arg_s[pp][w];
        const int oi2 = arg_i[pp][w];
        const bool take = (oi2 >= 0) && (bi < 0 || os2 > bs || (os2 == bs && oi2 < bi));
        bs = take ? os2 : bs;
        bi = take ? oi2 : bi;
      }
      if (bi < 0) break;   // exhausted (uniform); the tail keeps (-inf, -1)
      if (tid == 0) { win_s[r] = bs; win_i[r] = bi; }
      last_s = bs;
      last_i = bi;
    }
  }
  __syncthreads();

  // ---- phase 2: re-score the k' tiles (scan_refine.hip's arithmetic) -------------------------------------------
  {
    const int halves = tile_rows / 16;
    const int units = kc * halves;
    const float t1 = win_s[kc - 1];
    const float bar = (win_i[kc - 1] >= 0) ? t1 - (1e-5f * fabsf(t1) + 1e-30f) : kNegInfF;
    f16x8 qf[kKs];   // B operand: every column carries the query
    const _Float16* qrow = q16 + (size_t)q * D + kq * 8;
#pragma unroll
    for (int ks = 0; ks < kKs; ++ks) qf[ks] = *reinterpret_cast<const f16x8*>(qrow + ks * 32);
    for (int u = wave; u < units; u += kFinWaves) {
      const int j = u / halves, hb = u % halves;
      const int w = win_i[j];
      const int first = (w < 0) ? 0 : (w / tile_rows) * tile_rows + hb * 16;
      const int row = first + lr;
      const _Float16* arow = slab + (size_t)(row < n_rows ? row : n_rows - 1) * D + kq * 8;
      f16x8 af[kKs];
#pragma unroll
      for (int ks = 0; ks < kKs; ++ks) af[ks] = *reinterpret_cast<const f16x8*>(arow + ks * 32);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < kKs; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks], qf[ks], acc, 0, 0, 0);
      if (lr == 0 && w >= 0) {
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
          const int rr = first + 4 * kq + ii;
          if (rr < n_rows && acc[ii] >= bar) {
            const int p = atomicAdd(&cnt2, 1);   // p < kc * tile_rows <= kFinRows (finish_fits)
            r_s[p] = acc[ii];
            r_i[p] = rr;
          }
        }
      }
    }
  }
  __syncthreads();
  {
    const int n2 = cnt2;
    for (int c = tid; c < n2; c += kFinThreads) {
      const float s = r_s[c];
      const int id = r_i[c];
      int rank = 0;
      for (int o = 0; o < n2; ++o) {
        const float so = r_s[o];
        const int io = r_i[o];
        rank += (so > s || (so == s && io < id)) ? 1 : 0;
      }
      if (rank < kc) { fin_s[rank] = s; fin_i[rank] = (int64_t)id + id_base; }
    }
  }
  __syncthreads();
  if (tid < kc) { cand_s[(size_t)q * kc + tid] = fin_s[tid]; cand_i[(size_t)q * kc + tid] = fin_i[tid]; }

  // ---- phase 3: fp32 re-rank + certificate (exact.hip's refine_cert_kernel) -------------------------------------
  const float* a = q32 + (size_t)q * dim;
  if (tid < 256) {   // waves 0-3: |q16 - q|^2, |q|^2, max |q16| in the certificate kernel's 256-thread order
    const _Float16* a16 = q16 + (size_t)q * D;
    float d2 = 0.f, n2 = 0.f, am = 0.f;
    for (int e = tid; e < D; e += 256) {
      const float x = e < dim ? a[e] : 0.f, h = (float)a16[e];
      d2 = fmaf(h - x, h - x, d2);
      n2 = fmaf(x, x, n2);
      am = fmaxf(am, fabsf(h));
    }
    d2 = wsum(d2);
    n2 = wsum(n2);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = fmaxf(am, __shfl_xor(am, o));
    if (lane == 0) { red[wave][0] = d2; red[wave][1] = n2; red[wave][2] = am; }
  }
  {   // candidate c is scored by wave c % 16, up to four per wave: one round trip for k' <= 64
    const float* rows[4];
    int64_t ids[4];
    bool oks[4];
    int n = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = wave + kFinWaves * u;
      ids[u] = -1; oks[u] = false; rows[u] = shadow;
      if (c < kc) {
        n = u + 1;
        ids[u] = fin_i[c];
        const int64_t row = ids[u] - id_base;
        oks[u] = ids[u] >= 0 && row >= 0 && row < n_rows;
        if (oks[u]) rows[u] = shadow + (size_t)row * dim;
      }
    }
    if (n > 0) {
      float sc[4];
      dot4_f32(a, rows, n, dim, lane, sc);
      if (lane == 0) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int c = wave + kFinWaves * u;
          if (c < kc) { cer_s[c] = oks[u] ? sc[u] : kNegInfF; cer_i[c] = oks[u] ? ids[u] : (int64_t)-1; }
        }
      }
    }
  }
  __syncthreads();
  if (tid < k_out) { out_s[(size_t)q * k_out + tid] = kNegInfF; out_i[(size_t)q * k_out + tid] = -1; }
  __syncthreads();
  if (tid < kc) {
    const float s = cer_s[tid];
    const int64_t id = cer_i[tid];
    if (id >= 0) {
      int rank = 0;
      for (int j = 0; j < kc; ++j) {
        const float sj = cer_s[j];
        const int64_t ij = cer_i[j];
        rank += (ij >= 0 && (sj > s || (sj == s && (ij < id || (ij == id && j < tid))))) ? 1 : 0;
      }
      if (rank < k_out) { out_s[(size_t)q * k_out + rank] = s; out_i[(size_t)q * k_out + rank] = id; }
      if (rank == k_out - 1) kth_s = s;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const float dd = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    const float nn = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    const float dq = sqrtf(dd) * 1.0001f;
    const float eps = dq * (1.0f + err_rows) * 1.0001f + sqrtf(nn) * err_rows * 1.0002f + err_arith;
    int valid = 0, outside = 0;
    float tmin = __builtin_huge_valf();
    for (int c = 0; c < kc; ++c) {
      const int64_t id = fin_i[c];
      if (id < 0) continue;
      if (id - id_base >= 0 && id - id_base < n_rows) { ++valid; tmin = fminf(tmin, fin_s[c]); }
      else ++outside;
    }
    const float kth = kth_s;
    int st = 1;
    if (outside == 0 && (int64_t)valid >= n_rows) {
      st = 0;
    } else if (outside == 0 && valid == kc) {
      const float bound = tmin + eps + 2e-5f * fabsf(tmin);
      st = (kth > bound) ? 0 : 1;
    }
    status[q] = st;
    ws_thr[q] = kth - eps;
    ws_cnt[q] = 0;
    if (q == 0) *ws_done = 0;
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
  if (m > 16384 || (m + fin_entries_per_pass(kp) - 1) / fin_entries_per_pass(kp) > kFinRegE) return false;
  return pdim == 128 || pdim == 256 || pdim == 384 || pdim == 512 || pdim == 640;
}

int finish_cert_launch(const float* part_s, const int* part_r, int nlists, int kp, const _Float16* q16, int nq, int pdim,
                       const _Float16* slab, int n_rows, int tile_rows, const float* q32, int dim, const float* shadow, int64_t id_base,
                       int kc, int k_out, float err_rows, float* cand_s, int64_t* cand_i, float* out_s, int64_t* out_i, int* status,
                       float* ws_thr, int* ws_cnt, int* ws_done, hipStream_t stream) {
  if (!finish_fits(nlists, kp, kc, tile_rows, pdim)) return -1;
  const float err_arith = exact_err_arith(dim, pdim);
#define CRS_FINISH(DD) hipLaunchKernelGGL((finish_cert_kernel<DD>), dim3(nq), dim3(kFinThreads), 0, stream, part_s, part_r, nlists, kp, q16, \
                                          slab, n_rows, tile_rows, q32, dim, shadow, id_base, kc, k_out, err_rows, err_arith, cand_s, cand_i, \
                                          out_s, out_i, status, ws_thr, ws_cnt, ws_done)
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
