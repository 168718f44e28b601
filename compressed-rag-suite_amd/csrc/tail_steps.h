// tail_steps.h -- the steps of the search tail (everything after the scan), one definition each.
//
// The tail is merge -> tile re-score -> fp32 re-rank -> certificate -> escalation.  It runs as a chain of kernels (merge.hip,
// scan_refine.hip, convert.hip / exact.hip, large_k.hip) and as one fused kernel (finish.hip).  Those kernels own their staging
// (what lives in LDS, which thread loads what, the barriers) and compose the functions below, so a tie rule, the admission bar
// or the certificate's slack is written once and the chain and the fused kernel cannot drift apart.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace crs {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr float kNegInf = -__builtin_huge_valf();

// ---- wave64 butterflies ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wsum(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
__device__ __forceinline__ float wmax(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fmaxf(x, __shfl_xor(x, o));
  return x;
}
__device__ __forceinline__ float wmin(float x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x = fminf(x, __shfl_xor(x, o));
  return x;
}

// full bitonic sort (descending by lane) of one value per lane across a wave64
__device__ __forceinline__ float wave_sort_desc(float v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const float o = __shfl_xor(v, j);
      const bool lower = (lane & j) == 0;
      const bool desc = (lane & k) == 0;       // k == 64: always descending
      const bool want_max = (lower == desc);
      v = want_max ? fmaxf(v, o) : fminf(v, o);
    }
  }
  return v;
}
// v is a bitonic sequence across the wave -> sorted descending
__device__ __forceinline__ float wave_clean_desc(float v, int lane) {
#pragma unroll
  for (int j = 32; j > 0; j >>= 1) {
    const float o = __shfl_xor(v, j);
    v = ((lane & j) == 0) ? fmaxf(v, o) : fminf(v, o);
  }
  return v;
}

// ---- the order of every list of the tail: score desc, id asc ------------------------------------------------------------------------
template <typename IdT>
__device__ __forceinline__ bool before(float s, IdT id, float s2, IdT id2) {
  return s > s2 || (s == s2 && id < id2);
}

// Rank an LDS list of n (score, id) pairs by counting; store(rank, s, id) receives the entries of rank < k.  TH threads.
template <int TH, typename IdT, typename Store>
__device__ __forceinline__ void rank_by_count(const float* ls, const IdT* li, int n, int k, int tid, Store store) {
  for (int c = tid; c < n; c += TH) {
    const float s = ls[c];
    const IdT id = li[c];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += before<IdT>(ls[o], li[o], s, id) ? 1 : 0;
    if (rank < k) store(rank, s, id);
  }
}

// The <= 64 fp32-re-scored candidates of a query (LDS, id < 0 = empty slot) -> the query's k_out output slots.  Empty slots are
// skipped, equal (score, id) pairs keep their slot order, unfilled outputs stay (-inf, -1).  kth_s (LDS, preset to -inf by the
// caller, or null) receives the k_out-th score.  Called by every thread after the barrier that completes the list.
__device__ __forceinline__ void rank_rescored(const float* sh_s, const int64_t* sh_i, int k_in, int k_out, int t, float* __restrict__ out_s,
                                              int64_t* __restrict__ out_i, float* kth_s) {
  if (t < k_out) { out_s[t] = kNegInf; out_i[t] = -1; }
  __syncthreads();
  if (t < k_in) {
    const float s = sh_s[t];
    const int64_t id = sh_i[t];
    if (id >= 0) {
      int rank = 0;
      for (int j = 0; j < k_in; ++j) {
        const float sj = sh_s[j];
        const int64_t ij = sh_i[j];
        rank += (ij >= 0 && (sj > s || (sj == s && (ij < id || (ij == id && j < t))))) ? 1 : 0;
      }
      if (rank < k_out) { out_s[rank] = s; out_i[rank] = id; }
      if (kth_s && rank == k_out - 1) *kth_s = s;
    }
  }
}

// ---- fp32 candidate scoring ------------------------------------------------------------------------------------------------------
// up to four rows at once (loads of all rows in flight together: one HBM round trip instead of four); per row the
// identical FMA order as a single-row lane-strided FMA chain + butterfly (dot_f32 below)
__device__ __forceinline__ void dot4_f32(const float* __restrict__ a, const float* const* __restrict__ rows, int n, int dim, int lane,
                                         float* __restrict__ out) {
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int e = lane; e < dim; e += 64) {
    const float x = a[e];
    float y[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) y[u] = (u < n) ? rows[u][e] : 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = fmaf(x, y[u], acc[u]);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) out[u] = wsum(acc[u]);
}
__device__ __forceinline__ float dot_f32(const float* __restrict__ a, const float* __restrict__ b, int dim, int lane) {
  float acc = 0.f;
  for (int e = lane; e < dim; e += 64) acc = fmaf(a[e], b[e], acc);
  return wsum(acc);
}

// One wave scores candidates c0, c0 + stride, .. (up to four, those below n_c): id_at(c) -> in-shard check -> shadow row ->
// dot4_f32 -> (score, id) into ls / li at c.  A candidate that is empty or outside [id_base, id_base + n_rows) leaves (-inf, empty).
template <typename IdAt>
__device__ __forceinline__ void score_candidates4(const float* __restrict__ a, const float* __restrict__ shadow, int dim, int64_t n_rows,
                                                  int64_t id_base, int c0, int stride, int n_c, IdAt id_at, int64_t empty, int lane,
                                                  float* ls, int64_t* li) {
  const float* rows[4];
  int64_t ids[4];
  bool oks[4];
  int n = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int c = c0 + stride * u;
    ids[u] = -1; oks[u] = false; rows[u] = shadow;
    if (c < n_c) {
      n = u + 1;
      ids[u] = id_at(c);
      const int64_t row = ids[u] - id_base;
      oks[u] = ids[u] >= 0 && row >= 0 && row < n_rows;
      if (oks[u]) rows[u] = shadow + (size_t)row * dim;
    }
  }
  if (n == 0) return;   // (wave-uniform)
  float sc[4];
  dot4_f32(a, rows, n, dim, lane, sc);
  if (lane == 0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + stride * u;
      if (c < n_c) { ls[c] = oks[u] ? sc[u] : kNegInf; li[c] = oks[u] ? ids[u] : empty; }
    }
  }
}

// ---- fp16 tile re-score ----------------------------------------------------------------------------------------------------------
// The tile-best scans (scan.hip dump mode, scan_wide.hip, scan_tb.hip, scan_w1.hip) keep, per query and tile, only the tile's BEST
// SCORE, filed under the tile's first row, instead of filtering every score against a running threshold.  That is exact:
//   order representatives by (best score desc, tile asc) -- before() with id = first row.  Let x be a row of the final top-k
//   (order: score desc, row asc) and X its tile.  If X were not among the k best tiles, k tiles Y_1..Y_k would precede it; Y_i
//   holds a row y_i with score(y_i) = best(Y_i) > best(X) >= score(x), or with score(y_i) = best(X) >= score(x) and Y_i < X,
//   i.e. row(y_i) < row(x) because tiles are contiguous row ranges -- k distinct rows beat x, a contradiction.  Hence the k best
//   tiles contain every top-k row, and no arg-max is ever needed.
// The re-score opens those k tiles again (16, 32 or 64 rows each) with the scan's own arithmetic (v_mfma_f32_16x16x32_f16, same
// k-chunk order) and keeps the rows that reach the bar.
//
// The bar: only rows scoring >= the k-th best tile representative t1 can reach the final top-k (that score is attained by k
// distinct rows already).  A hair below it: scan_wide.hip forms the same dot products with the 32x32x16 MFMA shape, and nothing
// promises the two shapes round the last bit alike; a lower bar only admits a few more candidates.
__device__ __forceinline__ float tile_bar(float t1, bool have_k) { return have_k ? t1 - (1e-5f * fabsf(t1) + 1e-30f) : kNegInf; }

// B operand: every column carries the query (lane (n, kq) holds Q[32 ks + 8 kq .. + 8])
template <int D>
__device__ __forceinline__ void tile_query_frags(const _Float16* __restrict__ qrow, int lane, f16x8 (&qf)[D / 32]) {
#pragma unroll
  for (int ks = 0; ks < D / 32; ++ks) qf[ks] = *reinterpret_cast<const f16x8*>(qrow + (lane >> 4) * 8 + ks * 32);
}

// NWAVES waves: wave u re-scores 16-row block u, u + NWAVES, .. of the k winning tiles (win_at(j): a row of tile j, < 0 = none);
// every load is unconditional (rows past the end are clamped and masked afterwards) so that the D / 32 loads of a block are all
// in flight at once.  Rows >= bar are appended to (rs, ri) through *cnt; the list cannot exceed k * tile_rows entries.
template <int D, int NWAVES, typename WinAt>
__device__ __forceinline__ void tile_rescore_f16(const f16x8 (&qf)[D / 32], const _Float16* __restrict__ slab, int n_rows, int tile_rows, int k,
                                                 WinAt win_at, float bar, int wave, int lane, int* cnt, float* rs, int* ri) {
  constexpr int kKs = D / 32;
  const int lr = lane & 15, kq = lane >> 4;
  const int halves = tile_rows / 16;          // 16-row MFMA blocks per tile: 1, 2 or 4
  const int units = k * halves;               // <= 128
  for (int u = wave; u < units; u += NWAVES) {
    const int j = u / halves, hb = u % halves;
    const int w = win_at(j);
    const int first = (w < 0) ? 0 : (w / tile_rows) * tile_rows + hb * 16;
    const int row = first + lr;
    const _Float16* arow = slab + (size_t)(row < n_rows ? row : n_rows - 1) * D + kq * 8;
    f16x8 af[kKs];
#pragma unroll
    for (int ks = 0; ks < kKs; ++ks) af[ks] = *reinterpret_cast<const f16x8*>(arow + ks * 32);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < kKs; ++ks) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[ks], qf[ks], acc, 0, 0, 0);
    // lane (n = lr, kq) holds rows 4 kq + i of column n; column 0 is as good as any
    if (lr == 0 && w >= 0) {
#pragma unroll
      for (int ii = 0; ii < 4; ++ii) {
        const int rr = first + 4 * kq + ii;
        if (rr < n_rows && acc[ii] >= bar) {
          const int p = atomicAdd(cnt, 1);
          rs[p] = acc[ii];
          ri[p] = rr;
        }
      }
    }
  }
}

// ---- the exactness certificate ---------------------------------------------------------------------------------------------------
// The store over-fetches k' candidates per query from the fp16 / int8 slab and re-ranks them by their fp32 scores against the fp32
// shadow.  That result IS the fp32 top-k of ALL rows whenever no un-fetched row can reach it:
//     every un-fetched row j has   slab_score(j) <= t            (t = the k'-th slab score: the scan is exact on its
//                                                                 own scores; + 2e-5 |t| for the last-bit difference
//                                                                 between the scan's and the tile refine's MFMA shape)
//     and                          |slab_score(j) - s32(j)| <= eps_q
// so s32(j) <= t + eps_q =: bound, and the re-ranked list is exact iff its k-th fp32 score is > bound.
// eps_q is a worst-case (Cauchy-Schwarz) bound, per query, from quantities that are MEASURED, not assumed:
//     slab_score - s32 = <q16 - q, c^_j> + <q, c^_j - c_j>  (+ accumulation error)      c^_j = the row as the slab holds it
//     |.| <= dq (1 + E) + |q| E + arith
//     dq    = |q16 - q|_2 computed from the very two query blocks the scan and the re-rank read
//             (+ sqrt(pdim) max|q16| / 65024 for int8 slabs: the scan moves the query to 16-bit fixed point, scan_i8.hip)
//     E     = max over the shard's rows of |c^_j - c_j|_2, tracked by slab_store_row (slab_row.h) in a device scalar
//     arith = (1.5 pdim + 8) 2^-23: pdim exact products summed in fp32 in any order with truncation (<= pdim 2^-23
//             sum |a_i b_i| <= pdim 2^-23) plus the fp32 FMA chain of the re-rank (<= dim 2^-24 + the butterfly)
//
// cert_query_partials: called by the first 256 threads (t = 0..255) of a workgroup: |q16 - q|^2, |q|^2 and max |q16| over the
// padded row (elements past dim: q = 0), one partial per wave into red[wave].  The caller synchronises before cert_query_eps.
__device__ __forceinline__ void cert_query_partials(const float* __restrict__ a, const _Float16* __restrict__ a16, int dim, int pdim, int t,
                                                    float (*red)[3]) {
  const int lane = t & 63, wave = t >> 6;
  float d2 = 0.f, n2 = 0.f, am = 0.f;
  for (int e = t; e < pdim; e += 256) {
    const float x = e < dim ? a[e] : 0.f, h = (float)a16[e];
    d2 = fmaf(h - x, h - x, d2);
    n2 = fmaf(x, x, n2);
    am = fmaxf(am, fabsf(h));
  }
  d2 = wsum(d2); n2 = wsum(n2); am = wmax(am);
  if (lane == 0) { red[wave][0] = d2; red[wave][1] = n2; red[wave][2] = am; }
}

// eps_q = dq (1 + E) + |q| E + arith from the four partials (dq: + the 16-bit fixed-point query term on int8 slabs)
__device__ __forceinline__ float cert_query_eps(const float (*red)[3], int pdim, int is_i8, float err_rows, float err_arith) {
  const float dd = red[0][0] + red[1][0] + red[2][0] + red[3][0];
  const float nn = red[0][1] + red[1][1] + red[2][1] + red[3][1];
  const float mx = fmaxf(fmaxf(red[0][2], red[1][2]), fmaxf(red[2][2], red[3][2]));
  float dq = sqrtf(dd) * 1.0001f;
  if (is_i8) dq += sqrtf((float)pdim) * mx * (1.0001f / 65024.0f);
  return dq * (1.0f + err_rows) * 1.0001f + sqrtf(nn) * err_rows * 1.0002f + err_arith;
}

// what no un-fetched row's fp32 score can exceed, t = the lowest slab score of a full candidate list
__device__ __forceinline__ float cert_bound(float t, float eps) { return t + eps + 2e-5f * fabsf(t); }

// One thread: the verdict over a query's k_in slab candidates (id_at(c), slab_at(c)); kth = the k_out-th fp32 score of the re-rank
// (-inf with fewer than k_out candidates: never passes the bound).  0 = the re-ranked list is proven, 1 = not proven.
// Proof without a bound only when the list holds every row of the shard (valid in-shard candidates >= n_rows); a -1 slot on a
// larger shard, or an id outside [id_base, id_base + n_rows), proves nothing.
template <typename IdAt, typename SlabAt>
__device__ __forceinline__ int cert_verdict(int k_in, IdAt id_at, SlabAt slab_at, int64_t id_base, int64_t n_rows, float kth, float eps) {
  int valid = 0, outside = 0;
  float tmin = __builtin_huge_valf();
  for (int c = 0; c < k_in; ++c) {
    const int64_t id = id_at(c);
    if (id < 0) continue;
    if (id - id_base >= 0 && id - id_base < n_rows) { ++valid; tmin = fminf(tmin, slab_at(c)); }
    else ++outside;
  }
  if (outside == 0 && (int64_t)valid >= n_rows) return 0;   // every row of the shard is in the list
  if (outside == 0 && valid == k_in) return (kth > cert_bound(tmin, eps)) ? 0 : 1;
  return 1;
}

// One thread per query: the status and the escalation workspace's per-query threshold and counter.  An uncertified query is
// escalated by listing every row whose slab score is >= kth - eps_q: a row of the true fp32 top-k cannot score lower.
__device__ __forceinline__ void cert_publish(int q, int st, float kth, float eps, int* __restrict__ status, float* __restrict__ ws_thr,
                                             int* __restrict__ ws_cnt, int* __restrict__ ws_done) {
  status[q] = st;
  ws_thr[q] = kth - eps;
  ws_cnt[q] = 0;
  if (q == 0) *ws_done = 0;       // the escalation kernel's "blocks through" counter
}

// ---- merge: m = nlists * k_in sorted-list entries of a query, TH threads ------------------------------------------------------------
// Which entry a thread visits in pass p.  Plain striding (entry = tid + TH p) gives thread t the SAME slot t % k_in of
// every list whenever k_in divides TH (a few slots when it shares a factor) -- and the lists arrive sorted, so a few
// threads own every list's best entries, the k-th largest "bucket maximum" is then the maximum of a bucket of
// 4th-best entries, far too low a bar, the LDS list overflows and the exact-but-slow fallback runs (k = 32 over 512
// lists: 210-250 us instead of ~ 15).  So a pass covers WHOLE lists (C = the largest multiple of k_in <= TH entries;
// threads >= C sit the pass out) and the slot is rotated by the pass number -- a bijection inside each list: every
// thread meets all slots in turn.  A pass advances a thread by C / k_in whole lists, so (list, slot) need ONE division per
// thread, not two per entry (k_in is a run-time value: at 123 slots per list the divisions were most of a 31 488-candidate
// merge, 53 us).
template <int TH>
__host__ __device__ inline int merge_entries_per_pass(int k_in) { return (k_in > 1 && k_in <= TH) ? (TH / k_in) * k_in : TH; }

template <int TH>
struct MergePasses {
  int tid, k_in, nlists, m;
  bool rotate;
  int C, lpp, list0, slot0, n_pass;   // entries per pass, lists per pass, this thread's first list and slot
  __device__ __forceinline__ MergePasses(int tid_, int nlists_, int k_in_) : tid(tid_), k_in(k_in_), nlists(nlists_), m(nlists_ * k_in_) {
    rotate = k_in > 1 && k_in <= TH;
    C = merge_entries_per_pass<TH>(k_in);
    lpp = rotate ? TH / k_in : 0;
    list0 = rotate ? tid / k_in : 0;
    slot0 = rotate ? tid - list0 * k_in : 0;
    n_pass = (m + C - 1) / C;
  }
  // slot = (slot0 + p) % k_in, kept by the caller (next_slot); -1 = no entry
  __device__ __forceinline__ int entry_at(int p, int slot) const {
    if (tid >= C) return -1;
    const int e = rotate ? (list0 + p * lpp) * k_in + slot : p * TH + tid;
    return e < m && (!rotate || list0 + p * lpp < nlists) ? e : -1;
  }
  __device__ __forceinline__ int next_slot(int slot) const { return (slot + 1 == k_in) ? 0 : slot + 1; }
};

// A thread's <= REGE entries of a contiguous [nlists, k_in] block into registers, all loads in flight at once (needs
// n_pass <= REGE); returns the thread's best score (its "bucket maximum").
template <int REGE, int TH, typename IdT>
__device__ __forceinline__ float merge_load_entries(const MergePasses<TH>& g, const float* __restrict__ qs, const IdT* __restrict__ qi,
                                                    float (&cs)[REGE], IdT (&ci)[REGE]) {
  int sl = g.slot0;
#pragma unroll
  for (int u = 0; u < REGE; ++u) {
    const int e = (u < g.n_pass) ? g.entry_at(u, sl) : -1;
    sl = g.next_slot(sl);
    cs[u] = e >= 0 ? qs[e] : kNegInf;
    ci[u] = e >= 0 ? qi[e] : (IdT)-1;
  }
  float best = kNegInf;
#pragma unroll
  for (int u = 0; u < REGE; ++u) best = fmaxf(best, (ci[u] >= 0) ? cs[u] : kNegInf);
  return best;
}

// entry (s, id) joins the LDS list when it reaches tau; *cnt keeps counting past cap (the caller sees the overflow)
template <typename IdT>
__device__ __forceinline__ void merge_append(float s, IdT id, float tau, int* cnt, int cap, float* ls, IdT* li) {
  if (id >= 0 && s >= tau) {
    const int p = atomicAdd(cnt, 1);
    if (p < cap) { ls[p] = s; li[p] = id; }
  }
}

// The 64 largest of the NW * 64 bucket maxima of a workgroup, sorted descending, identical in every wave.  `sorted` is the wave's
// own 64 maxima sorted (wave_sort_desc); "top 64 of two sorted lists" = elementwise max of one list with the other reversed (a
// bitonic sequence) + wave_clean_desc.  NW -> 4 lists through LDS (two buffers), the last four in registers.
// The k-th of them is a lower bound tau on the true k-th best entry (those k maxima are k distinct entries), and the selection
// ">= tau, then rank" is exact for any such bound.
template <int NW>
__device__ __forceinline__ float top64_of_sorted(float (*buf)[NW][64], float sorted, int wave, int lane) {
  buf[0][wave][lane] = sorted;
  __syncthreads();
  int src = 0;
#pragma unroll
  for (int n = NW; n > 4; n >>= 1) {
    if (wave < n / 2) buf[src ^ 1][wave][lane] = wave_clean_desc(fmaxf(buf[src][2 * wave][lane], buf[src][2 * wave + 1][63 - lane]), lane);
    __syncthreads();
    src ^= 1;
  }
  float a = fmaxf(buf[src][0][lane], buf[src][1][63 - lane]);
  float b = fmaxf(buf[src][2][lane], buf[src][3][63 - lane]);
  a = wave_clean_desc(a, lane);
  b = wave_clean_desc(b, lane);
  return wave_clean_desc(fmaxf(a, __shfl(b, 63 - lane)), lane);
}

// The overflow fallback (an LDS list longer than its capacity: exact ties by the thousand): k rounds of "best entry strictly
// after the previous winner".  argmax_after: does (s, id) come after the last winner?  argmax_take: does it beat (bs, bi)?
template <typename IdT>
__device__ __forceinline__ bool argmax_after(float s, IdT id, float last_s, IdT last_i) { return (s < last_s) || (s == last_s && id > last_i); }
template <typename IdT>
__device__ __forceinline__ bool argmax_take(float s, IdT id, float bs, IdT bi) { return (id >= 0) && (bi < 0 || before<IdT>(s, id, bs, bi)); }

// every thread's (bs, bi) -> the workgroup's best in every thread; round r alternates between two LDS rows (one barrier per round)
template <int NW, typename IdT>
__device__ __forceinline__ void wg_argmax(float& bs, IdT& bi, int r, float (*arg_s)[NW], IdT (*arg_i)[NW], int wave, int lane) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float os2 = __shfl_xor(bs, off);
    const IdT oi2 = __shfl_xor(bi, off);
    const bool take = argmax_take<IdT>(os2, oi2, bs, bi);
    bs = take ? os2 : bs;
    bi = take ? oi2 : bi;
  }
  const int pp = r & 1;
  if (lane == 0) { arg_s[pp][wave] = bs; arg_i[pp][wave] = bi; }
  __syncthreads();
  bs = arg_s[pp][0];
  bi = arg_i[pp][0];
  constexpr int kUnroll = NW <= 4 ? NW : 1;   // (16 waves' pairs in flight at once would set finish_cert_kernel's register peak)
#pragma unroll kUnroll
  for (int w = 1; w < NW; ++w) {
    const float os2 = arg_s[pp][w];
    const IdT oi2 = arg_i[pp][w];
    const bool take = argmax_take<IdT>(os2, oi2, bs, bi);
    bs = take ? os2 : bs;
    bi = take ? oi2 : bi;
  }
}

}  // namespace
}  // namespace crs
