// maxsim_scan.hip -- exact late-interaction retrieval: one sweep of the whole token index scores EVERY row by MaxSim on the matrix
// cores and keeps the k best per query inside the sweep (gfx950).  Declared in include/crs_hip.h: crs_maxsim_topk,
// crs_maxsim_topk_workspace_bytes, crs_maxsim_topk_plan_describe.  Plan and limits: maxsim_scan.h.
//
//     score[q][r] = sum_{i < q_len[q]} max_{j in [offsets[r], offsets[r + 1])} <q_i, d_j>       rows with at least one token
//     out[q]      = the k largest (score, r), score descending, ties by lower row; missing slots (-inf, -1)
//
// The score of a pair is bit for bit crs_maxsim's (maxsim.hip): the same v_mfma_f32_16x16x32_f16 with the k-steps accumulated in
// ascending order from a zero accumulator (a column of D depends on that column of B alone, so which column a token sits in and
// how a document is cut into groups of 16 changes nothing), dead columns set to -inf by a select, a running fmaxf per (row block,
// register) -- exact and order-free -- and that file's step 4 for the sum: (b, e) order within a 16-lane group, then
// ((g0 + g1) + g2) + g3.
//
// Queries in registers, documents through LDS.  A 256-thread workgroup serves 8 queries (blockIdx.y = the group), two per wave:
// the A fragments of both stay in registers for the whole sweep, laid out as maxsim.hip step 1 (2 x 4 row blocks x KS k-steps of
// f16x8: 128 VGPRs at dimp 128; one wave per SIMD owns 512).  Row blocks at or past ceil(q_len / 16) are skipped, wave-uniformly.
//
// Items and windows.  The G workgroups of a query group walk items of 64 consecutive rows (w, w + G, ...).  For an item, lane l of
// every wave holds the clamped end offset of row l (made non-decreasing by a prefix maximum, so a malformed CSR can shorten a row
// but never move a read outside [0, n_tokens)); windows are found by ballots over those lanes, never on the host.  A window is
// the tokens of as many whole consecutive rows as fit in 256 tokens -- one contiguous byte range -- or, when the next row alone
// is longer, the next 256 tokens of that row (its running maxima carry to the next window; its tail then shares a window with the
// rows behind it).  The window is copied by LDS-DMA (lds_dma.h, 16 bytes per lane, per-lane source address) into one of two
// buffers of 256 x dimp fp16.
//
// One barrier per window.  Iteration n: wait for the own transfers of window n, barrier, issue window n + 1 into the other
// buffer, multiply window n.  The other buffer was last read while window n - 1 was multiplied, and every wave finished that
// before it reached this barrier; the transfers of window n + 1 are waited for (each wave its own) before the next barrier, so
// what a wave reads after a barrier has landed.  An item's first window continues the alternation across items, so the argument
// does not restart.
//
// Swizzle.  Sixteen lanes of a ds_read_b128 pass read the same 16-byte chunk column of 16 consecutive tokens; a token row is
// 64 KS bytes, so unswizzled they would meet in 16 / gcd(16, 4 KS) .. 16 ways.  Chunk c = 4 s + h of LDS row p is stored at
//     dimp 128 (16 chunks):  c ^ (p & 15)               bank group (16 p + c') mod 16 = c ^ (p & 15)
//     dimp  64 ( 8 chunks):  c ^ ((p >> 1) & 7)         bank group 8 (p & 1) + (c ^ ((p >> 1) & 7))
//     dimp  96 (12 chunks):  4 s + (h ^ ((p >> 2) & 3)) bank group 4 ((3 p + s) & 3) + (h ^ ((p >> 2) & 3))
//     dimp  32 ( 4 chunks):  h ^ ((p >> 2) & 3)         bank group 4 (p & 3) + (h ^ ((p >> 2) & 3))
// In every case the bank group is a bijection of p mod 16, and 16 consecutive p cover every residue wherever the group starts:
// no conflicts.  The transfer is linear on the LDS side, so the (self-inverse) swizzle is applied to the source address.
//
// Selection.  Each (wave, query) keeps up to kp (32 or 64) keys, one per lane: ordered score << 32 | ~(row - row_first), 0 = empty,
// and the list's minimum.  A score that does not beat the minimum costs one 64-bit compare; one that does replaces the minimum's
// lane and the minimum is recomputed by a wave reduction.  The row is part of the key, so ties are resolved by row number and the
// list does not depend on the order of arrival.  At the end every list is sorted (wave_sort.h) and written as [G][nq][kp]; merge.hip
// (crs_merge_topk's kernel, nlists = G) finishes under the same order.  No host read of the offsets, no atomics, no scratch.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "lds_dma.h"
#include "maxsim_scan.h"
#include "scan.h"
#include "scan_common.h"
#include "wave_sort.h"

namespace crs {
namespace {

typedef __attribute__((address_space(3))) void* ms_lds_ptr_t;

constexpr int kWin = CRS_MAXSIM_SCAN_WINDOW;
constexpr int kItem = CRS_MAXSIM_SCAN_ITEM_ROWS;
static_assert(kItem == 64, "one lane per row of an item");
static_assert(kWin == kMsScanThreads, "window transfers are counted in passes of one chunk per thread");

struct MsScanArgs {
  const _Float16* q16;          // [nq, lq_max, dimp]
  const int* q_len;             // [nq]
  const char* tok;              // [n_tokens, dimp] fp16
  const long long* offsets;     // [n_rows + 1]
  long long n_tokens, row_first, row_count, items;
  float* part_s;                // [G][nq][kp]
  long long* part_r;
  int nq, lq_max, kp;
};

__device__ __forceinline__ long long uniform_ll(long long v) {
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(unsigned long long)v);
  const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long lane_ll(long long v, int l) { return uniform_ll(__shfl(v, l)); }
__device__ __forceinline__ long long clamp_ll(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the chunk of LDS row p that holds chunk c of the token (and the reverse: the map is its own inverse)
template <int KS>
__device__ __forceinline__ int ms_swz(int c, int p) {
  if (KS == 4) return c ^ (p & 15);
  if (KS == 2) return c ^ ((p >> 1) & 7);
  return c ^ ((p >> 2) & 3);      // dimp 96 and 32: the two low bits, the k-step untouched
}

struct MsWindow {
  long long ws;      // first token
  int n;             // tokens, 1..256
  int row, rb;       // whole rows [row, rb) end in this window (item-relative); rb == row: a 256-token piece of row `row`
};

template <int KS>
__global__ __launch_bounds__(kMsScanThreads) void maxsim_scan_kernel(const MsScanArgs a) {
  constexpr int kDimp = 32 * KS, kCpr = 4 * KS, kRowB = 64 * KS, kBufB = kWin * kRowB;
  extern __shared__ __attribute__((aligned(16))) char ms_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, h = lane >> 4;
  const int G = gridDim.x, w0 = blockIdx.x;
  const float ninf = -__builtin_huge_valf();
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(ms_lds_ptr_t)ms_lds);

  // ---- the wave's two queries and their fragments (maxsim.hip step 1)
  int qi[2], lq[2], nrb[2];
  f16x8 af[2][4][KS];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    qi[j] = (int)blockIdx.y * kMsScanGroupQ + wave * 2 + j;
    int l = qi[j] < a.nq ? a.q_len[qi[j]] : 0;
    l = l < 0 ? 0 : (l > a.lq_max ? a.lq_max : l);
    lq[j] = __builtin_amdgcn_readfirstlane(l);
    nrb[j] = (lq[j] + 15) >> 4;
    const _Float16* qb = a.q16 + (size_t)(qi[j] < a.nq ? qi[j] : 0) * a.lq_max * kDimp + 8 * h;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        af[j][b][s] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (16 * b + r < lq[j]) af[j][b][s] = *reinterpret_cast<const f16x8*>(qb + (size_t)(16 * b + r) * kDimp + 32 * s);
      }
  }

  // ---- the lists: lane < kp holds one key, 0 = empty; the other lanes hold all ones and are never the minimum
  u64 key[2], minkey[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) { key[j] = lane < a.kp ? 0ull : ~0ull; minkey[j] = 0ull; }
  auto offer = [&](u64& mine, u64& least, float score, unsigned rel) {
    const u64 cand = ((u64)ord_of(score) << 32) | (u64)(0xffffffffu - rel);
    if (cand > least) {                                      // (every lane holds the same two values)
      const u64 at = __ballot(mine == least);                // the minimum's lane (the first of several empty ones)
      if (lane == (int)__builtin_ctzll(at)) mine = cand;
      u64 m = mine;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = umin64(m, __shfl_xor(m, o));
      least = m;
    }
  };

  float best[2][4][4];
  int wn = 0;      // windows this workgroup has staged: window n lives in buffer n & 1

  // transfer window w into buffer `buf`: LDS chunk P = pass * 256 + tid <- chunk swz(P % kCpr) of token ws + P / kCpr
  auto issue = [&](const MsWindow& w, int buf) {
    const int chunks = w.n * kCpr;
    const unsigned dst0 = lds_base + (unsigned)(buf * kBufB) + (unsigned)(wave * 1024);
    const char* src0 = a.tok + (size_t)w.ws * kRowB;
    for (int pass = 0; pass * kMsScanThreads < chunks; ++pass) {      // (uniform) at most kCpr passes: P < 256 kCpr, inside the buffer
      int P = pass * kMsScanThreads + tid;
      P = P < chunks ? P : chunks - 1;                                // past the window: its last chunk again, bytes nobody reads unmasked
      const int p = P / kCpr, c = P % kCpr;
      lds_dma16(__builtin_amdgcn_readfirstlane(dst0 + (unsigned)(pass * kMsScanThreads * 16)), src0 + (size_t)(p * kCpr + ms_swz<KS>(c, p)) * 16);
    }
  };

  for (long long item = w0; item < a.items; item += G) {
    const long long r0 = a.row_first + item * kItem;
    const long long left = a.row_first + a.row_count - r0;
    const int nr = left < kItem ? (int)left : kItem;
    // ---- row ends of the item, one per lane, clamped and non-decreasing
    const long long T0 = uniform_ll(clamp_ll(a.offsets[r0], a.n_tokens));
    long long e = clamp_ll(a.offsets[r0 + 1 + (lane < nr ? lane : nr - 1)], a.n_tokens);
    e = e < T0 ? T0 : e;
    int ln = lane;                                                    // compared afresh per item (see lqv below)
    asm volatile("" : "+v"(ln));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long v = __shfl_up(e, o);
      if (ln >= o && v > e) e = v;
    }
    const long long T1 = lane_ll(e, 63);
    if (T1 <= T0) continue;                                           // (uniform) no tokens in the item

    // the window that starts at token `cur` with row `row` the first unfinished one; false when the item is done
    auto next_window = [&](int row, long long cur, MsWindow& w) -> bool {
      row += (int)__popcll(__ballot(lane >= row && lane < nr && e <= cur));      // rows that are empty or done
      if (row >= nr) return false;
      const int fits = (int)__popcll(__ballot(lane >= row && lane < nr && e - cur <= (long long)kWin));
      w.ws = cur;
      w.row = row;
      w.rb = row + fits;
      w.n = fits ? (int)(lane_ll(e, row + fits - 1) - cur) : kWin;
      return true;
    };

    MsWindow w, nx;
    next_window(0, T0, w);                                            // T1 > T0: there is one
    issue(w, wn & 1);
    bool carry = false;                                               // best[] holds the maxima of row w.row's earlier pieces
    for (;;) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // my transfers of window wn have landed
      __syncthreads();                                                // everybody's have; everybody is done with window wn - 1
      const bool more = next_window(w.rb, w.ws + w.n, nx);
      if (more) issue(nx, (wn + 1) & 1);
      const char* buf = ms_lds + (wn & 1) * kBufB;

      // ---- walk the window's rows in order, for both queries
      const int n_rows_here = w.rb > w.row ? w.rb - w.row : 1;
      int t0 = 0;
      for (int i = 0; i < n_rows_here; ++i) {
        const bool piece = w.rb == w.row;
        const int t1 = piece ? kWin : (int)(lane_ll(e, w.row + i) - w.ws);
        if (t1 <= t0) continue;                                       // (uniform) an empty row is never scored
        if (!carry) {
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
              for (int q = 0; q < 4; ++q) best[j][b][q] = ninf;
        }
        // B fragments of the 16 tokens from t: lane (r, h) reads chunks 4 s + h of LDS row t + r.  A row at or past t1 holds the
        // next document or stale bytes; past the buffer the last row is read instead.  The select below masks those columns.
        auto load_b = [&](int t, f16x8 (&f)[KS]) {
          const int p = t + r;
          const int pc = p < kWin ? p : kWin - 1;
          const char* rowp = buf + pc * kRowB;
#pragma unroll
          for (int s = 0; s < KS; ++s) f[s] = *reinterpret_cast<const f16x8*>(rowp + 16 * ms_swz<KS>(4 * s + h, pc));
        };
        f16x8 bf[KS], nxt[KS];
        load_b(t0, bf);
#pragma unroll
        for (int s = 0; s < KS; ++s) nxt[s] = bf[s];
        for (int t = t0; t < t1; t += 16) {
          if (t + 16 < t1) load_b(t + 16, nxt);                       // (uniform) the next group, ahead of this group's MFMAs
          const bool live = t + r < t1;                               // this lane's column
#pragma unroll
          for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (b < nrb[j]) {                                       // (uniform)
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[j][b][s], bf[s], acc, 0, 0, 0);
#pragma unroll
                for (int q = 0; q < 4; ++q) best[j][b][q] = fmaxf(best[j][b][q], live ? acc[q] : ninf);
              }
            }
#pragma unroll
          for (int s = 0; s < KS; ++s) bf[s] = nxt[s];
        }
        carry = piece;
        if (!piece) {
          // ---- maxsim.hip step 4: row maxima over the 16 columns, then the sum in its fixed order
          const unsigned rel = (unsigned)(item * kItem + w.row + i);
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            if (nrb[j] != 0) {                                          // (uniform) no query, or an empty one: nothing is kept
            float sum = 0.f;
            int lqv = lq[j];                                          // compared afresh per row: hoisted out of the sweep the 32
            asm volatile("" : "+v"(lqv));                               // lane masks would live in 64 scalar registers and spill
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (b < nrb[j]) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  float m = best[j][b][q];
#pragma unroll
                  for (int o = 8; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
                  if (16 * b + 4 * h + q < lqv) sum += m;
                }
              }
            }
            const float g1 = __shfl(sum, 16), g2 = __shfl(sum, 32), g3 = __shfl(sum, 48);
            const float score = ((sum + g1) + g2) + g3;
            offer(key[j], minkey[j], __shfl(score, 0), rel);
            }
          }
        }
        t0 = t1;
      }
      ++wn;
      if (!more) break;
      w = nx;
    }
  }

  // ---- every (workgroup, query) leaves its list sorted: [G][nq][kp]
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    u64 k1[1] = {lane < a.kp ? key[j] : 0ull};
    wave_sort_keys<1>(k1, lane);
    if (lane < a.kp && qi[j] < a.nq) {
      const size_t o = ((size_t)w0 * a.nq + qi[j]) * a.kp + lane;
      const bool in = k1[0] != 0;
      a.part_s[o] = in ? float_of_ord((unsigned)(k1[0] >> 32)) : ninf;
      a.part_r[o] = in ? a.row_first + (long long)(0xffffffffu - (unsigned)k1[0]) : -1;
    }
  }
}

__global__ void maxsim_scan_fill_kernel(float* out_s, long long* out_r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { out_s[i] = -__builtin_huge_valf(); out_r[i] = -1; }
}

using MsScanKernel = void (*)(const MsScanArgs);
MsScanKernel scan_kernel(int ksteps) {
  switch (ksteps) {
    case 1: return maxsim_scan_kernel<1>;
    case 2: return maxsim_scan_kernel<2>;
    case 3: return maxsim_scan_kernel<3>;
    default: return maxsim_scan_kernel<4>;
  }
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_maxsim_topk_workspace_bytes(int nq, int k, int64_t row_count, size_t* bytes) {
  crs::MaxsimScanPlan p;
  const char* why = "";
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer (bytes)");
  if (crs::maxsim_scan_make_plan(nq, 1, 32, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  *bytes = crs::maxsim_scan_workspace_bound(nq, k, row_count);
  return CRS_OK;
}

int crs_maxsim_topk_plan_describe(int nq, int lq_max, int dimp, int k, int64_t row_count, char* buf, size_t cap) {
  crs::MaxsimScanPlan p;
  const char* why = "";
  if (!buf || cap == 0) return crs::set_error(CRS_EINVAL, "null buffer");
  if (crs::maxsim_scan_make_plan(nq, lq_max, dimp, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  crs::maxsim_scan_plan_describe(p, buf, cap);
  return CRS_OK;
}

int crs_maxsim_topk(const void* q16_dev, const int32_t* q_len_dev, int nq, int lq_max, const void* tok16_dev,
                    const int64_t* offsets_dev, int64_t n_rows, int64_t n_tokens, int64_t row_first, int64_t row_count, int dimp, int k,
                    void* workspace_dev, size_t workspace_bytes, float* out_scores_dev, int64_t* out_rows_dev, void* stream) {
  using namespace crs;
  MaxsimScanPlan p;
  const char* why = "";
  if (n_rows < 0 || n_tokens < 0) return set_error(CRS_EINVAL, "bad n_rows/n_tokens");
  if (row_first < 0 || row_count < 0 || row_first > n_rows || row_count > n_rows - row_first)
    return set_error(CRS_EINVAL, "row range leaves [0, n_rows)");
  if (maxsim_scan_make_plan(nq, lq_max, dimp, k, row_count, &p, &why)) return set_error(CRS_EINVAL, why);
  if (!q16_dev) return set_error(CRS_EINVAL, "q16_dev is null");
  if (!q_len_dev) return set_error(CRS_EINVAL, "q_len_dev is null");
  if (!offsets_dev) return set_error(CRS_EINVAL, "offsets_dev is null");
  if (n_tokens > 0 && !tok16_dev) return set_error(CRS_EINVAL, "tok16_dev is null");
  if (!workspace_dev) return set_error(CRS_EINVAL, "workspace_dev is null");
  if (!out_scores_dev || !out_rows_dev) return set_error(CRS_EINVAL, "out_scores_dev / out_rows_dev is null");
  if (((uintptr_t)q16_dev | (uintptr_t)tok16_dev | (uintptr_t)workspace_dev) & 15)
    return set_error(CRS_EINVAL, "q16_dev / tok16_dev / workspace_dev must be 16-byte aligned");
  if (workspace_bytes < p.bytes) return set_error(CRS_EINVAL, "workspace too small (crs_maxsim_topk_workspace_bytes)");
  if (nq == 0) return CRS_OK;
  hipStream_t st = (hipStream_t)stream;
  if (row_count == 0) {
    const int n = nq * k;
    hipLaunchKernelGGL(maxsim_scan_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out_scores_dev,
                       reinterpret_cast<long long*>(out_rows_dev), n);
    return launch_status("maxsim_topk (empty range)");
  }
  char* ws = static_cast<char*>(workspace_dev);
  float* part_s = reinterpret_cast<float*>(ws + p.part_s);
  int64_t* part_r = reinterpret_cast<int64_t*>(ws + p.part_r);
  const MsScanArgs a{static_cast<const _Float16*>(q16_dev), q_len_dev, static_cast<const char*>(tok16_dev),
                     reinterpret_cast<const long long*>(offsets_dev), (long long)n_tokens, (long long)row_first, (long long)row_count,
                     (long long)p.items, part_s, reinterpret_cast<long long*>(part_r), nq, lq_max, p.kp};
  const MsScanKernel kern = scan_kernel(p.ksteps);
  if (p.lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes) != hipSuccess)
    return launch_status("maxsim_topk (LDS size)");
  hipLaunchKernelGGL(kern, dim3((unsigned)p.g, (unsigned)p.qgroups), dim3(kMsScanThreads), (size_t)p.lds_bytes, st, a);
  merge_launch_i64(part_s, part_r, p.g, nq, p.kp, k, out_scores_dev, out_rows_dev, st);
  return launch_status("maxsim_topk");
}

}  // extern "C"
