// maxsim_scan_rc.hip -- exact late-interaction retrieval over a 2-bit residual token index: one sweep scores EVERY row by MaxSim
// over the decoded tokens and keeps the k best per query inside the sweep (gfx950).  Declared in include/crs_hip.h:
// crs_maxsim_topk_rc, crs_maxsim_topk_rc_workspace_bytes, crs_maxsim_topk_rc_plan_describe.  Plan and limits: maxsim_scan.h.
//
//     score[q][r] = sum_{i < q_len[q]} max_{j in [offsets[r], offsets[r + 1])} <Q_i, V_j>     V_j the decoded token (maxsim_rc.h)
//     out[q]      = the k largest (score, r), score descending, ties by lower row; missing slots (-inf, -1)
//
// The score of a pair is bit for bit crs_maxsim_rc's (maxsim_rc.hip): both take their fragments, their decode and their MFMAs per
// 16 x 16 block from maxsim_rc.h (a column of D depends on that column of B alone), mask dead columns to -inf by a select, keep a
// running fmaxf per (row block, register) and add the row maxima in maxsim.hip's step-4 order.
//
// This is the sweep of maxsim_scan.hip / maxsim_scan_f8.hip -- items of 64 rows, windows of at most 256 tokens
// found by ballots over the clamped, non-decreasing row ends, two buffers, one barrier per window, key lists with the row in the
// key, partial lists reduced by merge.hip -- and those parts are that file's, line for line.  What the format changes is how a
// window becomes B fragments:
//
// What is staged.  A window buffer holds the window's three plane slices and nothing else: 256 code rows of dimp / 4 bytes (8 KB
// at dimp 128), 256 cids, 256 scales -- 9.5 KB, two buffers 19 KB where the fp8 sweep stages 64 KB.  The code rows, the bulk,
// move by LDS-DMA: 16 bytes a lane where a code row is a multiple of 16 bytes (dimp 64, 128), else 4 bytes a lane, because a
// window then starts at an address that is only 8-byte aligned (dimp 32, 96).  The cids are one more transfer of 4 bytes a lane.
// A window's scales start at an address that is only 2-byte aligned, which no transfer takes: each thread loads its token's scale
// into a register when the window is issued and stores it to the buffer on the far side of its own vmcnt(0), before the barrier
// -- the buffer was last read two windows ago, which every wave left before the previous barrier.
// A code row is read back as the 2 KS consecutive bytes of the lane's coordinates: 64 lanes read 512 consecutive bytes at dimp
// 128, conflict-free without a swizzle.
//
// Gathers.  The centroid rows never pass through LDS.  Lane (r, h) reads the cid of token t + r from the buffer and loads its own
// 8 KS coordinates of that centroid with KS 16-byte global loads, for the group of 16 tokens AFTER the one being multiplied.  A
// slot past the window's tokens holds stale bytes: maxsim_rc.h's check turns any cid outside the table into centroid 0 with scale
// +0 before it is used as an index, and the column is masked to -inf as in every MaxSim kernel here.
//
// Decode.  16 bits of codes and 16 bytes of centroid per lane and k-step become one f16x8 (maxsim_rc.h), once per group, and the
// group is multiplied against both resident queries of the wave (kMsRcWaveQ = 2, 8 per workgroup), as the fp8 sweep does.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "lds_dma.h"
#include "maxsim_rc.h"
#include "maxsim_scan.h"
#include "scan.h"
#include "scan_common.h"
#include "wave_sort.h"

namespace crs {
namespace {

typedef __attribute__((address_space(3))) void* msrc_lds_ptr_t;

constexpr int kWin = CRS_MAXSIM_SCAN_WINDOW;
constexpr int kItem = CRS_MAXSIM_SCAN_ITEM_ROWS;
constexpr int kQW = kMsRcWaveQ;
static_assert(kItem == 64, "one lane per row of an item");
static_assert(kWin == kMsScanThreads, "one cid and one scale per thread and window; code transfers are counted in passes of one chunk per thread");
static_assert(kMsRcGroupQ == kQW * (kMsScanThreads / 64), "a workgroup's queries are its waves' queries");

struct MsRcScanArgs {
  const _Float16* q16;          // [nq, lq_max, dimp]
  const int* q_len;             // [nq]
  RcPlanes tok;
  RcCodec codec;
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

struct MsRcWindow {
  long long ws;      // first token
  int n;             // tokens, 1..256
  int row, rb;       // whole rows [row, rb) end in this window (item-relative); rb == row: a 256-token piece of row `row`
};

template <int KS>
__global__ __launch_bounds__(kMsScanThreads) void maxsim_scan_rc_kernel(const MsRcScanArgs a) {
  constexpr int kDimp = 32 * KS, kRowB = 8 * KS;            // a code row
  constexpr int kChunk = KS % 2 ? 4 : 16;                   // bytes a lane moves per transfer
  constexpr int kCidAt = kWin * kRowB, kScaleAt = kCidAt + kWin * 4, kBufB = kMsRcTokenLdsBytes(kDimp) * kWin;
  static_assert(kScaleAt + kWin * 2 == kBufB, "a buffer is the three slices of a window");
  extern __shared__ __attribute__((aligned(16))) char msrc_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, h = lane >> 4;
  const int G = gridDim.x, w0 = blockIdx.x;
  const float ninf = -__builtin_huge_valf();
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(msrc_lds_ptr_t)msrc_lds);
  RcWeights wt = rc_weights(a.codec.weights);
  wt.lo = __builtin_amdgcn_readfirstlane(wt.lo);
  wt.hi = __builtin_amdgcn_readfirstlane(wt.hi);

  // ---- the wave's queries and their fragments (maxsim_rc.hip step 1)
  int qi[kQW], lq[kQW], nrb[kQW];
  RcFrag<KS> af[kQW][4];
#pragma unroll
  for (int j = 0; j < kQW; ++j) {
    qi[j] = (int)blockIdx.y * kMsRcGroupQ + wave * kQW + j;
    int l = qi[j] < a.nq ? a.q_len[qi[j]] : 0;
    l = l < 0 ? 0 : (l > a.lq_max ? a.lq_max : l);
    lq[j] = __builtin_amdgcn_readfirstlane(l);
    nrb[j] = (lq[j] + 15) >> 4;
    const _Float16* qb = a.q16 + (size_t)(qi[j] < a.nq ? qi[j] : 0) * a.lq_max * kDimp;
#pragma unroll
    for (int b = 0; b < 4; ++b) af[j][b] = 16 * b + r < lq[j] ? rc_load_query<KS>(qb + (size_t)(16 * b + r) * kDimp, h) : rc_zero<KS>();
  }

  // ---- the lists: lane < kp holds one key, 0 = empty; the other lanes hold all ones and are never the minimum
  u64 key[kQW], minkey[kQW];
#pragma unroll
  for (int j = 0; j < kQW; ++j) { key[j] = lane < a.kp ? 0ull : ~0ull; minkey[j] = 0ull; }
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

  float best[kQW][4][4];
  int wn = 0;      // windows this workgroup has staged: window n lives in buffer n & 1
  unsigned short my_scale = 0;   // of token ws + tid of the window in flight, until it is stored to the window's buffer

  // stage window w: the code rows into buffer `buf` by LDS-DMA -- chunk P = pass * 256 + tid of the w.n kRowB bytes from the
  // first token's row on lands at byte P kChunk --, the cids by one more transfer of 4 bytes a lane, the thread's scale into a register
  auto issue = [&](const MsRcWindow& w, int buf) {
    const int chunks = w.n * (kRowB / kChunk);
    const unsigned dst0 = lds_base + (unsigned)(buf * kBufB) + (unsigned)(wave * 64 * kChunk);
    const unsigned char* src0 = a.tok.codes + (size_t)w.ws * kRowB;
    for (int pass = 0; pass * kMsScanThreads < chunks; ++pass) {      // (uniform) chunks <= 256 kRowB / kChunk: inside the code slice
      int P = pass * kMsScanThreads + tid;
      P = P < chunks ? P : chunks - 1;                                // past the window: its last chunk again, bytes nobody reads unmasked
      const unsigned dst = __builtin_amdgcn_readfirstlane(dst0 + (unsigned)(pass * kMsScanThreads * kChunk));
      if (kChunk == 16) lds_dma16(dst, src0 + (size_t)P * 16);
      else lds_dma4(dst, src0 + (size_t)P * 4);
    }
    const long long t = w.ws + (tid < w.n ? tid : w.n - 1);           // inside [ws, ws + n), a sub-range of [0, n_tokens)
    lds_dma4(__builtin_amdgcn_readfirstlane(lds_base + (unsigned)(buf * kBufB + kCidAt + wave * 256)), a.tok.cid + t);
    my_scale = a.tok.scale[t];
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
    auto next_window = [&](int row, long long cur, MsRcWindow& w) -> bool {
      row += (int)__popcll(__ballot(lane >= row && lane < nr && e <= cur));      // rows that are empty or done
      if (row >= nr) return false;
      const int fits = (int)__popcll(__ballot(lane >= row && lane < nr && e - cur <= (long long)kWin));
      w.ws = cur;
      w.row = row;
      w.rb = row + fits;
      w.n = fits ? (int)(lane_ll(e, row + fits - 1) - cur) : kWin;
      return true;
    };

    MsRcWindow w, nx;
    next_window(0, T0, w);                                            // T1 > T0: there is one
    issue(w, wn & 1);
    bool carry = false;                                               // best[] holds the maxima of row w.row's earlier pieces
    for (;;) {
      char* buf = msrc_lds + (wn & 1) * kBufB;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // my transfers and my scale of window wn have landed
      reinterpret_cast<unsigned short*>(buf + kScaleAt)[tid] = my_scale;      // buffer wn & 1 was last read for window wn - 2
      __syncthreads();                                                // everybody's have; everybody is done with window wn - 1
      const bool more = next_window(w.rb, w.ws + w.n, nx);
      if (more) issue(nx, (wn + 1) & 1);

      // ---- walk the window's rows in order, for all the wave's queries
      const int n_rows_here = w.rb > w.row ? w.rb - w.row : 1;
      int t0 = 0;
      for (int i = 0; i < n_rows_here; ++i) {
        const bool piece = w.rb == w.row;
        const int t1 = piece ? kWin : (int)(lane_ll(e, w.row + i) - w.ws);
        if (t1 <= t0) continue;                                       // (uniform) an empty row is never scored
        if (!carry) {
#pragma unroll
          for (int j = 0; j < kQW; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
              for (int q = 0; q < 4; ++q) best[j][b][q] = ninf;
        }
        // lane (r, h)'s share of the 16 tokens from t is slot t + r of the buffer (past the buffer: its last slot).  A slot at or
        // past t1 holds the next document or stale bytes: rc_checked keeps its cid inside the table, the select below masks its
        // column.  Only the gathered centroid words are carried from one group to the next: cid, scale and codes are read again
        // from the buffer when the group is decoded, which keeps six registers out of the loop (256 are all there is at dimp 128).
        auto slot = [&](int t, RcRaw<KS>& raw) {
          const int p = t + r;
          const int pc = p < kWin ? p : kWin - 1;
          int cid = reinterpret_cast<const int*>(buf + kCidAt)[pc];
          unsigned sc = reinterpret_cast<const unsigned short*>(buf + kScaleAt)[pc];
          rc_checked(cid, sc, a.codec.n_centroids);
          raw.scale2 = sc | (sc << 16);
          raw.codes = rc_load_codes<KS>(reinterpret_cast<const unsigned char*>(buf) + pc * kRowB, h);
          return cid;
        };
        RcRaw<KS> bf;
        rc_gather<KS>(bf, a.codec, slot(t0, bf), h);
        for (int t = t0; t < t1; t += 16) {
          const bool live = t + r < t1;                               // this lane's column
          slot(t, bf);
          const RcFrag<KS> bd = rc_decode<KS>(bf, wt);                // once per group, for every query and row block
          if (t + 16 < t1) rc_gather<KS>(bf, a.codec, slot(t + 16, bf), h);        // (uniform) the next group's gathers, ahead of this group's MFMAs,
                                                                                  // into the registers the decode has just read for the last time
#pragma unroll
          for (int j = 0; j < kQW; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (b < nrb[j]) {                                       // (uniform)
                const f8_f32x4 acc = rc_mfma<KS>(af[j][b], bd);
#pragma unroll
                for (int q = 0; q < 4; ++q) best[j][b][q] = fmaxf(best[j][b][q], live ? acc[q] : ninf);
              }
            }
        }
        carry = piece;
        if (!piece) {
          // ---- maxsim.hip step 4: row maxima over the 16 columns, then the sum in its fixed order
          const unsigned rel = (unsigned)(item * kItem + w.row + i);
#pragma unroll
          for (int j = 0; j < kQW; ++j) {
            if (nrb[j] != 0) {                                        // (uniform) no query, or an empty one: nothing is kept
              int lqv = lq[j];                                        // compared afresh per row: hoisted out of the sweep the
              asm volatile("" : "+v"(lqv));                           // lane masks would live in scalar registers and spill
              offer(key[j], minkey[j], f8_row_sum(best[j], nrb[j], lqv, h), rel);
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
  for (int j = 0; j < kQW; ++j) {
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

__global__ void maxsim_scan_rc_fill_kernel(float* out_s, long long* out_r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { out_s[i] = -__builtin_huge_valf(); out_r[i] = -1; }
}

using MsRcScanKernel = void (*)(const MsRcScanArgs);
MsRcScanKernel scan_kernel(int ksteps) {
  switch (ksteps) {
    case 1: return maxsim_scan_rc_kernel<1>;
    case 2: return maxsim_scan_rc_kernel<2>;
    case 3: return maxsim_scan_rc_kernel<3>;
    default: return maxsim_scan_rc_kernel<4>;
  }
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_maxsim_topk_rc_workspace_bytes(int nq, int k, int64_t row_count, size_t* bytes) {
  crs::MaxsimScanPlan p;
  const char* why = "";
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer (bytes)");
  if (crs::maxsim_scan_rc_make_plan(nq, 1, 32, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  *bytes = crs::maxsim_scan_rc_workspace_bound(nq, k, row_count);
  return CRS_OK;
}

int crs_maxsim_topk_rc_plan_describe(int nq, int lq_max, int dimp, int k, int64_t row_count, char* buf, size_t cap) {
  crs::MaxsimScanPlan p;
  const char* why = "";
  if (!buf || cap == 0) return crs::set_error(CRS_EINVAL, "null buffer");
  if (crs::maxsim_scan_rc_make_plan(nq, lq_max, dimp, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  crs::maxsim_scan_rc_plan_describe(p, buf, cap);
  return CRS_OK;
}

int crs_maxsim_topk_rc(const void* q16_dev, const int32_t* q_len_dev, int nq, int lq_max, const int32_t* cid_dev, const void* codes_dev,
                       const void* scale_dev, const void* centroids_dev, int n_centroids, const float* weights_dev,
                       const int64_t* offsets_dev, int64_t n_rows, int64_t n_tokens, int64_t row_first, int64_t row_count, int dimp, int k,
                       void* workspace_dev, size_t workspace_bytes, float* out_scores_dev, int64_t* out_rows_dev, void* stream) {
  using namespace crs;
  MaxsimScanPlan p;
  const char* why = "";
  if (n_rows < 0 || n_tokens < 0) return set_error(CRS_EINVAL, "bad n_rows/n_tokens");
  if (row_first < 0 || row_count < 0 || row_first > n_rows || row_count > n_rows - row_first)
    return set_error(CRS_EINVAL, "row range leaves [0, n_rows)");
  if (maxsim_scan_rc_make_plan(nq, lq_max, dimp, k, row_count, &p, &why)) return set_error(CRS_EINVAL, why);
  if (n_centroids < CRS_RC_MIN_CENTROIDS || n_centroids > CRS_RC_MAX_CENTROIDS)
    return set_error(CRS_EINVAL, "n_centroids must be in CRS_RC_MIN_CENTROIDS..CRS_RC_MAX_CENTROIDS");
  if (!q16_dev) return set_error(CRS_EINVAL, "q16_dev is null");
  if (!q_len_dev) return set_error(CRS_EINVAL, "q_len_dev is null");
  if (!centroids_dev || !weights_dev) return set_error(CRS_EINVAL, "centroids_dev / weights_dev is null");
  if (!offsets_dev) return set_error(CRS_EINVAL, "offsets_dev is null");
  if (n_tokens > 0 && (!cid_dev || !codes_dev || !scale_dev)) return set_error(CRS_EINVAL, "cid_dev / codes_dev / scale_dev is null");
  if (!workspace_dev) return set_error(CRS_EINVAL, "workspace_dev is null");
  if (!out_scores_dev || !out_rows_dev) return set_error(CRS_EINVAL, "out_scores_dev / out_rows_dev is null");
  if (((uintptr_t)q16_dev | (uintptr_t)codes_dev | (uintptr_t)centroids_dev | (uintptr_t)workspace_dev) & 15)
    return set_error(CRS_EINVAL, "q16_dev / codes_dev / centroids_dev / workspace_dev must be 16-byte aligned");
  if (workspace_bytes < p.bytes) return set_error(CRS_EINVAL, "workspace too small (crs_maxsim_topk_rc_workspace_bytes)");
  if (nq == 0) return CRS_OK;
  hipStream_t st = (hipStream_t)stream;
  if (row_count == 0) {
    const int n = nq * k;
    hipLaunchKernelGGL(maxsim_scan_rc_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out_scores_dev,
                       reinterpret_cast<long long*>(out_rows_dev), n);
    return launch_status("maxsim_topk_rc (empty range)");
  }
  char* ws = static_cast<char*>(workspace_dev);
  float* part_s = reinterpret_cast<float*>(ws + p.part_s);
  int64_t* part_r = reinterpret_cast<int64_t*>(ws + p.part_r);
  const MsRcScanArgs a{static_cast<const _Float16*>(q16_dev), q_len_dev,
                       RcPlanes{cid_dev, static_cast<const unsigned char*>(codes_dev), static_cast<const unsigned short*>(scale_dev)},
                       RcCodec{static_cast<const _Float16*>(centroids_dev), weights_dev, n_centroids},
                       reinterpret_cast<const long long*>(offsets_dev), (long long)n_tokens, (long long)row_first, (long long)row_count,
                       (long long)p.items, part_s, reinterpret_cast<long long*>(part_r), nq, lq_max, p.kp};
  hipLaunchKernelGGL(scan_kernel(p.ksteps), dim3((unsigned)p.g, (unsigned)p.qgroups), dim3(kMsScanThreads), (size_t)p.lds_bytes, st, a);
  merge_launch_i64(part_s, part_r, p.g, nq, p.kp, k, out_scores_dev, out_rows_dev, st);
  return launch_status("maxsim_topk_rc");
}

}  // extern "C"
