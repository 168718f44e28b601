// maxsim_scan_f8.hip -- exact late-interaction retrieval over an fp8 (e4m3) token index: one sweep scores EVERY row by MaxSim and
// keeps the k best per query inside the sweep (gfx950).  Declared in include/crs_hip.h: crs_maxsim_topk_f8,
// crs_maxsim_topk_f8_workspace_bytes, crs_maxsim_topk_f8_plan_describe.  Plan and limits: maxsim_scan.h.
//
//     score[q][r] = 2^(-2 S) sum_{i < q_len[q]} max_{j in [offsets[r], offsets[r + 1])} <Q_i, D_j>     rows with at least one token
//     out[q]      = the k largest (score, r), score descending, ties by lower row; missing slots (-inf, -1)
//
// The score of a pair is bit for bit crs_maxsim_f8's (maxsim_f8.hip): both take their fragments, their decode and their MFMAs per 16 x 16
// block from maxsim_f8.h (a column of D depends on that column of B alone, so which column a token sits in and how a document is
// cut into groups of 16 changes nothing), mask dead columns to -inf by a select, keep a running fmaxf per (row block, register)
// -- exact and order-free -- and add the row maxima in maxsim.hip's step-4 order.
//
// This is the sweep of maxsim_scan.hip -- items of 64 rows, windows of at most 256 tokens found by ballots over the
// clamped, non-decreasing row ends, LDS-DMA into two buffers, one barrier per window, key lists with the row in the key -- and
// those parts are that file's, line for line.  What the format changes:
//
// Decode.  A group of 16 tokens is read from LDS once (two ds_read_b128 per lane at dimp 128, where fp16 needs four), decoded
// to fp16 once (maxsim_f8.h: exact, and why the fp8 matrix instructions are not used) and multiplied against both queries' row
// blocks.  The queries are decoded once, before the sweep: kMsF8WaveQ = 2 per wave, 8 per workgroup, 237 VGPRs at dimp 128.
//
// Windows of bytes.  A buffer is 256 rows of dimp bytes, 32 KB at dimp 128, two of them 64 KB: two workgroups fit a CU's LDS.
// A row is 2 KS chunks of 16 bytes; the transfer moves chunk P = pass * 256 + tid, at most 2 KS passes a window.
//
// Swizzle.  Sixteen lanes of a ds_read_b128 pass read the same chunk column c of 16 consecutive LDS rows p; a row is 2 KS chunks,
// so unswizzled the 16 reads would fall on 16 / gcd(16, 2 KS) distinct 16-byte bank groups only.  Chunk c of row p is stored at
//     dimp 128 (8 chunks):  c ^ ((p >> 1) & 7)      bank group (8 p + c') mod 16 = 8 (p & 1) + (c ^ ((p >> 1) & 7))
//     dimp  64 (4 chunks):  c ^ ((p >> 2) & 3)      bank group (4 p + c') mod 16 = 4 (p & 3) + (c ^ ((p >> 2) & 3))
//     dimp  96 (6 chunks):  c ^ ((p >> 3) & 1)      bank group (6 p + c') mod 16 = 2 ((3 p + (c >> 1)) & 7) + ((c & 1) ^ ((p >> 3) & 1))
//     dimp  32 (2 chunks):  c ^ ((p >> 3) & 1)      bank group (2 p + c') mod 16 = 2 (p & 7) + (c ^ ((p >> 3) & 1))
// The xor never leaves the row (it touches bits below the chunk count's lowest set bit's span: 8 and 4 chunks are powers of two,
// 6 and 2 chunks flip bit 0 of an even-sized row).  For a fixed c each bank group is a bijection of p mod 16: at 128 and 64 the
// two terms split p mod 16 into its low and high bits; at 96, p -> 3 p + const is a bijection mod 8 and bit 3 of p is the low
// bit; at 32 likewise with p itself.  Sixteen consecutive p cover every residue wherever the group starts: no conflicts.  The
// transfer is linear on the LDS side, so the (self-inverse) swizzle is applied to the source address.
//
// One barrier per window: maxsim_scan.hip's argument, unchanged -- iteration n waits for its own transfers of window n, meets
// the barrier, issues window n + 1 into the buffer last read while window n - 1 was multiplied, multiplies window n.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "lds_dma.h"
#include "maxsim_f8.h"
#include "maxsim_scan.h"
#include "scan.h"
#include "scan_common.h"
#include "wave_sort.h"

namespace crs {
namespace {

typedef __attribute__((address_space(3))) void* ms8_lds_ptr_t;

constexpr int kWin = CRS_MAXSIM_SCAN_WINDOW;
constexpr int kItem = CRS_MAXSIM_SCAN_ITEM_ROWS;
constexpr int kQW = kMsF8WaveQ;
static_assert(kItem == 64, "one lane per row of an item");
static_assert(kWin == kMsScanThreads, "window transfers are counted in passes of one chunk per thread");
static_assert(kMsF8GroupQ == kQW * (kMsScanThreads / 64), "a workgroup's queries are its waves' queries");

struct Ms8ScanArgs {
  const unsigned char* q8;      // [nq, lq_max, dimp]
  const int* q_len;             // [nq]
  const char* tok;              // [n_tokens, dimp] e4m3
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
__device__ __forceinline__ int ms8_swz(int c, int p) {
  if (KS == 4) return c ^ ((p >> 1) & 7);
  if (KS == 2) return c ^ ((p >> 2) & 3);
  return c ^ ((p >> 3) & 1);      // dimp 96 and 32: bit 0 of an even number of chunks
}

struct Ms8Window {
  long long ws;      // first token
  int n;             // tokens, 1..256
  int row, rb;       // whole rows [row, rb) end in this window (item-relative); rb == row: a 256-token piece of row `row`
};

template <int KS>
__global__ __launch_bounds__(kMsScanThreads) void maxsim_scan_f8_kernel(const Ms8ScanArgs a) {
  constexpr int kDimp = 32 * KS, kCpr = 2 * KS, kRowB = kDimp, kBufB = kWin * kRowB;
  extern __shared__ __attribute__((aligned(16))) char ms8_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, h = lane >> 4;
  const int G = gridDim.x, w0 = blockIdx.x;
  const float ninf = -__builtin_huge_valf();
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(ms8_lds_ptr_t)ms8_lds);

  // ---- the wave's queries and their fragments (maxsim_f8.hip step 1)
  int qi[kQW], lq[kQW], nrb[kQW];
  F8Frag16<KS> af[kQW][4];
#pragma unroll
  for (int j = 0; j < kQW; ++j) {
    qi[j] = (int)blockIdx.y * kMsF8GroupQ + wave * kQW + j;
    int l = qi[j] < a.nq ? a.q_len[qi[j]] : 0;
    l = l < 0 ? 0 : (l > a.lq_max ? a.lq_max : l);
    lq[j] = __builtin_amdgcn_readfirstlane(l);
    nrb[j] = (lq[j] + 15) >> 4;
    const unsigned char* qb = a.q8 + (size_t)(qi[j] < a.nq ? qi[j] : 0) * a.lq_max * kDimp;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      f8x32 raw = f8x32{0, 0, 0, 0, 0, 0, 0, 0};
      if (16 * b + r < lq[j]) raw = f8_load_frag<KS>(qb + (size_t)(16 * b + r) * kDimp, h);
      af[j][b] = f8_decode<KS>(raw);
    }
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

  // transfer window w into buffer `buf`: LDS chunk P = pass * 256 + tid <- chunk swz(P % kCpr) of token ws + P / kCpr
  auto issue = [&](const Ms8Window& w, int buf) {
    const int chunks = w.n * kCpr;
    const unsigned dst0 = lds_base + (unsigned)(buf * kBufB) + (unsigned)(wave * 1024);
    const char* src0 = a.tok + (size_t)w.ws * kRowB;
    for (int pass = 0; pass * kMsScanThreads < chunks; ++pass) {      // (uniform) at most kCpr passes: P < 256 kCpr, inside the buffer
      int P = pass * kMsScanThreads + tid;
      P = P < chunks ? P : chunks - 1;                                // past the window: its last chunk again, bytes nobody reads unmasked
      const int p = (int)((unsigned)P / kCpr), c = (int)((unsigned)P % kCpr);
      lds_dma16(__builtin_amdgcn_readfirstlane(dst0 + (unsigned)(pass * kMsScanThreads * 16)), src0 + (size_t)(p * kCpr + ms8_swz<KS>(c, p)) * 16);
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
    auto next_window = [&](int row, long long cur, Ms8Window& w) -> bool {
      row += (int)__popcll(__ballot(lane >= row && lane < nr && e <= cur));      // rows that are empty or done
      if (row >= nr) return false;
      const int fits = (int)__popcll(__ballot(lane >= row && lane < nr && e - cur <= (long long)kWin));
      w.ws = cur;
      w.row = row;
      w.rb = row + fits;
      w.n = fits ? (int)(lane_ll(e, row + fits - 1) - cur) : kWin;
      return true;
    };

    Ms8Window w, nx;
    next_window(0, T0, w);                                            // T1 > T0: there is one
    issue(w, wn & 1);
    bool carry = false;                                               // best[] holds the maxima of row w.row's earlier pieces
    for (;;) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                // my transfers of window wn have landed
      __syncthreads();                                                // everybody's have; everybody is done with window wn - 1
      const bool more = next_window(w.rb, w.ws + w.n, nx);
      if (more) issue(nx, (wn + 1) & 1);
      const char* buf = ms8_lds + (wn & 1) * kBufB;

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
        // B fragment of the 16 tokens from t: lane (r, h) reads chunks h and 4 + h of LDS row t + r.  A row at or past t1 holds the
        // next document or stale bytes; past the buffer the last row is read instead.  The select below masks those columns.
        auto load_b = [&](int t) {
          const int p = t + r;
          const int pc = p < kWin ? p : kWin - 1;
          const char* rowp = buf + pc * kRowB;
          uint4 lo = uint4{0, 0, 0, 0}, hi = uint4{0, 0, 0, 0};
          if (f8_chunk_live<KS>(h)) lo = *reinterpret_cast<const uint4*>(rowp + 16 * ms8_swz<KS>(h, pc));
          if (KS > 2 && f8_chunk_live<KS>(4 + h)) hi = *reinterpret_cast<const uint4*>(rowp + 16 * ms8_swz<KS>(4 + h, pc));
          return f8_frag(lo, hi);
        };
        f8x32 bf = load_b(t0), nxt = bf;
        for (int t = t0; t < t1; t += 16) {
          if (t + 16 < t1) nxt = load_b(t + 16);                      // (uniform) the next group, ahead of this group's MFMAs
          const bool live = t + r < t1;                               // this lane's column
          const F8Frag16<KS> bd = f8_decode<KS>(bf);                  // once per group, for every query and row block
#pragma unroll
          for (int j = 0; j < kQW; ++j)
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (b < nrb[j]) {                                       // (uniform)
                const f8_f32x4 acc = f8_mfma<KS>(af[j][b], bd);
#pragma unroll
                for (int q = 0; q < 4; ++q) best[j][b][q] = fmaxf(best[j][b][q], live ? acc[q] : ninf);
              }
            }
          bf = nxt;
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

__global__ void maxsim_scan_f8_fill_kernel(float* out_s, long long* out_r, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { out_s[i] = -__builtin_huge_valf(); out_r[i] = -1; }
}

using Ms8ScanKernel = void (*)(const Ms8ScanArgs);
Ms8ScanKernel scan_kernel(int ksteps) {
  switch (ksteps) {
    case 1: return maxsim_scan_f8_kernel<1>;
    case 2: return maxsim_scan_f8_kernel<2>;
    case 3: return maxsim_scan_f8_kernel<3>;
    default: return maxsim_scan_f8_kernel<4>;
  }
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_maxsim_topk_f8_workspace_bytes(int nq, int k, int64_t row_count, size_t* bytes) {
  crs::MaxsimScanPlan p;
  const char* why = "";
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer (bytes)");
  if (crs::maxsim_scan_f8_make_plan(nq, 1, 32, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  *bytes = crs::maxsim_scan_f8_workspace_bound(nq, k, row_count);
  return CRS_OK;
}

int crs_maxsim_topk_f8_plan_describe(int nq, int lq_max, int dimp, int k, int64_t row_count, char* buf, size_t cap) {
  crs::MaxsimScanPlan p;
  const char* why = "";
  if (!buf || cap == 0) return crs::set_error(CRS_EINVAL, "null buffer");
  if (crs::maxsim_scan_f8_make_plan(nq, lq_max, dimp, k, row_count, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  crs::maxsim_scan_f8_plan_describe(p, buf, cap);
  return CRS_OK;
}

int crs_maxsim_topk_f8(const void* q8_dev, const int32_t* q_len_dev, int nq, int lq_max, const void* tok8_dev,
                       const int64_t* offsets_dev, int64_t n_rows, int64_t n_tokens, int64_t row_first, int64_t row_count, int dimp, int k,
                       void* workspace_dev, size_t workspace_bytes, float* out_scores_dev, int64_t* out_rows_dev, void* stream) {
  using namespace crs;
  MaxsimScanPlan p;
  const char* why = "";
  if (n_rows < 0 || n_tokens < 0) return set_error(CRS_EINVAL, "bad n_rows/n_tokens");
  if (row_first < 0 || row_count < 0 || row_first > n_rows || row_count > n_rows - row_first)
    return set_error(CRS_EINVAL, "row range leaves [0, n_rows)");
  if (maxsim_scan_f8_make_plan(nq, lq_max, dimp, k, row_count, &p, &why)) return set_error(CRS_EINVAL, why);
  if (!q8_dev) return set_error(CRS_EINVAL, "q8_dev is null");
  if (!q_len_dev) return set_error(CRS_EINVAL, "q_len_dev is null");
  if (!offsets_dev) return set_error(CRS_EINVAL, "offsets_dev is null");
  if (n_tokens > 0 && !tok8_dev) return set_error(CRS_EINVAL, "tok8_dev is null");
  if (!workspace_dev) return set_error(CRS_EINVAL, "workspace_dev is null");
  if (!out_scores_dev || !out_rows_dev) return set_error(CRS_EINVAL, "out_scores_dev / out_rows_dev is null");
  if (((uintptr_t)q8_dev | (uintptr_t)tok8_dev | (uintptr_t)workspace_dev) & 15)
    return set_error(CRS_EINVAL, "q8_dev / tok8_dev / workspace_dev must be 16-byte aligned");
  if (workspace_bytes < p.bytes) return set_error(CRS_EINVAL, "workspace too small (crs_maxsim_topk_f8_workspace_bytes)");
  if (nq == 0) return CRS_OK;
  hipStream_t st = (hipStream_t)stream;
  if (row_count == 0) {
    const int n = nq * k;
    hipLaunchKernelGGL(maxsim_scan_f8_fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, out_scores_dev,
                       reinterpret_cast<long long*>(out_rows_dev), n);
    return launch_status("maxsim_topk_f8 (empty range)");
  }
  char* ws = static_cast<char*>(workspace_dev);
  float* part_s = reinterpret_cast<float*>(ws + p.part_s);
  int64_t* part_r = reinterpret_cast<int64_t*>(ws + p.part_r);
  const Ms8ScanArgs a{static_cast<const unsigned char*>(q8_dev), q_len_dev, static_cast<const char*>(tok8_dev),
                      reinterpret_cast<const long long*>(offsets_dev), (long long)n_tokens, (long long)row_first, (long long)row_count,
                      (long long)p.items, part_s, reinterpret_cast<long long*>(part_r), nq, lq_max, p.kp};
  const Ms8ScanKernel kern = scan_kernel(p.ksteps);
  if (p.lds_bytes > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes) != hipSuccess)
    return launch_status("maxsim_topk_f8 (LDS size)");
  hipLaunchKernelGGL(kern, dim3((unsigned)p.g, (unsigned)p.qgroups), dim3(kMsScanThreads), (size_t)p.lds_bytes, st, a);
  merge_launch_i64(part_s, part_r, p.g, nq, p.kp, k, out_scores_dev, out_rows_dev, st);
  return launch_status("maxsim_topk_f8");
}

}  // extern "C"
