// join.hip -- thresholded self-join of the slab (gfx950): crs_pairs_above_f16 and crs_pairs_verify_f32.
//
// Near-duplicate detection: every pair of rows i < j whose cosine is at least t, each pair once, in two stages.
//
//   Stage 1, pairs_above_kernel: an N x N fp16 GEMM of the slab with itself whose epilogue COMPARES instead of storing.  One
//   512-thread workgroup owns a 256 x 256 tile of the score matrix (rows of range A x rows of range B); eight waves as 2 (A rows)
//   x 4 (B rows), wave tile 128 x 64 = 8 x 4 accumulator tiles of v_mfma_f32_16x16x32_f16 -- the tile, the wave layout and the
//   LDS image of enc_gemm8.hip (two k-tile buffers of four 16 KB half tiles, 128-byte rows, 16-byte chunks XOR-swizzled by
//   (row >> 1) & 7 on the SOURCE address, filled by lds_dma16), so the staged bytes per flop are that kernel's: a k-tile stages
//   2 x 256 x 64 x 2 = 64 KB for 2 x 256 x 256 x 64 flops = 128 flops per staged byte.  The k loop is the plain two-buffer form:
//   ONE barrier per k-tile; behind it every wave issues its share of k-tile t + 1 into the other buffer, then multiplies
//   k-tile t.  Hazards:
//     RAW  every wave waits vmcnt(0) for its own transfers of k-tile t before the barrier at the top of step t; the reads of
//          k-tile t come after that barrier;
//     WAR  the buffer that receives k-tile t + 1 was last read by the fragment reads of step t - 1, which every wave retires
//          (lgkmcnt(0), in the same wait) before it reaches the barrier at the top of step t; the transfers are issued after it.
//   Rows at or past the end of a range are never loaded: the source row of a transfer is clamped to the last row of its range
//   (the clamped copies are masked in the epilogue), so nothing outside [0, n_rows) x pdim is read.  pdim padding is the zeros
//   the slab holds.
//   Tile pairs wholly on or below the diagonal (no i < j inside) leave at the top.  blockIdx.x walks B tiles in panels of 8:
//   inside a panel the B tile is the fastest index, so the eight workgroups that start together (one per XCD under round-robin
//   placement -- speed only) share ONE A tile, and workgroups b, b + 8, b + 16 ... -- the ones that share an XCD -- keep ONE B
//   tile hot in that XCD's L2 while the A tiles pass over it.
//   Epilogue: each lane compares its 128 accumulators with thr under the masks (i in A, j in B, i < j), the workgroup counts its
//   hits with one LDS add per lane that has any, and ONLY a workgroup that has hits issues one returned device-scope atomicAdd
//   (lane 0) that reserves its slots; the lanes then write their pairs (one 16-byte store) and scores behind it, none past cap.
//   The counter receives every hit whether or not it fitted: count > cap is the overflow signal.
//
//   Stage 2, pairs_verify_kernel: a quarter wave per candidate pair; lane l of the 16 sums coordinates l, l + 16, ... of the two
//   fp32 shadow rows with one fmaf chain, then an xor butterfly over the 16 lanes (token_match.hip's norms): a fixed order that
//   depends on nothing but d, so a pair's sim32 is bitwise independent of the launch it shares.  Pairs with sim32 >= thr are
//   compacted through a counter, one returned atomicAdd per wave that has any.  Rows outside [0, n_rows) are never dereferenced.
//
// No scratch, no workgroup waits for another, no host synchronisation.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "lds_dma.h"
#include "scan.h"

namespace crs {
namespace {

typedef _Float16 jn_f16x8 __attribute__((ext_vector_type(8)));
typedef float jn_f32x4 __attribute__((ext_vector_type(4)));
typedef long long jn_i64x2 __attribute__((ext_vector_type(2)));

constexpr int kJT = CRS_PAIRS_TILE;            // tile edge: rows of A x rows of B per workgroup
constexpr int kJK = 64;                        // k-tile
constexpr int kJThreads = 512;
constexpr int kJHalf = 128 * kJK * 2;          // one half tile: 128 rows x 128 bytes = 16 KB
constexpr int kJBuf = 4 * kJHalf;              // one k-tile: [A0 | A1 | B0 | B1] = 64 KB
constexpr int kJLdsMain = 2 * kJBuf;           // 128 KB
constexpr int kJLds = kJLdsMain + 16;          // + the workgroup's hit count and its reserved base
constexpr int kJPanel = 8;                     // B tiles per panel of the walk
static_assert(kJT == 256, "the wave layout below is 2 x 4 waves of 128 x 64");

__global__ __launch_bounds__(kJThreads, 2) void pairs_above_kernel(const _Float16* __restrict__ slab, int pdim, long long a_first,
                                                                   long long a_end, long long b_first, long long b_end, int n_at,
                                                                   int n_bt, float thr, long long* __restrict__ pairs_out,
                                                                   float* __restrict__ scores_out, long long cap,
                                                                   unsigned long long* __restrict__ counter) {
  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  extern __shared__ __attribute__((aligned(16))) char smj[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;

  // ---- the walk: panels of kJPanel B tiles; inside a panel the B tile is the fastest index
  const int id = (int)blockIdx.x;
  const int per_panel = kJPanel * n_at;
  const int panel = id / per_panel, rem = id - panel * per_panel;
  const int pb = n_bt - panel * kJPanel < kJPanel ? n_bt - panel * kJPanel : kJPanel;   // B tiles of this panel
  const int at = rem / pb, bt = panel * kJPanel + rem % pb;
  if (at >= n_at) return;                                  // (the last panel is narrower: its spare ids have no tile)
  const long long a0 = a_first + (long long)at * kJT, b0 = b_first + (long long)bt * kJT;
  const long long j_last = (b0 + kJT < b_end ? b0 + kJT : b_end) - 1;
  if (a0 >= j_last) return;                                // no i < j in this tile pair: on or below the diagonal

  unsigned* cnt = reinterpret_cast<unsigned*>(smj + kJLdsMain);
  if (tid == 0) cnt[0] = 0u;                               // (the barriers of the k loop order this before the epilogue's adds)

  // ---- transfers.  LDS position P = j * 512 + tid (16-byte units) of a half tile = (row P >> 3, slot P & 7) receives source
  // chunk slot ^ ((row >> 1) & 7) of that row; the row is clamped to the last row of its range.
  unsigned voff[4][2];
#pragma unroll
  for (int half = 0; half < 4; ++half) {
    const long long t0 = (half < 2 ? a0 : b0), last = (half < 2 ? a_end : b_end) - 1 - t0;   // last >= 0: the tile has a row
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int p = j * kJThreads + tid, row = p >> 3, slot = p & 7;
      long long r = (half & 1) * 128 + row;
      r = r > last ? last : r;
      voff[half][j] = (unsigned)r * (unsigned)pdim * 2u + (unsigned)((slot ^ ((row >> 1) & 7)) << 4);
    }
  }
  const _Float16* a_src = uniform_ptr(slab + (size_t)a0 * pdim);
  const _Float16* b_src = uniform_ptr(slab + (size_t)b0 * pdim);
  const unsigned lds0 = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_ptr_t)smj + (unsigned)wave * 1024u);
  auto issue = [&](int buf, int kt) {
#pragma unroll
    for (int half = 0; half < 4; ++half) {
      const _Float16* base = (half < 2 ? a_src : b_src) + (size_t)kt * kJK;
      const unsigned d = lds0 + (unsigned)(buf * kJBuf + half * kJHalf);
      lds_dma16(d, voff[half][0], base);
      lds_dma16(d + 8192u, voff[half][1], base);
    }
  };

  // ---- fragment addresses: lane (r = lane & 15, h = lane >> 4) reads row r of a 16-row tile, 16-byte chunk 4 s + h
  const int r = lane & 15, h = lane >> 4;
  const int sw = (r >> 1) & 7;
  const int lo0 = r * 128 + ((h ^ sw) << 4);            // k sub-step 0
  const int lo1 = r * 128 + (((4 + h) ^ sw) << 4);      // k sub-step 1
  const char* a_base = smj + wm * kJHalf;                                           // this wave's 128 A rows
  const char* b_base = smj + (2 + (wn >> 1)) * kJHalf + (wn & 1) * 64 * 128;        // this wave's 64 B rows

  jn_f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = jn_f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = pdim / kJK;
  issue(0, 0);
  for (int t = 0; t < nk; ++t) {
    const int b = t & 1;
    // this wave's transfers of k-tile t have landed, and its fragment reads of step t - 1 are retired (not merely issued)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();                                      // ... everybody's: buffer b is whole, buffer b ^ 1 is no longer read
    if (t + 1 < nk) issue(b ^ 1, t + 1);
    const char* ab = a_base + b * kJBuf;
    const char* bb = b_base + b * kJBuf;
    jn_f16x8 bf[4][2];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf[j][0] = *reinterpret_cast<const jn_f16x8*>(bb + j * 2048 + lo0);
      bf[j][1] = *reinterpret_cast<const jn_f16x8*>(bb + j * 2048 + lo1);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g) {                         // A rows 0-63, then 64-127 of the wave tile
      jn_f16x8 af[4][2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i][0] = *reinterpret_cast<const jn_f16x8*>(ab + (4 * g + i) * 2048 + lo0);
        af[i][1] = *reinterpret_cast<const jn_f16x8*>(ab + (4 * g + i) * 2048 + lo1);
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[4 * g + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i][s], bf[j][s], acc[4 * g + i][j], 0, 0, 0);
    }
  }

  // ---- epilogue.  Accumulator tile (i, j), register e of lane (c = lane & 15, q = lane >> 4) is the score of
  // A row a0 + wm 128 + i 16 + 4 q + e and B row b0 + wn 64 + j 16 + c.
  const long long ra0 = a0 + wm * 128 + 4 * (lane >> 4), rb0 = b0 + wn * 64 + (lane & 15);
  int n = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long ra = ra0 + i * 16 + e, rb = rb0 + j * 16;
        n += (ra < a_end && rb < b_end && ra < rb && acc[i][j][e] >= thr) ? 1 : 0;
      }
  unsigned at_off = 0u;
  if (n) at_off = atomicAdd(&cnt[0], (unsigned)n);        // LDS
  __syncthreads();
  const unsigned total = cnt[0];
  if (total == 0u) return;                                 // (workgroup-uniform)
  if (tid == 0) {
    const unsigned long long base = atomicAdd(counter, (unsigned long long)total);   // the ONE global atomic of a workgroup with hits
    cnt[2] = (unsigned)base;
    cnt[3] = (unsigned)(base >> 32);
  }
  __syncthreads();
  if (n == 0) return;
  long long slot = (long long)(((unsigned long long)cnt[3] << 32) | cnt[2]) + at_off;
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long long ra = ra0 + i * 16 + e, rb = rb0 + j * 16;
        if (ra < a_end && rb < b_end && ra < rb && acc[i][j][e] >= thr) {
          if (slot < cap) {
            *reinterpret_cast<jn_i64x2*>(pairs_out + 2 * slot) = jn_i64x2{ra, rb};
            scores_out[slot] = acc[i][j][e];
          }
          ++slot;
        }
      }
}

constexpr int kVThreads = 256;

__global__ __launch_bounds__(kVThreads) void pairs_verify_kernel(const long long* __restrict__ pairs, long long m,
                                                                 const float* __restrict__ shadow, long long n_rows, int d, float thr,
                                                                 long long* __restrict__ rows_a, long long* __restrict__ rows_b,
                                                                 float* __restrict__ sims, unsigned long long* __restrict__ counter) {
  const int lane = threadIdx.x & 63, l16 = lane & 15;
  const long long p = ((long long)blockIdx.x * kVThreads + threadIdx.x) >> 4;
  long long ra = -1, rb = -1;
  if (p < m) {
    const jn_i64x2 ab = *reinterpret_cast<const jn_i64x2*>(pairs + 2 * p);
    ra = ab[0];
    rb = ab[1];
  }
  const bool valid = ra >= 0 && ra < n_rows && rb >= 0 && rb < n_rows;
  const float* x = shadow + (size_t)(valid ? ra : 0) * d;
  const float* y = shadow + (size_t)(valid ? rb : 0) * d;
  float s = 0.f;
  if (valid)
    for (int k = l16; k < d; k += 16) s = fmaf(x[k], y[k], s);
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const bool hit = valid && l16 == 0 && s >= thr;
  const unsigned long long mask = __ballot(hit);
  if (mask == 0ull) return;                               // (wave-uniform)
  unsigned long long base = 0ull;
  if (lane == 0) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)base), hi = __builtin_amdgcn_readfirstlane((unsigned)(base >> 32));
  if (hit) {
    const long long at = (long long)(((unsigned long long)hi << 32) | lo) + __popcll(mask & ((1ull << lane) - 1ull));
    if (at >= m) return;                                  // (a counter the caller did not zero: never past the m slots)
    rows_a[at] = ra;
    rows_b[at] = rb;
    sims[at] = s;
  }
}

}  // namespace

int pairs_above_launch(const void* slab, int pdim, int64_t a_first, int64_t a_rows, int64_t b_first, int64_t b_rows, float thr,
                       int64_t* pairs_out, float* scores_out, int64_t cap, int64_t* counter, hipStream_t stream) {
  static bool done = false;
  if (!done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&pairs_above_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kJLds);
    if (e != hipSuccess) return (int)e;
    done = true;
  }
  const int n_at = (int)((a_rows + kJT - 1) / kJT), n_bt = (int)((b_rows + kJT - 1) / kJT);
  const int panels = (n_bt + kJPanel - 1) / kJPanel;
  const unsigned grid = (unsigned)panels * (unsigned)kJPanel * (unsigned)n_at;
  hipLaunchKernelGGL(pairs_above_kernel, dim3(grid), dim3(kJThreads), kJLds, stream, static_cast<const _Float16*>(slab), pdim,
                     (long long)a_first, (long long)(a_first + a_rows), (long long)b_first, (long long)(b_first + b_rows), n_at, n_bt, thr,
                     reinterpret_cast<long long*>(pairs_out), scores_out, (long long)cap, reinterpret_cast<unsigned long long*>(counter));
  return (int)hipGetLastError();
}

int pairs_verify_launch(const int64_t* pairs, int64_t m, const float* shadow, int64_t n_rows, int d, float thr, int64_t* rows_a,
                        int64_t* rows_b, float* sims, int64_t* counter, hipStream_t stream) {
  const unsigned grid = (unsigned)((m * 16 + kVThreads - 1) / kVThreads);
  hipLaunchKernelGGL(pairs_verify_kernel, dim3(grid), dim3(kVThreads), 0, stream, reinterpret_cast<const long long*>(pairs), (long long)m,
                     shadow, (long long)n_rows, d, thr, reinterpret_cast<long long*>(rows_a), reinterpret_cast<long long*>(rows_b), sims,
                     reinterpret_cast<unsigned long long*>(counter));
  return (int)hipGetLastError();
}

}  // namespace crs
