// enc_gemm.hip -- K2/K4/K5/K6: fp16 MFMA GEMM with fused epilogues for the encoder (gfx950).
//
//   C[M, N] = epilogue( A[M, K] x W[N, K]^T + bias[N] )         (torch.nn.Linear layout)
//
// 128 x 128 output tile per 256-thread workgroup (4 wave64 as 2 x 2, 64 x 64 each, as 2 x 2
// v_mfma_f32_32x32x16_f16 tiles), K stepped 64 at a time through a double-buffered LDS stage.
// Both operands are K-contiguous, so a tile row is one 128-byte line: global loads are
// 16 bytes/lane, 8 lanes per row, and the LDS image is XOR-swizzled by row
// (chunk ^= (row >> 1) & 7) so every ds_read_b128 fragment read is bank-conflict free.
// Staging is LDS-DMA (global_load_lds_dwordx4): the next K-tile is fetched into the other buffer
// under the current tile's MFMAs, one vmcnt(0) + barrier per K-tile; the epilogue goes through
// LDS so that global loads / stores are 16-byte coalesced rows.
// Epilogues (fp32 accumulators -> ...):
//   0  + bias                      -> fp16      (QKV projection)
//   1  + bias, erf-GELU            -> fp16      (FFN up)
//   2  + bias + residual (fp32)    -> fp32      (attention out / FFN down; LayerNorm follows)
//   4  + bias, silu(gate) * up     -> fp16 [M, N / 2]   (gated FFN up: W rows interleaved [16 gate | 16 up], crs_encoder.h)
//   5  + bias, gelu(gate) * up     -> fp16 [M, N / 2]   (mode 4's epilogue with the erf GELU on the activated half: GeGLU)
// MFMA-bound for index-build batches (thousands of tokens); launch-bound for a single short query.

#include "enc.h"
#include "enc_gelu.h"

#include <stdlib.h>

namespace crs {
namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int BM = forms::kTiledM, BN = forms::kTiledN, BK = 64;
constexpr int kThreads = forms::kTiledThreads;
constexpr int kStageBytes = (BM + BN) * BK * 2;  // 32 KiB

__device__ __forceinline__ int lds_off(int row, int chunk) {  // 128-byte rows, 8 x 16-byte chunks
  return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

template <int MODE>
__global__ __launch_bounds__(kThreads, 2) void gemm_f16_kernel(const _Float16* __restrict__ A,
                                                              const _Float16* __restrict__ W,
                                                              const float* __restrict__ bias,
                                                              const float* __restrict__ residual,
                                                              void* __restrict__ out, int M, int N, int K) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kStageBytes];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  // 1-D grid; the column blocks of one row block are neighbours in one XCD's range (enc.h) and share the A panel there
  const int ncb = (N + BN - 1) / BN;
  const int wid = xcd_chunked_id((int)blockIdx.x, (int)gridDim.x);
  const int m0 = (wid / ncb) * BM, n0 = (wid % ncb) * BN;

  // staging by LDS-DMA: chunk P = j*256 + tid of a [128 rows][8 chunks] panel lands at LDS offset P*16
  // (linear); the bank swizzle chunk ^= (row >> 1) & 7 is applied to the SOURCE column instead.
  // Rows past M / N are clamped to the last valid row (their products are never stored).
  const _Float16* ga[4];
  const _Float16* gw[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int id = j * kThreads + tid;
    const int row = id >> 3, cp = id & 7;
    const int c = cp ^ ((row >> 1) & 7);
    ga[j] = A + (size_t)min(m0 + row, M - 1) * K + c * 8;
    gw[j] = W + (size_t)min(n0 + row, N - 1) * K + c * 8;
  }
  auto stage = [&](int buf, int k0) {
    char* sa = smem + buf * kStageBytes + wave * 1024;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      __builtin_amdgcn_global_load_lds((gptr_t)(ga[j] + k0), (lptr_t)(sa + j * (kThreads * 16)), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)(gw[j] + k0), (lptr_t)(sa + BM * 128 + j * (kThreads * 16)), 16, 0, 0);
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int fr = lane & 31, fh = lane >> 5;
  stage(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  int cur = 0;
  for (int k0 = 0; k0 < K; k0 += BK) {
    if (k0 + BK < K) stage(cur ^ 1, k0 + BK);     // next tile in flight under this tile's MFMAs
    const char* sa = smem + cur * kStageBytes;
    const char* sw = sa + BM * 128;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      f16x8 af[2], bf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = *reinterpret_cast<const f16x8*>(sa + lds_off(wm * 64 + i * 32 + fr, ks * 2 + fh));
        bf[i] = *reinterpret_cast<const f16x8*>(sw + lds_off(wn * 64 + i * 32 + fr, ks * 2 + fh));
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue through LDS: accumulators -> fp32 tile [128][128] (the two staging buffers, 64 KiB),
  // then each thread finishes 4 (fp32 out) or 8 (fp16 out) consecutive columns of a row with
  // 16-byte coalesced loads / stores.  Lane holds column (lane & 31), rows (r&3) + 8(r>>2) + 4(lane>>5).
  float* tile = reinterpret_cast<float*>(smem);
  // mode 2: the residual values this thread will add (16 x 16 bytes) are requested BEFORE the accumulators go through
  // LDS -- one global round trip per workgroup.  (As first written the load sat inside the store loop: load, wait, store,
  // sixteen dependent round trips per thread with the matrix pipe idle; same finding as in enc_rowln.hip.)
  constexpr int kIt2 = BM * (BN / 4) / kThreads;   // 16
  const int c4 = (tid % (BN / 4)) * 4, gc2 = n0 + c4;          // this thread's column group is the same in every pass
  // 16-byte accesses only where every row starts 16-byte aligned (N a multiple of 4 here, of 8 for the fp16 stores below), as in the
  // panel and streaming kernels; any other N goes element by element
  const bool cols_in = gc2 + 3 < N && (N & 3) == 0;
  f32x4 rs[kIt2];
  f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 2) {
    if (bias && cols_in) b4 = *reinterpret_cast<const f32x4*>(bias + gc2);
#pragma unroll
    for (int it = 0; it < kIt2; ++it) {
      const int gr = m0 + (tid + it * kThreads) / (BN / 4);
      rs[it] = (gr < M && cols_in) ? *reinterpret_cast<const f32x4*>(residual + (size_t)gr * N + gc2) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * fh;
        tile[row * BN + wn * 64 + j * 32 + fr] = acc[i][j][r];
      }
  __syncthreads();
  if (MODE == 2) {
    float* o = reinterpret_cast<float*>(out);
#pragma unroll
    for (int it = 0; it < kIt2; ++it) {
      const int row = (tid + it * kThreads) / (BN / 4);
      const int gr = m0 + row;
      if (gr >= M || gc2 >= N) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(tile + row * BN + c4);
      const size_t at = (size_t)gr * N + gc2;
      if (cols_in) {
        *reinterpret_cast<f32x4*>(o + at) = v + b4 + rs[it];
      } else {
        for (int e = 0; e < 4 && gc2 + e < N; ++e) o[at + e] = v[e] + (bias ? bias[gc2 + e] : 0.f) + residual[at + e];
      }
    }
  } else if (MODE >= 4) {
    // gated epilogue: the tile's 128 columns are 4 blocks of [16 gate | 16 up] columns (include/crs_encoder.h) = 64 output
    // columns; a thread finishes 8 consecutive output columns of a row, all of one block.  N / 2 is a multiple of 32 (checked by
    // the caller), so an 8-column group is inside the output or outside it as a whole and every row is 16-byte aligned.
    _Float16* o = reinterpret_cast<_Float16*>(out);
    const int NO = N >> 1, o0 = n0 >> 1;
    for (int id = tid; id < BM * (BN / 16); id += kThreads) {
      const int row = id / (BN / 16), c8 = (id % (BN / 16)) * 8;
      const int gr = m0 + row, gc = o0 + c8;
      if (gr >= M || gc >= NO) continue;
      const int tg = 32 * (c8 >> 4) + (c8 & 15);   // the gate's column in the tile; the up value sits 16 columns on
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gt = tile[row * BN + tg + e] + (bias ? bias[n0 + tg + e] : 0.f);
        const float up = tile[row * BN + tg + 16 + e] + (bias ? bias[n0 + tg + 16 + e] : 0.f);
        h[e] = (_Float16)(gate_act<MODE>(gt) * up);
      }
      *reinterpret_cast<f16x8*>(o + (size_t)gr * NO + gc) = h;
    }
  } else {
    _Float16* o = reinterpret_cast<_Float16*>(out);
    for (int id = tid; id < BM * (BN / 8); id += kThreads) {
      const int row = id / (BN / 8), c8 = (id % (BN / 8)) * 8;
      const int gr = m0 + row, gc = n0 + c8;
      if (gr >= M || gc >= N) continue;
      float v[8];
#pragma unroll
      for (int e = 0; e < 8; e += 2) {
        gelu_f32x2 x = {tile[row * BN + c8 + e] + ((bias && gc + e < N) ? bias[gc + e] : 0.f),
                        tile[row * BN + c8 + e + 1] + ((bias && gc + e + 1 < N) ? bias[gc + e + 1] : 0.f)};
        if (MODE == 1) x = gelu_erf2(x);
        v[e] = x[0];
        v[e + 1] = x[1];
      }
      const size_t at = (size_t)gr * N + gc;
      if (gc + 7 < N && (N & 7) == 0) {
        f16x8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (_Float16)v[e];
        *reinterpret_cast<f16x8*>(o + at) = h;
      } else {
        for (int e = 0; e < 8 && gc + e < N; ++e) o[at + e] = (_Float16)v[e];
      }
    }
  }
}


// ---------------------------------------------------------------------------------------------
// Panel variant for the launch/latency-bound regime (query batches: M of a few hundred to a few
// thousand rows).  There the pipelined loop above pays one HBM/L2 round trip per 64-deep K step
// on a grid far smaller than the chip.  Here a workgroup owns a 64 x 64 output tile and ONE K
// chunk of <= 384: it issues every load of both operand panels at once as LDS-DMA
// (global_load_lds_dwordx4, nothing staged in VGPRs), waits once, and runs all its MFMAs out of
// LDS.  Long contractions are split over blockIdx.z (split-K); the fp32 partial tiles are summed
// by the LayerNorm kernel that follows anyway (enc_misc.hip), so no extra pass or atomics exist.
// LDS image: rows of kc halves, 16-byte chunks XOR-swizzled by row inside each 256-byte group;
// the DMA writes LDS linearly, so the swizzle is applied to the per-lane SOURCE address.
typedef float f32x4v __attribute__((ext_vector_type(4)));
constexpr int PN = forms::kPanelN, PKC = forms::kPanelMaxChunk;

// MODE 0: +bias -> fp16; 1: +bias, GELU -> fp16; 3: raw fp32 partial tile -> out[z][M][N]; 4: +bias, silu(gate) * up -> fp16 [M, N / 2]; 5: the same with gelu(gate).
// TM = rows of A per workgroup: 64 (most workgroups, for tiny M) or 128 (halves the operand re-reads
// and the workgroup count -- one wave of workgroups on 256 CUs for the 1024-token query batch).
constexpr int kPanelThreads = forms::kPanelThreads;   // 512, 8 waves: the LDS-DMA issue (1 KiB per wave-instruction) is the long
                                      // pole of a one-shot panel fetch, so it is spread over more waves

template <int MODE, int TM>
__global__ __launch_bounds__(kPanelThreads, 1) void gemm_panel_kernel(const _Float16* __restrict__ A,
                                                                     const _Float16* __restrict__ W,
                                                                     const float* __restrict__ bias,
                                                                     void* __restrict__ out, int M, int N, int K,
                                                                     int kc, int kin) {
  // kin > 1: the workgroup's K range (kc * kin) is walked in kin chunks through ONE staging buffer of kc columns --
  // (TM + 64) * kc * 2 bytes of LDS (48 KB at TM = 128, kc = 128), small enough to sit on a CU beside two scan
  // workgroups, so that the encoder of the next query batch runs in the matrix/issue slots the HBM-bound scan leaves
  // idle instead of waiting for a scan boundary ("encoder beside the scan")
  constexpr int kTiles = (TM / 32) * (PN / 32);   // 32 x 32 output tiles: one per wave (8 or 4)
  extern __shared__ __attribute__((aligned(16))) char psm[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * TM, n0 = blockIdx.x * PN;
  const int cpr = kc >> 3;                 // 16-byte chunks per panel row (multiple of 16)
  char* sa = psm;
  char* sw = psm + TM * cpr * 16;
  const bool computes = wave < kTiles;   // TM = 64: waves 4..7 only help fetching
  const int fr = lane & 31, fh = lane >> 5;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  for (int ci = 0; ci < kin; ++ci) {
  const int k0 = (blockIdx.z * kin + ci) * kc;
  // ---- one shot: every chunk of both panels (rows past M / N are clamped; their results are never
  // stored).  LDS position P = base + tid walks (row, chunk) incrementally: no divisions in the loop.
  {
    int row = tid / cpr, cp = tid - row * cpr;
    const int drow = kPanelThreads / cpr, dcp = kPanelThreads - drow * cpr;
    for (int base = 0; base < TM * cpr; base += kPanelThreads) {
      const int c = (cp & ~15) | ((cp ^ row) & 15);
      const _Float16* ga = A + (size_t)min(m0 + row, M - 1) * K + k0 + c * 8;
      __builtin_amdgcn_global_load_lds((gptr_t)ga, (lptr_t)(sa + (base + wave * 64) * 16), 16, 0, 0);
      if (base < PN * cpr) {
        const _Float16* gw = W + (size_t)min(n0 + row, N - 1) * K + k0 + c * 8;
        __builtin_amdgcn_global_load_lds((gptr_t)gw, (lptr_t)(sw + (base + wave * 64) * 16), 16, 0, 0);
      }
      row += drow;
      cp += dcp;
      if (cp >= cpr) { cp -= cpr; ++row; }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (computes) {
    const int arow = wm * 32 + fr, wrow = wn * 32 + fr;
    const char* pa = sa + arow * (cpr * 16);
    const char* pw = sw + wrow * (cpr * 16);
    const int ksteps = kc >> 4;
#pragma unroll 4
    for (int ks = 0; ks < ksteps; ++ks) {
      const int c = ks * 2 + fh;
      const f16x8 af = *reinterpret_cast<const f16x8*>(pa + (((c & ~15) | ((c ^ arow) & 15)) << 4));
      const f16x8 bf = *reinterpret_cast<const f16x8*>(pw + (((c & ~15) | ((c ^ wrow) & 15)) << 4));
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc, 0, 0, 0);
    }
  }
  __syncthreads();   // every fragment read done: the staging buffer may be refilled / becomes the waves' output tiles
  }
  if (!computes) return;

  // Epilogue through a wave-private LDS tile so that a lane stores 16 bytes of one row: 4 (fp32) or 2 (fp16)
  // store instructions per 32 x 32 tile instead of 16 -- a vector-memory instruction costs the wave ~100
  // cycles of issue whatever its width, and these kernels are latency chains, not bandwidth.
  const int col = n0 + wn * 32 + fr;
  const float b = (MODE != 3 && bias && col < N) ? bias[col] : 0.f;
  const int c0 = n0 + wn * 32, r0 = m0 + wm * 32;
  if (MODE == 3) {
    constexpr int TS = 36;   // floats per tile row (144 bytes: 16-byte aligned, bank-spread)
    float* my = reinterpret_cast<float*>(psm) + wave * (32 * TS);
#pragma unroll
    for (int r = 0; r < 16; ++r) my[((r & 3) + 8 * (r >> 2) + 4 * fh) * TS + fr] = acc[r];
    __builtin_amdgcn_wave_barrier();
    float* o = reinterpret_cast<float*>(out) + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int lrow = q * 8 + (lane >> 3), lc = (lane & 7) * 4;
      const int row = r0 + lrow;
      if (row >= M) continue;
      const f32x4v v = *reinterpret_cast<const f32x4v*>(&my[lrow * TS + lc]);
      float* dst = o + (size_t)row * N + c0 + lc;
      if (c0 + lc + 3 < N && (N & 3) == 0) {
        *reinterpret_cast<f32x4v*>(dst) = v;
      } else {
        for (int e = 0; e < 4 && c0 + lc + e < N; ++e) dst[e] = v[e];
      }
    }
  } else if (MODE >= 4) {
    // gated epilogue: a wave's 32 columns are one block of [16 gate | 16 up] columns (include/crs_encoder.h) = 16 output columns.
    // The biased accumulators go through the wave-private fp32 tile (mode 3's); a lane then finishes 8 output columns of a row:
    // one 16-byte store.  N / 2 is a multiple of 32 (checked by the caller): a wave's block is inside the output or outside it.
    constexpr int TS = 36;
    float* my = reinterpret_cast<float*>(psm) + wave * (32 * TS);
#pragma unroll
    for (int r = 0; r < 16; ++r) my[((r & 3) + 8 * (r >> 2) + 4 * fh) * TS + fr] = acc[r] + b;
    __builtin_amdgcn_wave_barrier();
    if (c0 >= N) return;
    _Float16* o = reinterpret_cast<_Float16*>(out);
    const int NO = N >> 1, lrow = lane >> 1, lc = (lane & 1) * 8;
    const int row = r0 + lrow;
    if (row < M) {
      const f32x4v g0 = *reinterpret_cast<const f32x4v*>(&my[lrow * TS + lc]), g1 = *reinterpret_cast<const f32x4v*>(&my[lrow * TS + lc + 4]);
      const f32x4v u0 = *reinterpret_cast<const f32x4v*>(&my[lrow * TS + 16 + lc]), u1 = *reinterpret_cast<const f32x4v*>(&my[lrow * TS + 20 + lc]);
      f16x8 h;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        h[e] = (_Float16)(gate_act<MODE>(g0[e]) * u0[e]);
        h[e + 4] = (_Float16)(gate_act<MODE>(g1[e]) * u1[e]);
      }
      *reinterpret_cast<f16x8*>(o + (size_t)row * NO + (c0 >> 1) + lc) = h;
    }
  } else {
    constexpr int TS = 40;   // halves per tile row (80 bytes)
    _Float16* my = reinterpret_cast<_Float16*>(psm) + wave * (32 * TS);
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      gelu_f32x2 v = {acc[r] + b, acc[r + 1] + b};
      if (MODE == 1) v = gelu_erf2(v);
      my[((r & 3) + 8 * (r >> 2) + 4 * fh) * TS + fr] = (_Float16)v[0];
      my[(((r + 1) & 3) + 8 * (r >> 2) + 4 * fh) * TS + fr] = (_Float16)v[1];
    }
    __builtin_amdgcn_wave_barrier();
    _Float16* o = reinterpret_cast<_Float16*>(out);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int lrow = q * 16 + (lane >> 2), lc = (lane & 3) * 8;
      const int row = r0 + lrow;
      if (row >= M) continue;
      const f16x8 h = *reinterpret_cast<const f16x8*>(&my[lrow * TS + lc]);
      _Float16* dst = o + (size_t)row * N + c0 + lc;
      if (c0 + lc + 7 < N && (N & 7) == 0) {
        *reinterpret_cast<f16x8*>(dst) = h;
      } else {
        for (int e = 0; e < 8 && c0 + lc + e < N; ++e) dst[e] = h[e];
      }
    }
  }
}

// the plan (plan_gemm_panel) chose the row tile, the staged chunk kc and the chunks walked per workgroup kin
template <int MODE, int TM>
int launch_panel_t(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, void* out, hipStream_t stream) {
  static bool attr_done = false;
  if (!attr_done) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_panel_kernel<MODE, TM>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (TM + PN) * PKC * 2);
    if (e != hipSuccess) return (int)e;
    attr_done = true;
  }
  hipLaunchKernelGGL((gemm_panel_kernel<MODE, TM>), dim3(p.d.gx, p.d.gy, p.d.gz), dim3(kPanelThreads), p.d.lds, stream, a, w, bias, out,
                     p.m, p.n, p.k, p.kc, p.kin);
  return (int)hipGetLastError();
}

template <int MODE>
int launch_panel(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, void* out, hipStream_t stream) {
  return p.tm == 128 ? launch_panel_t<MODE, 128>(p, a, w, bias, out, stream) : launch_panel_t<MODE, 64>(p, a, w, bias, out, stream);
}

}  // namespace

int gemm_launch(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, const float* residual, void* out,
                hipStream_t stream) {
  switch (p.family) {
    case GemmFamily::Gemm8:
    case GemmFamily::Gemm8SplitK: return gemm8_launch(p, a, w, bias, residual, out, stream);
    case GemmFamily::Big: return gemm_big_launch(p, a, w, bias, residual, out, stream);
    case GemmFamily::Stream:
    case GemmFamily::StreamKS: return gemm_stream_launch(p, a, w, bias, residual, out, stream);
    case GemmFamily::Panel:   // out: mode 0 / 1 fp16 [M, N]; mode 3 fp32 [slabs][M][N] partials; mode 4 fp16 [M, N / 2]
      switch (p.mode) {
        case 0: return launch_panel<0>(p, a, w, bias, out, stream);
        case 1: return launch_panel<1>(p, a, w, bias, out, stream);
        case 3: return launch_panel<3>(p, a, w, bias, out, stream);
        case 4: return launch_panel<4>(p, a, w, bias, out, stream);
        case 5: return launch_panel<5>(p, a, w, bias, out, stream);
        default: return -1;
      }
    case GemmFamily::Tiled: {
      const dim3 grid(p.d.gx);
      switch (p.mode) {
        case 0: hipLaunchKernelGGL((gemm_f16_kernel<0>), grid, dim3(kThreads), 0, stream, a, w, bias, residual, out, p.m, p.n, p.k); break;
        case 1: hipLaunchKernelGGL((gemm_f16_kernel<1>), grid, dim3(kThreads), 0, stream, a, w, bias, residual, out, p.m, p.n, p.k); break;
        case 2: hipLaunchKernelGGL((gemm_f16_kernel<2>), grid, dim3(kThreads), 0, stream, a, w, bias, residual, out, p.m, p.n, p.k); break;
        case 4: hipLaunchKernelGGL((gemm_f16_kernel<4>), grid, dim3(kThreads), 0, stream, a, w, bias, residual, out, p.m, p.n, p.k); break;
        case 5: hipLaunchKernelGGL((gemm_f16_kernel<5>), grid, dim3(kThreads), 0, stream, a, w, bias, residual, out, p.m, p.n, p.k); break;
        default: return -1;
      }
      return (int)hipGetLastError();
    }
    default: return -1;
  }
}

}  // namespace crs
