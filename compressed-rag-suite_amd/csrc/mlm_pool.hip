// mlm_pool.hip -- the masked-language-model head of a learned sparse encoder (SPLADE) with the max-pool in the vocabulary
// projection's epilogue (gfx950): crs_mlm_sparse_pool.
//
//     t_i       = LayerNorm(GELU(W_t h_i + b_t))                  i < lens[b]
//     out[b, v] = log1p(max(0, max_i (t_i . Wd_v + bias_v)))
//
// Four launches on one stream, walking the plan of mlm_plan.cpp; the [tokens, V] logits never exist in memory.
//   mlm_zero_kernel       out[b, 0 .. V) = 0 (columns [V, Vp) are the caller's and are not touched).
//   mlm_transform_kernel  one workgroup per 32 token rows, four waves.  A row-complete MFMA tile as token_project.hip's: wave w owns
//                         the 16-column tiles w, w + 4, ... of ALL of H for both 16-row blocks (2 x H / 64 accumulator tiles of
//                         v_mfma_f32_16x16x32_f16), so the LayerNorm statistics are formed from registers: per row a butterfly over
//                         the 16 lanes of a column tile, then the four waves' partial sums through 1 KB of LDS, added in wave
//                         order.  Two passes (mean, then the centred squares).  A operand: the fp32 hidden row, rounded to fp16 in
//                         registers; a padding position (i >= lens[b]) or a row past the last token is NEVER read -- its fragment
//                         is zeros and its row of t is written as zeros, so that no later load meets undefined memory.  B operand:
//                         W_t straight from global memory (at most 2 MB, L2-resident).
//   mlm_pool_kernel       the vocabulary projection: 128 x 128 output tile per workgroup, four waves 2 x 2, each 4 x 4 accumulator
//                         tiles (64 VGPRs); K staged 64 at a time through LDS (A and B tiles, rows padded by 16 bytes), the next
//                         step's global loads in flight under the MFMAs.  B rows at or past V are zeros and are not read.
//                         Epilogue, per wave and per sequence b that its 64 rows touch: each lane takes the maximum of
//                         (acc + bias) over its rows that lie in [b seq, b seq + lens[b]), starting from 0; the four row groups
//                         are joined by two butterflies; one atomic integer maximum per column on the bit pattern of the
//                         non-negative float into out[b, v] -- exact and order-free, so tiles may finish in any order.
//   mlm_log1p_kernel      out[b, v] = (float)log1p((double)out[b, v]).  Taken after the maximum (log1p is monotone, so it
//                         commutes with it mathematically; taken before, two tiles' candidates would meet already rounded).
// A text's row depends on its own real tokens alone: every accumulator sums one A row against one B row in ascending k, and the
// maximum is exact.  No scratch, no host synchronisation, nothing waits on another workgroup.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "enc.h"
#include "enc_gelu.h"
#include "mlm_plan.h"

namespace crs {
namespace {

typedef _Float16 mp_f16x8 __attribute__((ext_vector_type(8)));
typedef float mp_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int mp_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kMlmThreads) void mlm_zero_kernel(float* __restrict__ out, int V, int Vp) {
  const int v = blockIdx.x * kMlmThreads + threadIdx.x;
  if (v < V) out[(size_t)blockIdx.y * Vp + v] = 0.0f;
}

__global__ __launch_bounds__(kMlmThreads) void mlm_log1p_kernel(float* __restrict__ out, int V, int Vp) {
  const int v = blockIdx.x * kMlmThreads + threadIdx.x;
  if (v < V) {
    float* p = out + (size_t)blockIdx.y * Vp + v;
    *p = (float)log1p((double)*p);
  }
}

// ---- the transform ---------------------------------------------------------------------------------------------------------------
template <int NJ>   // column tiles of 16 per wave: H = 64 NJ
__global__ __launch_bounds__(kMlmThreads) void mlm_transform_kernel(const float* __restrict__ hidden, const int* __restrict__ lens,
                                                                   int seq, int M, const _Float16* __restrict__ wt,
                                                                   const float* __restrict__ bt, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, float eps,
                                                                   _Float16* __restrict__ t16) {
  constexpr int H = 64 * NJ;
  constexpr int RT = kMlmXformRows / 16;
  __shared__ float part[2][4][kMlmXformRows];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 15, h = lane >> 4;
  const int row0 = blockIdx.x * kMlmXformRows;

  // rows of the A operand: lane (r, h) reads row 16 rt + r
  bool live[RT];
  const float* hrow[RT];
  unsigned long long live_mask[RT];                    // bit r (< 16): row 16 rt + r is a real token
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) {
    const int tok = row0 + 16 * rt + r;
    live[rt] = false;
    if (tok < M) {
      const int b = tok / seq, i = tok - b * seq;
      live[rt] = i < mp_clamp(lens[b], 0, seq);
    }
    hrow[rt] = hidden + (size_t)(live[rt] ? tok : 0) * H + 8 * h;
    live_mask[rt] = __ballot(live[rt]);
  }

  mp_f32x4 acc[RT][NJ];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int j = 0; j < NJ; ++j) acc[rt][j] = mp_f32x4{0.f, 0.f, 0.f, 0.f};

  bool any = false;
#pragma unroll
  for (int rt = 0; rt < RT; ++rt) any = any || live_mask[rt] != 0ull;
  if (any) {                                           // (the same in all four waves: every wave looks at all 32 rows)
    const _Float16* wrow = wt + (size_t)(16 * wave + r) * H + 8 * h;
    for (int k0 = 0; k0 < H; k0 += 32) {
      mp_f16x8 af[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        af[rt] = mp_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (live[rt]) {
          const mp_f32x4 lo = *reinterpret_cast<const mp_f32x4*>(hrow[rt] + k0), hi = *reinterpret_cast<const mp_f32x4*>(hrow[rt] + k0 + 4);
          af[rt] = mp_f16x8{(_Float16)lo[0], (_Float16)lo[1], (_Float16)lo[2], (_Float16)lo[3],
                            (_Float16)hi[0], (_Float16)hi[1], (_Float16)hi[2], (_Float16)hi[3]};
        }
      }
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        const mp_f16x8 bf = *reinterpret_cast<const mp_f16x8*>(wrow + (size_t)(64 * j) * H + k0);   // W_t row 16 (wave + 4 j) + r
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[rt], bf, acc[rt][j], 0, 0, 0);
      }
    }
  }

  // ---- epilogue.  Register e of lane (c = lane & 15, g = lane >> 4), tile j is column 16 (wave + 4 j) + c of row 16 rt + 4 g + e.
  const int c = r, g = h;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const float bj = bt[16 * (wave + 4 * j) + c];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const gelu_f32x2 a = gelu_erf2(gelu_f32x2{acc[rt][j][0] + bj, acc[rt][j][1] + bj});
      const gelu_f32x2 b = gelu_erf2(gelu_f32x2{acc[rt][j][2] + bj, acc[rt][j][3] + bj});
      acc[rt][j] = mp_f32x4{a[0], a[1], b[0], b[1]};
    }
  }
  float mean[RT][4], inv[RT][4];
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const float d = pass ? acc[rt][j][e] - mean[rt][e] : acc[rt][j][e];
          s += pass ? d * d : d;
        }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (c == 0) part[pass][wave][16 * rt + 4 * g + e] = s;
      }
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = 16 * rt + 4 * g + e;
        const float s = ((part[pass][0][row] + part[pass][1][row]) + part[pass][2][row]) + part[pass][3][row];
        if (pass == 0) mean[rt][e] = s * (1.0f / H);
        else inv[rt][e] = 1.0f / sqrtf(s * (1.0f / H) + eps);
      }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int col = 16 * (wave + 4 * j) + c;
    const float gj = gamma[col], bej = beta[col];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int lr = 4 * g + e;
        const bool row_live = (live_mask[rt] >> lr) & 1ull;
        const float y = (acc[rt][j][e] - mean[rt][e]) * inv[rt][e] * gj + bej;
        t16[(size_t)(row0 + 16 * rt + lr) * H + col] = row_live ? (_Float16)y : (_Float16)0.0f;
      }
  }
}

// ---- the vocabulary projection with the max-pool epilogue ----------------------------------------------------------------------------
__global__ __launch_bounds__(kMlmThreads) void mlm_pool_kernel(const _Float16* __restrict__ t16, const _Float16* __restrict__ wd,
                                                              const float* __restrict__ bias, const int* __restrict__ lens, int seq,
                                                              int M, int H, int V, int Vp, int grid_m, int grid_n,
                                                              float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) _Float16 smem[2 * kMlmTileM * kMlmLdsRow];
  _Float16* sA = smem;
  _Float16* sB = smem + kMlmTileM * kMlmLdsRow;

  // consecutive workgroups share kMlmGroupM row tiles and walk the vocabulary: what runs together re-reads little of either operand
  const int id = blockIdx.x;
  const int per_group = kMlmGroupM * grid_n;
  const int group = id / per_group, in_group = id - group * per_group;
  const int first_m = group * kMlmGroupM;
  const int gsz = grid_m - first_m < kMlmGroupM ? grid_m - first_m : kMlmGroupM;
  const int pn = in_group / gsz, pm = first_m + (in_group - pn * gsz);
  const int m0 = pm * kMlmTileM, n0 = pn * kMlmTileN;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wr = wave >> 1, wc = wave & 1;
  const int r = lane & 15, h = lane >> 4;

  // staging: 16-byte piece p = tid + 256 i of a 128 x 64 tile is row p >> 3, halves 8 (p & 7) ..
  const _Float16* a_src[4];
  const _Float16* b_src[4];
  bool b_ok[4];
  int s_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = tid + kMlmThreads * i, row = p >> 3, kc = p & 7;
    a_src[i] = t16 + (size_t)(m0 + row) * H + 8 * kc;            // rows < tokens_padded: t16 holds whole row tiles
    b_ok[i] = n0 + row < V;
    b_src[i] = wd + (size_t)(b_ok[i] ? n0 + row : 0) * H + 8 * kc;
    s_off[i] = row * kMlmLdsRow + 8 * kc;
  }
  mp_f16x8 ra[4], rb[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const mp_f16x8*>(a_src[i] + k0);
      rb[i] = mp_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (b_ok[i]) rb[i] = *reinterpret_cast<const mp_f16x8*>(b_src[i] + k0);
    }
  };

  mp_f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = mp_f32x4{0.f, 0.f, 0.f, 0.f};

  const _Float16* fa = sA + (wr * 64 + r) * kMlmLdsRow + 8 * h;
  const _Float16* fb = sB + (wc * 64 + r) * kMlmLdsRow + 8 * h;
  fetch(0);
  for (int k0 = 0; k0 < H; k0 += kMlmTileK) {
    __syncthreads();                                   // the previous step's fragments have been read
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<mp_f16x8*>(sA + s_off[i]) = ra[i];
      *reinterpret_cast<mp_f16x8*>(sB + s_off[i]) = rb[i];
    }
    __syncthreads();
    if (k0 + kMlmTileK < H) fetch(k0 + kMlmTileK);     // in flight under the MFMAs
#pragma unroll
    for (int kk = 0; kk < kMlmTileK; kk += 32) {
      mp_f16x8 af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        af[i] = *reinterpret_cast<const mp_f16x8*>(fa + 16 * i * kMlmLdsRow + kk);
        bf[i] = *reinterpret_cast<const mp_f16x8*>(fb + 16 * i * kMlmLdsRow + kk);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue.  Register e of lane (c, g), tile (i, j) is column n0 + 64 wc + 16 j + c of token row R0 + 16 i + 4 g + e.
  const int R0 = m0 + wr * 64;
  if (R0 >= M) return;                                 // (wave-uniform) rows past the last token
  const int c = r, g = h;
  float bj[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = n0 + wc * 64 + 16 * j + c;
    bj[j] = col < V ? bias[col] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][j][e] += bj[j];
  }
  const int last_row = R0 + 63 < M - 1 ? R0 + 63 : M - 1;
  const int b_first = R0 / seq, b_last = last_row / seq;
  const int my_col = n0 + wc * 64 + 16 * g + c;        // the column this lane publishes: tile j == g
  for (int b = b_first; b <= b_last; ++b) {            // (wave-uniform)
    const int lo = b * seq - R0, hi = lo + mp_clamp(lens[b], 0, seq);    // the sequence's real tokens, as rows of this wave's 64
    float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int lr = 16 * i + 4 * g + e;
        const bool in = lr >= lo && lr < hi;
#pragma unroll
        for (int j = 0; j < 4; ++j) m[j] = in ? fmaxf(m[j], acc[i][j][e]) : m[j];
      }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m[j] = fmaxf(m[j], __shfl_xor(m[j], 16));
      m[j] = fmaxf(m[j], __shfl_xor(m[j], 32));
    }
    const float v = g == 0 ? m[0] : (g == 1 ? m[1] : (g == 2 ? m[2] : m[3]));
    if (my_col < V && v > 0.f) atomicMax(reinterpret_cast<int*>(out + (size_t)b * Vp + my_col), __float_as_int(v));
  }
}

}  // namespace

int mlm_sparse_pool_launch(const crs_mlm_plan& p, const float* hidden32, const int* lens, int batch, int seq, const crs_mlm_head& head,
                           _Float16* t16, float* out, int vp, hipStream_t stream) {
  const int H = head.hidden, V = head.vocab, M = p.tokens;
  const _Float16* wt = static_cast<const _Float16*>(head.transform_w16);
  const _Float16* wd = static_cast<const _Float16*>(head.decoder_w16);
  const dim3 ew_grid((unsigned)p.ew_grid_x, (unsigned)batch);
  hipLaunchKernelGGL(mlm_zero_kernel, ew_grid, dim3(p.ew_threads), 0, stream, out, V, vp);
#define CRS_MLM_XFORM(NJ)                                                                                                          \
  hipLaunchKernelGGL(mlm_transform_kernel<NJ>, dim3((unsigned)p.xform_grid), dim3(p.xform_threads), 0, stream, hidden32, lens, seq, \
                     M, wt, head.transform_bias, head.ln_gamma, head.ln_beta, head.ln_eps, t16)
  switch (H) {
    case 64: CRS_MLM_XFORM(1); break;
    case 128: CRS_MLM_XFORM(2); break;
    case 256: CRS_MLM_XFORM(4); break;
    case 384: CRS_MLM_XFORM(6); break;
    case 512: CRS_MLM_XFORM(8); break;
    case 768: CRS_MLM_XFORM(12); break;
    case 1024: CRS_MLM_XFORM(16); break;
    default: return -1;
  }
#undef CRS_MLM_XFORM
  hipLaunchKernelGGL(mlm_pool_kernel, dim3((unsigned)p.pool_grid), dim3(p.pool_threads), 0, stream, t16, wd, head.decoder_bias, lens, seq,
                     M, H, V, vp, p.grid_m, p.grid_n, out);
  hipLaunchKernelGGL(mlm_log1p_kernel, ew_grid, dim3(p.ew_threads), 0, stream, out, V, vp);
  return (int)hipGetLastError();
}

}  // namespace crs
