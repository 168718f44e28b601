// enc_misc.hip -- K1 (embedding gather + LayerNorm), LayerNorm, K7/K8 (pooling + L2 normalise).
// All HBM-bound row kernels: one wave64 per token row (hidden <= 1024 -> <= 16 elements per lane),
// statistics in fp32 with a two-pass (mean, then centred variance) form, eps inside the sqrt
// exactly as torch.nn.LayerNorm.  Each writes the fp32 residual stream AND the fp16 copy the next
// GEMM reads, so no separate cast pass exists.

#include "enc.h"
#include "enc_ln.h"

namespace crs {
namespace {

constexpr int kMaxPerLane = 16;  // hidden <= 1024 (generic instantiation); hot shapes get exact counts

// wave_sum, ln_store<PL> (4-byte columns lane + 64 i) and ln_store2<P2> (8-byte column pairs 128 i + 2 lane): enc_ln.h

__device__ __forceinline__ int clamp_row(int i, int rows) { return i < 0 ? 0 : (i >= rows ? rows - 1 : i); }

// Embedding gather + LayerNorm, two forms (float2 column pairs at hidden 384 / 768, 4-byte columns otherwise).  TYPES: the
// token-type row is looked up per token (type_ids[t] clamped to [0, type_rows): the segment ids of "[CLS] a [SEP] b [SEP]");
// without it row 0 is added and type_ids / type_rows are not read.  Same sum order either way, so an all-zero type block
// gives the bits of the plain form.
template <int P2, bool TYPES>
__global__ __launch_bounds__(256) void embed_ln2_kernel(const int* __restrict__ ids, const float* __restrict__ word,
                                                       const float* __restrict__ pos, const float* __restrict__ type_tab,
                                                       const float* __restrict__ g, const float* __restrict__ b,
                                                       float eps, int tokens, int seq, int hidden, int vocab,
                                                       float* __restrict__ x32, _Float16* __restrict__ x16,
                                                       const int* __restrict__ type_ids, int type_rows) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* w = word + (size_t)clamp_row(ids[t], vocab) * hidden;
  const float* type0 = type_tab;
  if constexpr (TYPES) type0 += (size_t)clamp_row(type_ids[t], type_rows) * hidden;
  const float* p = pos ? pos + (size_t)(t % seq) * hidden : nullptr;   // null: no position row (rotary models)
  float v[P2][2];
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const int c = 128 * i + 2 * lane;
    const float2 a = *reinterpret_cast<const float2*>(w + c), ty = *reinterpret_cast<const float2*>(type0 + c),
                 pp = p ? *reinterpret_cast<const float2*>(p + c) : float2{0.f, 0.f};
    v[i][0] = (a.x + ty.x) + pp.x;   // (word + token_type) + position, as modeling_bert
    v[i][1] = (a.y + ty.y) + pp.y;
  }
  ln_store2<P2>(v, hidden, lane, g, b, eps, x32 + (size_t)t * hidden, x16 + (size_t)t * hidden);
}

template <int P2, int NS>
__global__ __launch_bounds__(256) void layernorm2_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                        const float* residual,   // may alias x32 (in place)
                                                        const float* __restrict__ g, const float* __restrict__ b,
                                                        float eps, int tokens, int hidden, float* x32,
                                                        _Float16* __restrict__ x16) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* src = y + (size_t)t * hidden;
  const size_t split_stride = (size_t)tokens * hidden;
  float2 part[NS][P2], extra[2][P2];
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const int c = 128 * i + 2 * lane;
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) part[sidx][i] = *reinterpret_cast<const float2*>(src + sidx * split_stride + c);
    extra[0][i] = bias ? *reinterpret_cast<const float2*>(bias + c) : float2{0.f, 0.f};
    extra[1][i] = residual ? *reinterpret_cast<const float2*>(residual + (size_t)t * hidden + c) : float2{0.f, 0.f};
  }
  float v[P2][2];
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    float a0 = part[0][i].x, a1 = part[0][i].y;
#pragma unroll
    for (int sidx = 1; sidx < NS; ++sidx) { a0 += part[sidx][i].x; a1 += part[sidx][i].y; }
    v[i][0] = (a0 + extra[0][i].x) + extra[1][i].x;
    v[i][1] = (a1 + extra[0][i].y) + extra[1][i].y;
  }
  ln_store2<P2>(v, hidden, lane, g, b, eps, x32 + (size_t)t * hidden, x16 + (size_t)t * hidden);
}

template <int PL, bool TYPES>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int* __restrict__ ids, const float* __restrict__ word,
                                                      const float* __restrict__ pos, const float* __restrict__ type_tab,
                                                      const float* __restrict__ g, const float* __restrict__ b,
                                                      float eps, int tokens, int seq, int hidden, int vocab,
                                                      float* __restrict__ x32, _Float16* __restrict__ x16,
                                                      const int* __restrict__ type_ids, int type_rows) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* w = word + (size_t)clamp_row(ids[t], vocab) * hidden;
  const float* type0 = type_tab;
  if constexpr (TYPES) type0 += (size_t)clamp_row(type_ids[t], type_rows) * hidden;
  const float* p = pos ? pos + (size_t)(t % seq) * hidden : nullptr;   // null: no position row (rotary models)
  float v[PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int c = lane + 64 * i;
    v[i] = (c < hidden) ? (w[c] + type0[c]) + (p ? p[c] : 0.f) : 0.f;   // (word + token_type) + position, as modeling_bert
  }
  ln_store<PL>(v, hidden, lane, g, b, eps, x32 + (size_t)t * hidden, x16 + (size_t)t * hidden);
}

// y: [NS][tokens][hidden] fp32 split-K partial sums of the preceding GEMM (NS = 1: the full product);
// bias / residual are added here when given, so the GEMM needs no epilogue pass.  NS is a template
// parameter so that every partial-sum load of a row is in flight at once (a runtime loop made hipcc
// wait for each split before issuing the next: one memory round trip per split).
template <int PL, int NS>
__global__ __launch_bounds__(256) void layernorm_kernel(const float* __restrict__ y,
                                                       const float* __restrict__ bias,
                                                       const float* residual,   // may alias x32 (in place)
                                                       const float* __restrict__ g,
                                                       const float* __restrict__ b, float eps, int tokens,
                                                       int hidden, float* x32, _Float16* __restrict__ x16) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* src = y + (size_t)t * hidden;
  const size_t split_stride = (size_t)tokens * hidden;
  float part[NS][PL], extra[2][PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int c = lane + 64 * i;
    const bool in = c < hidden;
#pragma unroll
    for (int sidx = 0; sidx < NS; ++sidx) part[sidx][i] = in ? src[sidx * split_stride + c] : 0.f;
    extra[0][i] = (in && bias) ? bias[c] : 0.f;
    extra[1][i] = (in && residual) ? residual[(size_t)t * hidden + c] : 0.f;
  }
  float v[PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    float a = part[0][i];
#pragma unroll
    for (int sidx = 1; sidx < NS; ++sidx) a += part[sidx][i];
    v[i] = (a + extra[0][i]) + extra[1][i];
  }
  ln_store<PL>(v, hidden, lane, g, b, eps, x32 + (size_t)t * hidden, x16 + (size_t)t * hidden);
}

// one 256-thread block per sentence: mean over the real tokens (sum / clamp(count, 1e-9)) or the
// [CLS] row, then x / max(||x||, 1e-12).  Thread t owns columns t, t+256, ...; the token loop is
// unrolled so several rows are in flight per thread.
__global__ __launch_bounds__(256) void pool_kernel(const float* __restrict__ x32, const int* __restrict__ lens,
                                                  int batch, int seq, int hidden, int pooling, int normalize,
                                                  float* __restrict__ out, _Float16* __restrict__ out16, int pdim16) {
  __shared__ float red[4];
  __shared__ float part[4][1024];        // mean pooling: one partial row per wave (hidden <= 1024)
  const int bi = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = x32 + (size_t)bi * seq * hidden;
  int len = lens[bi];
  len = len < 0 ? 0 : (len > seq ? seq : len);
  float v[4] = {0.f, 0.f, 0.f, 0.f};   // hidden <= 1024
  if (pooling == 1) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      if (c < hidden) v[i] = base[c];
    }
  } else {
    // Mean over the real tokens.  Wave w sums tokens w, w + 4, ...; a lane covers column pairs 2 lane + 128 p (8-byte
    // loads), four tokens unrolled: up to 32 loads of 8 bytes in flight per lane.  (A thread per column walking the
    // tokens four 4-byte loads at a time kept 4 KB in flight per workgroup: 50 us for 256 x 256 x 384 at index build.)
    const int npair = (hidden + 127) >> 7;        // passes of 128 columns: 3 (hidden 384), 6 (768), 8 (1024)
    for (int p = 0; p < npair; ++p) {
      const int c = 2 * lane + 128 * p;
      float2 a[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
      if (c < hidden) {                            // hidden is even (head_dim multiples)
        int t = wave;
        for (; t + 12 < len; t += 16) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float2 x = *reinterpret_cast<const float2*>(base + (size_t)(t + 4 * u) * hidden + c);
            a[u].x += x.x;
            a[u].y += x.y;
          }
        }
        for (; t < len; t += 4) {
          const float2 x = *reinterpret_cast<const float2*>(base + (size_t)t * hidden + c);
          a[0].x += x.x;
          a[0].y += x.y;
        }
        part[wave][c] = (a[0].x + a[1].x) + (a[2].x + a[3].x);
        part[wave][c + 1] = (a[0].y + a[1].y) + (a[2].y + a[3].y);
      }
    }
    __syncthreads();
    const float inv = 1.0f / fmaxf((float)len, 1e-9f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = tid + 256 * i;
      if (c < hidden) v[i] = ((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) * inv;
    }
  }
  float scale = 1.f;
  if (normalize) {
    float q = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    q = wave_sum(q);
    if (lane == 0) red[wave] = q;
    __syncthreads();
    q = red[0] + red[1] + red[2] + red[3];
    scale = 1.0f / fmaxf(sqrtf(q), 1e-12f);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = tid + 256 * i;
    if (c < hidden) out[(size_t)bi * hidden + c] = v[i] * scale;
    // optional fp16 copy in the scan's query layout (row zero-padded to pdim16): saves the separate
    // normalise + cast launch between the encoder and the scan
    if (out16 && c < pdim16) out16[(size_t)bi * pdim16 + c] = (c < hidden) ? (_Float16)(v[i] * scale) : (_Float16)0.f;
  }
}

}  // namespace

int embed_ln_launch(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type_tab,
                    int type_rows, const float* g, const float* b, float eps, int tokens, int seq, int hidden, int vocab,
                    float* x32, _Float16* x16, hipStream_t stream) {
#define CRS_EMB(KERNEL, N)                                                                                                  \
  do {                                                                                                                      \
    if (type_ids) hipLaunchKernelGGL((KERNEL<N, true>), dim3((tokens + 3) / 4), dim3(256), 0, stream, ids, word, pos,       \
                                     type_tab, g, b, eps, tokens, seq, hidden, vocab, x32, x16, type_ids, type_rows);       \
    else hipLaunchKernelGGL((KERNEL<N, false>), dim3((tokens + 3) / 4), dim3(256), 0, stream, ids, word, pos, type_tab, g,  \
                            b, eps, tokens, seq, hidden, vocab, x32, x16, type_ids, type_rows);                             \
  } while (0)
  // the form per hidden size: with and without type ids the sums meet in the same order
  if (hidden == 384) CRS_EMB(embed_ln2_kernel, 3); else if (hidden == 768) CRS_EMB(embed_ln2_kernel, 6);
  else if (hidden <= 64) CRS_EMB(embed_ln_kernel, 1); else CRS_EMB(embed_ln_kernel, 16);
#undef CRS_EMB
  return (int)hipGetLastError();
}

int layernorm_launch(const float* y, int nsplit, const float* bias, const float* residual, const float* g,
                     const float* b, float eps, int tokens, int hidden, float* x32, _Float16* x16,
                     hipStream_t stream) {
#define CRS_LN_CASE(KERNEL, PL, NS)                                                                                        \
  case NS: hipLaunchKernelGGL((KERNEL<PL, NS>), dim3((tokens + 3) / 4), dim3(256), 0, stream, y, bias, residual, g, b, eps, tokens, \
                              hidden, x32, x16); break;
#define CRS_LN(KERNEL, PL) switch (nsplit) { CRS_LN_SLABS(CRS_LN_CASE, KERNEL, PL) default: return -1; }
  // the form per hidden size (forms::row_form), every slab count of enc_forms.h
  if (hidden == 384) { CRS_LN(layernorm2_kernel, 3) } else if (hidden == 768) { CRS_LN(layernorm2_kernel, 6) }
  else if (hidden <= 64) { CRS_LN(layernorm_kernel, 1) } else { CRS_LN(layernorm_kernel, 16) }
#undef CRS_LN
#undef CRS_LN_CASE
  return (int)hipGetLastError();
}

int pool_launch(const float* x32, const int* lens, int batch, int seq, int hidden, int pooling, int normalize,
                float* out, _Float16* out16, int pdim16, hipStream_t stream) {
  hipLaunchKernelGGL(pool_kernel, dim3(batch), dim3(256), 0, stream, x32, lens, batch, seq, hidden,
                     pooling, normalize, out, out16, pdim16);
  return (int)hipGetLastError();
}

}  // namespace crs
