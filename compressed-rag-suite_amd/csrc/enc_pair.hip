// enc_pair.hip -- the two kernels a sentence-PAIR classifier (cross-encoder) adds to the encoder:
//   embed_ln*_types_kernel   embedding gather + LayerNorm with a token-type row PER TOKEN (segment ids of "[CLS] a [SEP] b [SEP]")
//   pair_head_kernel         score = w_c . tanh(W_p h_CLS + b_p) + b_c  (BertPooler + a one-label classifier), optional sigmoid
// The embedding kernels are the ones of enc_misc.hip with the type row looked up per token: same forms for the same hidden sizes
// (float2 columns at 384 / 768, 4-byte columns otherwise), same sum order (word + type) + position, same LayerNorm (enc_ln.h) --
// an all-zero type block gives the bits of the kernels that always add row 0.

#include "enc.h"
#include "enc_ln.h"

namespace crs {
namespace {

__device__ __forceinline__ int clamp_row(int i, int rows) { return i < 0 ? 0 : (i >= rows ? rows - 1 : i); }

template <int P2>
__global__ __launch_bounds__(256) void embed_ln2_types_kernel(const int* __restrict__ ids, const int* __restrict__ type_ids,
                                                             const float* __restrict__ word, const float* __restrict__ pos,
                                                             const float* __restrict__ type_tab, int type_rows,
                                                             const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                             int tokens, int seq, int hidden, int vocab,
                                                             float* __restrict__ x32, _Float16* __restrict__ x16) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* w = word + (size_t)clamp_row(ids[t], vocab) * hidden;
  const float* tr = type_tab + (size_t)clamp_row(type_ids[t], type_rows) * hidden;
  const float* p = pos + (size_t)(t % seq) * hidden;
  float v[P2][2];
#pragma unroll
  for (int i = 0; i < P2; ++i) {
    const int c = 128 * i + 2 * lane;
    const float2 a = *reinterpret_cast<const float2*>(w + c), ty = *reinterpret_cast<const float2*>(tr + c),
                 pp = *reinterpret_cast<const float2*>(p + c);
    v[i][0] = (a.x + ty.x) + pp.x;   // (word + token_type) + position, as modeling_bert
    v[i][1] = (a.y + ty.y) + pp.y;
  }
  ln_store2<P2>(v, hidden, lane, g, b, eps, x32 + (size_t)t * hidden, x16 + (size_t)t * hidden);
}

template <int PL>
__global__ __launch_bounds__(256) void embed_ln_types_kernel(const int* __restrict__ ids, const int* __restrict__ type_ids,
                                                            const float* __restrict__ word, const float* __restrict__ pos,
                                                            const float* __restrict__ type_tab, int type_rows,
                                                            const float* __restrict__ g, const float* __restrict__ b, float eps,
                                                            int tokens, int seq, int hidden, int vocab,
                                                            float* __restrict__ x32, _Float16* __restrict__ x16) {
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= tokens) return;
  const float* w = word + (size_t)clamp_row(ids[t], vocab) * hidden;
  const float* tr = type_tab + (size_t)clamp_row(type_ids[t], type_rows) * hidden;
  const float* p = pos + (size_t)(t % seq) * hidden;
  float v[PL];
#pragma unroll
  for (int i = 0; i < PL; ++i) {
    const int c = lane + 64 * i;
    v[i] = (c < hidden) ? (w[c] + tr[c]) + p[c] : 0.f;   // (word + token_type) + position, as modeling_bert
  }
  ln_store<PL>(v, hidden, lane, g, b, eps, x32 + (size_t)t * hidden, x16 + (size_t)t * hidden);
}

// One 256-thread workgroup serves kPairGroup pairs: their [CLS] rows sit in LDS (kPairGroup x H floats: 24 KB at H = 768, 32 KB at
// the largest H), and every row of W_p a wave loads is used for all of them, so W_p (H x H fp32: 2.3 MB at 768) is read once per
// group instead of once per pair.  Wave w owns the pooler's output rows w, w + 4, ...: the lanes read one row of W_p coalesced
// (VEC = 2: 8-byte column pairs, H a multiple of 128; VEC = 1 otherwise), multiply it into the kPairGroup vectors, and a wave
// reduction leaves every lane with the full dot products; tanh, and the classifier's term w_c[j] * pooled[j] is added to the
// wave's running sum of each pair.  The four waves' sums meet in LDS in a fixed order.  A pair's result does not depend on its
// place in the group or on the batch it came in.
constexpr int kPairGroup = 8;

template <int VEC>
__global__ __launch_bounds__(256) void pair_head_kernel(const float* __restrict__ hidden32, int batch, int seq, int hidden,
                                                       const float* __restrict__ w_pool, const float* __restrict__ b_pool,
                                                       const float* __restrict__ w_cls, const float* __restrict__ b_cls,
                                                       int activation, float* __restrict__ scores, float* __restrict__ pooled_out) {
  extern __shared__ float hs[];                  // [kPairGroup][hidden]: token 0 of each pair of the group
  __shared__ float part[4][kPairGroup];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int p0 = blockIdx.x * kPairGroup;
  const int np = (batch - p0 < kPairGroup) ? batch - p0 : kPairGroup;
  for (int i = tid; i < kPairGroup * hidden; i += 256) {
    const int gi = i / hidden, c = i - gi * hidden;
    hs[i] = (gi < np) ? hidden32[(size_t)(p0 + gi) * seq * hidden + c] : 0.f;
  }
  __syncthreads();
  float cls[kPairGroup];
#pragma unroll
  for (int gi = 0; gi < kPairGroup; ++gi) cls[gi] = 0.f;
  for (int j = wave; j < hidden; j += 4) {
    const float* wr = w_pool + (size_t)j * hidden;
    float acc[kPairGroup];
#pragma unroll
    for (int gi = 0; gi < kPairGroup; ++gi) acc[gi] = 0.f;
    for (int c = VEC * lane; c < hidden; c += 64 * VEC) {
      if (VEC == 2) {
        const float2 w2 = *reinterpret_cast<const float2*>(wr + c);
#pragma unroll
        for (int gi = 0; gi < kPairGroup; ++gi) {
          const float2 h2 = *reinterpret_cast<const float2*>(hs + gi * hidden + c);
          acc[gi] += w2.x * h2.x;
          acc[gi] += w2.y * h2.y;
        }
      } else {
        const float w1 = wr[c];
#pragma unroll
        for (int gi = 0; gi < kPairGroup; ++gi) acc[gi] += w1 * hs[gi * hidden + c];
      }
    }
    const float bj = b_pool[j], wj = w_cls[j];
#pragma unroll
    for (int gi = 0; gi < kPairGroup; ++gi) {
      const float pooled = tanhf(wave_sum(acc[gi]) + bj);
      cls[gi] += wj * pooled;
      if (pooled_out && lane == 0 && gi < np) pooled_out[(size_t)(p0 + gi) * hidden + j] = pooled;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int gi = 0; gi < kPairGroup; ++gi) part[wave][gi] = cls[gi];
  }
  __syncthreads();
  if (tid < np) {
    float s = ((part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid])) + b_cls[0];
    if (activation == 1) s = 1.0f / (1.0f + expf(-s));
    scores[p0 + tid] = s;
  }
}

}  // namespace

int embed_ln_types_launch(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type_tab,
                          int type_rows, const float* g, const float* b, float eps, int tokens, int seq, int hidden, int vocab,
                          float* x32, _Float16* x16, hipStream_t stream) {
#define CRS_EMBT(PL) hipLaunchKernelGGL((embed_ln_types_kernel<PL>), dim3((tokens + 3) / 4), dim3(256), 0, stream, ids, type_ids, \
                                       word, pos, type_tab, type_rows, g, b, eps, tokens, seq, hidden, vocab, x32, x16)
#define CRS_EMBT2(P2) hipLaunchKernelGGL((embed_ln2_types_kernel<P2>), dim3((tokens + 3) / 4), dim3(256), 0, stream, ids, type_ids, \
                                        word, pos, type_tab, type_rows, g, b, eps, tokens, seq, hidden, vocab, x32, x16)
  // the same form per hidden size as embed_ln_launch (enc_misc.hip): the sums meet in the same order
  if (hidden == 384) CRS_EMBT2(3); else if (hidden == 768) CRS_EMBT2(6); else if (hidden <= 64) CRS_EMBT(1); else CRS_EMBT(16);
#undef CRS_EMBT2
#undef CRS_EMBT
  return (int)hipGetLastError();
}

int pair_head_launch(const float* hidden32, int batch, int seq, int hidden, const float* w_pool, const float* b_pool,
                     const float* w_cls, const float* b_cls, int activation, float* scores, float* pooled_out,
                     hipStream_t stream) {
  if (batch <= 0 || hidden <= 0 || hidden > 1024 || hidden % 64) return -1;
  const dim3 grid((batch + kPairGroup - 1) / kPairGroup);
  const size_t lds = (size_t)kPairGroup * hidden * sizeof(float);
  if (hidden % 128 == 0)
    hipLaunchKernelGGL((pair_head_kernel<2>), grid, dim3(256), lds, stream, hidden32, batch, seq, hidden, w_pool, b_pool, w_cls,
                       b_cls, activation, scores, pooled_out);
  else
    hipLaunchKernelGGL((pair_head_kernel<1>), grid, dim3(256), lds, stream, hidden32, batch, seq, hidden, w_pool, b_pool, w_cls,
                       b_cls, activation, scores, pooled_out);
  return (int)hipGetLastError();
}

}  // namespace crs
