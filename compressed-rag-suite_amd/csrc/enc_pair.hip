// enc_pair.hip -- the head of a sentence-PAIR classifier (cross-encoder):
//   pair_head_kernel         score = w_c . tanh(W_p h_CLS + b_p) + b_c  (BertPooler + a one-label classifier), optional sigmoid
// (the embedding with a token-type row per token is the TYPES form of enc_misc.hip's kernels)

#include "enc.h"
#include "enc_ln.h"

namespace crs {
namespace {

// One 256-thread workgroup serves kPairGroup pairs: their [CLS] rows sit in LDS (kPairGroup x H floats: 24 KB at H = 768, 32 KB at
// the largest H), and every row of W_p a wave loads is used for all of them, so W_p (H x H fp32: 2.3 MB at 768) is read once per
// group instead of once per pair.  Wave w owns the pooler's output rows w, w + 4, ...: the lanes read one row of W_p coalesced
// (VEC = 2: 8-byte column pairs, H a multiple of 128; VEC = 1 otherwise), multiply it into the kPairGroup vectors, and a wave
// reduction leaves every lane with the full dot products; tanh, and the classifier's term w_c[j] * pooled[j] is added to the
// wave's running sum of each pair.  The four waves' sums meet in LDS in a fixed order.  A pair's result does not depend on its
// place in the group or on the batch it came in: every multiply-add of a pair is written as fmaf, so that all kPairGroup
// accumulators run the same arithmetic (left to "a += b * c", the compiler fused six of them and gave the last two a separate
// multiply and add, and slots 6 and 7 of a group differed from slots 0 to 5 in the last bits;
// tests/test_row_kernels_gpu.py::test_a_pair_does_not_depend_on_its_place).
constexpr int kPairGroup = forms::kPairGroup;

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
          acc[gi] = fmaf(w2.x, h2.x, acc[gi]);
          acc[gi] = fmaf(w2.y, h2.y, acc[gi]);
        }
      } else {
        const float w1 = wr[c];
#pragma unroll
        for (int gi = 0; gi < kPairGroup; ++gi) acc[gi] = fmaf(w1, hs[gi * hidden + c], acc[gi]);
      }
    }
    const float bj = b_pool[j], wj = w_cls[j];
#pragma unroll
    for (int gi = 0; gi < kPairGroup; ++gi) {
      const float pooled = tanhf(wave_sum(acc[gi]) + bj);
      cls[gi] = fmaf(wj, pooled, cls[gi]);
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
