// mmr.hip -- greedy maximal-marginal-relevance ordering of retrieved lists on the device (gfx950): crs_mmr_order.
//
// The diversity step of the reference (rag/retrieval.py:219-277, ContextRetriever._apply_diversity here) re-orders the <= 64
// chunks of one query: position 0 first, then in every round the pending candidate with the largest
//     value = lam * rel - (1 - lam) * closest,      closest = max(0, max over the chosen of cos(candidate, chosen)),
// ties to the lowest position.  The chunks' vectors are rows of the shard's fp32 shadow, so the whole step is one launch that
// reads them in place: one 256-thread workgroup per query, three phases.
//
//   1. Gather + Gram.  G = X X^T of the list's rows (count x count, fp32 products, fp32 accumulation), accumulated over dim in
//      chunks of kKC columns staged in LDS (64 rows x 128 columns: 33 KB whatever dim is).  The 64 x 64 matrix is cut over a
//      16 x 16 thread grid: thread (ti, tj) owns G[ti + 16 u][tj + 16 v], u, v < ceil(count / 16) -- a 1 x 1 .. 4 x 4 register tile,
//      rows read from LDS as 16-byte groups (row pitch 132 floats: the 16 rows of a wave's read fall in 16 distinct slots).
//      A shadow row starts wherever row x 4 dim bytes falls: scalar head up to the 16-byte boundary, 16-byte body, scalar tail
//      (as mutate.hip's copy_row_f32).
//   2. Cosines.  norm_i = sqrt(G_ii); C_ij = G_ij / (norm_i norm_j) in fp32, 0 when either norm is 0 (never NaN from a zero row).
//   3. Selection by wave 0, lane c owning candidate c: closest = max(closest, C[c][newest]), the value in fp64 with closest
//      widened (the host's arithmetic, product and difference rounded separately), then a wave arg-max on (value desc, position asc).
//      A value that is NaN ranks as -inf, so the output is a permutation whatever rel holds.
//
// A row id outside [0, n_rows) is never dereferenced: that entry is a zero vector (cos 0 to everything).  counts are clamped to
// [0, m_max].  No scratch, no atomics, no workgroup depends on another.  The values are fp64 and the keys are positions, so the
// tail's float `before` does not fit here; the same rule (larger first, then lower index) is written out in argmax_step.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

constexpr int kThreads = 256;
constexpr int kM = CRS_MAX_K;        // longest list
constexpr int kKC = 128;             // columns per staged chunk
constexpr int kPitch = kKC + 4;      // floats per staged row: 528 bytes, a multiple of 16 that is no multiple of 256
constexpr int kGP = kM + 1;          // Gram row pitch (column reads of the selection fall on distinct banks)
static_assert(kM == 64, "one lane per candidate, 16 x 16 threads x 4 x 4 tiles");

// Columns [c0, c0 + n) of the list's rows -> sh_x[r][0, n), zero up to the next multiple of 4; rows that are past the list or
// carry no valid id are zero.  Half a wave per row: lanes 0..31 of the half move the 16-byte body, lanes 0..2 the head and 4..6
// the tail, 8..10 the zero padding.
__device__ __forceinline__ void stage_chunk(const float* __restrict__ vecs, int dim, const int64_t* sh_row, int count, int rows_pad,
                                            int c0, int n, float* sh_x, int wave, int lane) {
  const int half = lane >> 5, hl = lane & 31;
  const int n4 = (n + 3) & ~3;
  for (int r = wave * 2 + half; r < rows_pad; r += 8) {
    float* dst = sh_x + r * kPitch;
    const int64_t id = r < count ? sh_row[r] : (int64_t)-1;
    if (id < 0) {
      if (4 * hl < n4) *reinterpret_cast<f32x4*>(dst + 4 * hl) = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const float* src = vecs + (size_t)id * dim + c0;
    int head = (int)(((16 - (reinterpret_cast<uintptr_t>(src) & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int body = (n - head) >> 2;
    if (hl < body) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(src + head + 4 * hl);
      float* d = dst + head + 4 * hl;
      if (head == 0) {
        *reinterpret_cast<f32x4*>(d) = v;
      } else {
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
    if (hl < head) dst[hl] = src[hl];
    const int done = head + 4 * body;
    if (hl >= 4 && hl < 4 + (n - done)) dst[done + hl - 4] = src[done + hl - 4];
    if (hl >= 8 && hl < 8 + (n4 - n)) dst[n + hl - 8] = 0.f;
  }
}

// acc[u][v] += sum over the chunk's columns of x[ti + 16 u][c] x[tj + 16 v][c]
template <int NU>
__device__ __forceinline__ void gram_chunk(const float* sh_x, int n, int ti, int tj, float (&acc)[4][4]) {
  const int steps = (n + 3) >> 2;
  for (int k = 0; k < steps; ++k) {
    f32x4 a[NU], b[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      a[u] = *reinterpret_cast<const f32x4*>(sh_x + (ti + 16 * u) * kPitch + 4 * k);
      b[u] = *reinterpret_cast<const f32x4*>(sh_x + (tj + 16 * u) * kPitch + 4 * k);
    }
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int v = 0; v < NU; ++v) {
        float s = acc[u][v];
        s = fmaf(a[u].x, b[v].x, s);
        s = fmaf(a[u].y, b[v].y, s);
        s = fmaf(a[u].z, b[v].z, s);
        s = fmaf(a[u].w, b[v].w, s);
        acc[u][v] = s;
      }
  }
}

// one butterfly step of the arg-max: keep the larger value, the lower position among equals
__device__ __forceinline__ void argmax_step(double& v, int& p, int offset) {
  const double v2 = __shfl_xor(v, offset);
  const int p2 = __shfl_xor(p, offset);
  if (v2 > v || (v2 == v && p2 < p)) { v = v2; p = p2; }
}

__global__ __launch_bounds__(kThreads) void mmr_order_kernel(const float* __restrict__ vecs, int64_t n_rows, int dim,
                                                            const int64_t* __restrict__ rows, const double* __restrict__ rel,
                                                            const int* __restrict__ counts, int m_max, double lam,
                                                            int* __restrict__ order) {
  __shared__ __attribute__((aligned(16))) float sh_x[kM * kPitch];
  __shared__ float sh_g[kM * kGP];
  __shared__ float sh_norm[kM];
  __shared__ int64_t sh_row[kM];

  const int q = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int count = counts[q];
  count = count < 0 ? 0 : (count > m_max ? m_max : count);
  count = __builtin_amdgcn_readfirstlane(count);
  int* out = order + (size_t)q * m_max;

  if (count <= 2) {                     // nothing to choose: position 0 first, the other one behind it
    if (tid < m_max) out[tid] = tid < count ? tid : -1;
    return;
  }

  if (tid < kM) {
    int64_t id = -1;
    if (tid < count) {
      id = rows[(size_t)q * m_max + tid];
      if (id < 0 || id >= n_rows) id = -1;           // a poisoned id never becomes an address
    }
    sh_row[tid] = id;
  }
  __syncthreads();

  // ---- 1. gather + Gram ----
  const int nu = (count + 15) >> 4;                  // 1 .. 4 (uniform)
  const int ti = tid >> 4, tj = tid & 15;
  float acc[4][4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v) acc[u][v] = 0.f;
  for (int c0 = 0; c0 < dim; c0 += kKC) {
    const int n = dim - c0 < kKC ? dim - c0 : kKC;
    if (c0 > 0) __syncthreads();                     // the previous chunk has been read
    stage_chunk(vecs, dim, sh_row, count, nu * 16, c0, n, sh_x, wave, lane);
    __syncthreads();
    switch (nu) {
      case 1: gram_chunk<1>(sh_x, n, ti, tj, acc); break;
      case 2: gram_chunk<2>(sh_x, n, ti, tj, acc); break;
      case 3: gram_chunk<3>(sh_x, n, ti, tj, acc); break;
      default: gram_chunk<4>(sh_x, n, ti, tj, acc); break;
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int v = 0; v < 4; ++v)
      if (u < nu && v < nu) sh_g[(ti + 16 * u) * kGP + tj + 16 * v] = acc[u][v];
  __syncthreads();

  // ---- 2. cosines ----
  if (tid < count) sh_norm[tid] = sqrtf(sh_g[tid * kGP + tid]);
  __syncthreads();
  for (int e = tid; e < count * count; e += kThreads) {
    const int i = e / count, j = e - i * count;
    const float ni = sh_norm[i], nj = sh_norm[j];
    const float g = sh_g[i * kGP + j];
    sh_g[i * kGP + j] = (ni > 0.f && nj > 0.f) ? g / (ni * nj) : 0.f;
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- 3. greedy selection: lane c owns candidate c ----
  const bool mine = lane < count;
  const double r = mine ? rel[(size_t)q * m_max + lane] : 0.0;
  const double w = 1.0 - lam;
  float closest = 0.f;
  bool pending = mine && lane != 0;
  int newest = 0, chosen = mine ? 0 : -1;            // lane p: the position chosen in round p
  for (int round = 1; round < count; ++round) {
    double value = -__builtin_huge_val();
    if (pending) {
      closest = fmaxf(closest, sh_g[lane * kGP + newest]);
      // lam * rel - (1 - lam) * closest as the host evaluates it: two roundings, no contraction into an fma
      value = __dsub_rn(__dmul_rn(lam, r), __dmul_rn(w, (double)closest));
      if (!(value == value)) value = -__builtin_huge_val();
    }
    int pos = pending ? lane : kM;                   // lanes that are not pending lose every tie
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) argmax_step(value, pos, o);
    newest = __builtin_amdgcn_readfirstlane(pos);    // < count: at least one lane is pending in every round
    if (lane == round) chosen = newest;
    if (lane == newest) pending = false;
  }
  if (lane < m_max) out[lane] = chosen;
}

}  // namespace

int mmr_order_launch(const float* vecs, int64_t n_rows, int dim, const int64_t* rows, const double* rel, const int* counts, int nq,
                     int m_max, double lam, int* order, hipStream_t stream) {
  hipLaunchKernelGGL(mmr_order_kernel, dim3((unsigned)nq), dim3(kThreads), 0, stream, vecs, n_rows, dim, rows, rel, counts, m_max, lam,
                     order);
  return (int)hipGetLastError();
}

}  // namespace crs
