// space.hip -- inner-product and squared-L2 spaces on the cosine scan (gfx950, HBM-bound).  Declared in include/crs_hip.h
// (additive to ABI 3); DESIGN 3.12 holds the transform.
//
// Every scan family computes <fp16 query row, slab row>; it is a cosine only because both sides were normalised first.  A store
// with hnsw:space 'ip' / 'l2' keeps one scale R = 2^e >= every row norm it has seen (a device fp32 the kernels read, so a captured
// graph stays valid when it grows) and transforms rows on the way in, queries on the way in and distances on the way out:
//   rows_norm_max     fp32 [n, d] -> the largest |x|_2, atomicMax on the bit pattern (non-negative floats order like their bits)
//   append / write    x -> u = x / R (ip) or (v, t) = (x / 2R, fl(sum v^2)) (l2): jobs of row_build.hip, rows by slab_store_row
//   rescale           R grew by 2^j: shadow rows times 2^-j (t: recomputed, = times 2^-2j), slab rows rebuilt from them (likewise)
//   queries_to_space  q -> unit fp32 [nq, d'] and fp16 [nq, pdim]: q / |q| (ip), (q / R, -1) / |.| (l2)
//   space_distances   the certified list's rows -> 1 - <q, x> (ip) or sum (q - x)^2 (l2) from the recovered x = R u / 2R v, in
//                     fp32, ordered (distance asc, row asc)
// The scan, merge, certificate and escalation kernels run unchanged on d' = d (ip) or d + 1 (l2).
// One wave64 per row; rows are <= 1024 elements so a lane owns <= 16 strided elements.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

constexpr int kDistMaxK = CRS_MAX_K_CERT;

// grid: one wave per row, 4 waves per block.  A norm that is not finite leaves +inf in norm_max and 1 in flag.
__global__ __launch_bounds__(256) void rows_norm_max_kernel(const float* __restrict__ emb, int64_t n, int dim, float* __restrict__ norm_max,
                                                           int* __restrict__ flag) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const float* src = emb + r * dim;
  float ss = 0.f;
  for (int c = lane; c < dim; c += 64) ss = fmaf(src[c], src[c], ss);
  float nrm = sqrtf(wsum(ss));
  const bool bad = !(nrm < __builtin_huge_valf());       // inf or NaN
  if (bad) nrm = __builtin_huge_valf();
  if (lane == 0) {
    int* p = reinterpret_cast<int*>(norm_max);
    if (__float_as_int(nrm) > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, __float_as_int(nrm));
    if (bad && flag) atomicOr(flag, 1);
  }
}

// one wave per query: unit fp32 [nq, sdim] and fp16 [nq, pdim], zero padded
template <int SPACE>
__global__ __launch_bounds__(256) void queries_to_space_kernel(const float* __restrict__ q, int nq, int dim, int pdim,
                                                              const float* __restrict__ norm_scale, float* __restrict__ out32,
                                                              _Float16* __restrict__ out16) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= nq) return;
  const int sdim = dim + (SPACE == CRS_SPACE_L2 ? 1 : 0);
  const float mul = SPACE == CRS_SPACE_L2 ? 1.0f / *norm_scale : 1.0f;     // l2: p = q / R (exact)
  const float* src = q + (size_t)r * dim;
  float ss = 0.f;
  for (int c = lane; c < dim; c += 64) {
    const float x = src[c] * mul;
    ss = fmaf(x, x, ss);
  }
  ss = wsum(ss);
  if (SPACE == CRS_SPACE_L2) ss += 1.0f;                                    // the appended -1
  const float den = fmaxf(sqrtf(ss), 1e-12f);
  for (int c = lane; c < pdim; c += 64) {
    float x = 0.f;
    if (c < dim) x = (src[c] * mul) / den;
    else if (SPACE == CRS_SPACE_L2 && c == dim) x = -1.0f / den;
    if (c < sdim) out32[(size_t)r * sdim + c] = x;
    out16[(size_t)r * pdim + c] = (_Float16)x;
  }
}

// One 256-thread workgroup per query.  Wave w computes the distances of slots w, w + 4, ... straight from the recovered vectors
// (x_i = shadow_i * back, back = R or 2R: exact), the distances meet in LDS and every slot ranks itself by counting on
// (distance asc, row asc); a slot without a row of this view (id < 0 or outside [id_base, id_base + n_rows)) leaves as (+inf, -1),
// behind the others.
template <int SPACE>
__global__ __launch_bounds__(256) void space_distances_kernel(const float* __restrict__ q, int dim, const float* __restrict__ shadow,
                                                             int64_t n_rows, int64_t id_base, const float* __restrict__ norm_scale,
                                                             const int64_t* __restrict__ ids, int k, float* __restrict__ out_d,
                                                             int64_t* __restrict__ out_i) {
  __shared__ float sh_d[kDistMaxK];
  __shared__ int64_t sh_i[kDistMaxK];
  const int qi = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int sdim = dim + (SPACE == CRS_SPACE_L2 ? 1 : 0);
  const float back = (SPACE == CRS_SPACE_L2 ? 2.0f : 1.0f) * *norm_scale;
  const float* a = q + (size_t)qi * dim;
  for (int c = wave; c < k; c += 4) {
    const int64_t id = ids[(size_t)qi * k + c];
    const int64_t row = id - id_base;
    const bool ok = id >= 0 && row >= 0 && row < n_rows;                // wave-uniform
    float acc = 0.f;
    if (ok) {
      const float* b = shadow + (size_t)row * sdim;
      for (int e = lane; e < dim; e += 64) {
        const float x = b[e] * back;
        if (SPACE == CRS_SPACE_L2) { const float df = a[e] - x; acc = fmaf(df, df, acc); }
        else acc = fmaf(a[e], x, acc);
      }
      acc = wsum(acc);
    }
    if (lane == 0) {
      sh_d[c] = ok ? (SPACE == CRS_SPACE_L2 ? acc : 1.0f - acc) : __builtin_huge_valf();
      sh_i[c] = ok ? id : (int64_t)-1;
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < k; c += 256) {
    const float dc = sh_d[c];
    const int64_t ic = sh_i[c];
    int rank = 0;
    for (int o = 0; o < k; ++o) {
      const float d2 = sh_d[o];
      const int64_t i2 = sh_i[o];
      bool first;                                                       // does slot o precede slot c?
      if (i2 < 0) first = ic < 0 && o < c;
      else if (ic < 0) first = true;
      else first = d2 < dc || (d2 == dc && (i2 < ic || (i2 == ic && o < c)));
      rank += first ? 1 : 0;
    }
    out_d[(size_t)qi * k + rank] = dc;
    out_i[(size_t)qi * k + rank] = ic;
  }
}

bool bad_space(int space) { return space != CRS_SPACE_IP && space != CRS_SPACE_L2; }
bool bad_slab(int slab_type) { return slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8; }
// the caller's dimension: 1 .. 1024 (ip), 1 .. 1023 (l2: the stored row has one more coordinate)
bool bad_dim(int dim, int space) { return dim <= 0 || dim + (space == CRS_SPACE_L2 ? 1 : 0) > 1024; }

}  // namespace
}  // namespace crs

extern "C" {

int crs_space_row_dim(int dim, int space) {
  if (dim <= 0) return 0;
  if (space == CRS_SPACE_COSINE || space == CRS_SPACE_IP) return dim;
  return space == CRS_SPACE_L2 ? dim + 1 : 0;
}

int crs_rows_norm_max(const float* emb_dev, int64_t n, int dim, float* norm_max_dev, int32_t* flag_dev, void* stream) {
  if (n < 0 || dim <= 0 || dim > 1024) return crs::set_error(CRS_EINVAL, "bad n/dim");
  if (n == 0) return CRS_OK;
  if (!emb_dev || !norm_max_dev) return crs::set_error(CRS_EINVAL, "null pointer");
  hipLaunchKernelGGL(crs::rows_norm_max_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, emb_dev, n, dim,
                     norm_max_dev, flag_dev);
  return crs::launch_status("rows_norm_max");
}

int crs_queries_to_space(const float* q_dev, int nq, int dim, int space, int slab_type, const float* norm_scale_dev, float* q32_dev,
                         void* q16_dev, void* stream) {
  if (crs::bad_space(space)) return crs::set_error(CRS_EINVAL, "bad space (CRS_SPACE_IP or CRS_SPACE_L2)");
  if (nq < 0 || crs::bad_dim(dim, space)) return crs::set_error(CRS_EINVAL, "bad nq/dim");
  if (crs::bad_slab(slab_type)) return crs::set_error(CRS_EINVAL, "bad slab_type");
  if (nq == 0) return CRS_OK;
  if (!q_dev || !q32_dev || !q16_dev || !norm_scale_dev) return crs::set_error(CRS_EINVAL, "null pointer");
  const int pdim = crs_row_elems(crs_space_row_dim(dim, space), slab_type);
  const unsigned blocks = (unsigned)((nq + 3) / 4);
  if (space == CRS_SPACE_L2)
    hipLaunchKernelGGL((crs::queries_to_space_kernel<CRS_SPACE_L2>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, q_dev, nq, dim, pdim,
                       norm_scale_dev, q32_dev, reinterpret_cast<_Float16*>(q16_dev));
  else
    hipLaunchKernelGGL((crs::queries_to_space_kernel<CRS_SPACE_IP>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, q_dev, nq, dim, pdim,
                       norm_scale_dev, q32_dev, reinterpret_cast<_Float16*>(q16_dev));
  return crs::launch_status("queries_to_space");
}

int crs_space_distances(const float* q_dev, int nq, int dim, int space, const float* shadow_f32_dev, int64_t n_rows, int64_t id_base,
                        const float* norm_scale_dev, const int64_t* ids_dev, int k, float* out_dist_dev, int64_t* out_ids_dev,
                        void* stream) {
  if (crs::bad_space(space)) return crs::set_error(CRS_EINVAL, "bad space (CRS_SPACE_IP or CRS_SPACE_L2)");
  if (nq < 0 || crs::bad_dim(dim, space) || n_rows < 0) return crs::set_error(CRS_EINVAL, "bad nq/dim/n_rows");
  if (k < 1 || k > CRS_MAX_K_CERT) return crs::set_error(CRS_EINVAL, "k must be in 1..CRS_MAX_K_CERT");
  if (nq == 0) return CRS_OK;
  if (!q_dev || !shadow_f32_dev || !norm_scale_dev || !ids_dev || !out_dist_dev || !out_ids_dev)
    return crs::set_error(CRS_EINVAL, "null pointer");
  if (ids_dev == out_ids_dev) return crs::set_error(CRS_EINVAL, "out_ids must not be ids");
  if (space == CRS_SPACE_L2)
    hipLaunchKernelGGL((crs::space_distances_kernel<CRS_SPACE_L2>), dim3(nq), dim3(256), 0, (hipStream_t)stream, q_dev, dim,
                       shadow_f32_dev, n_rows, id_base, norm_scale_dev, ids_dev, k, out_dist_dev, out_ids_dev);
  else
    hipLaunchKernelGGL((crs::space_distances_kernel<CRS_SPACE_IP>), dim3(nq), dim3(256), 0, (hipStream_t)stream, q_dev, dim,
                       shadow_f32_dev, n_rows, id_base, norm_scale_dev, ids_dev, k, out_dist_dev, out_ids_dev);
  return crs::launch_status("space_distances");
}

}  // extern "C"
