// slab_row.h -- one fp32 vector -> one slab row (+ scale, + fp32 shadow row, + the row-error maximum) of a cosine, inner-product
// or squared-L2 store.
//
// The ONE definition of how a row is stored; slab_rows_kernel (row_build.hip) is its only caller, for the append (dr = row0 + r),
// the scatter update (dr = rows[r]) and the rescale (dr = r, src = the row's own shadow row): an updated or rescaled row therefore
// equals the same vector appended, bit for bit.
//
// The head computes the row's values v (sdim = dim of them, dim + 1 for l2):
//   cosine  v = x / max(|x|_2, 1e-12), a division per element; |x|_2^2 is the lane's strided fmaf chain, then the xor butterfly
//   ip      v = x * mul, mul an exact power of two (1/R, or 2^-j in the rescale); NOT normalised
//   l2      likewise (mul = 1/(2R)), and one more coordinate t = fl(sum v_i^2) summed in that same fixed order: a power of two scales
//           every term and every partial sum of that order exactly, so a rescaled row equals the same vector stored under the new R,
//           t included
// The tail is the same for every space: the shadow row (stride sdim) receives v, the slab row its fp16 / int8 image zero padded to
// pdim, scales[dr] the int8 scale max|v| / 127, and row_err_max is raised over all sdim coordinates.  src may be the shadow row
// itself: a lane reads only the elements it writes, and reads them all first.
// One wave64 per row; rows are <= 1024 elements so a lane owns <= 16 strided elements.
#pragma once
#include "../../include/crs_hip.h"
#include "tail_steps.h"

namespace crs {
namespace {

template <bool I8, int SPACE>
__device__ __forceinline__ void slab_store_row(const float* src, int dim, float mul, int pdim, void* __restrict__ slab,
                                               float* __restrict__ scales, float* shadow, int64_t dr,
                                               float* __restrict__ row_err_max, int lane) {
  const int sdim = dim + (SPACE == CRS_SPACE_L2 ? 1 : 0);
  float v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {      // nothing but the loads under the lane's predicate: all of them are in flight together
    const int c = lane + 64 * u;
    v[u] = c < dim ? src[c] : 0.f;
  }
  float ss = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    if (SPACE != CRS_SPACE_COSINE) v[u] *= mul;      // exact; slots past dim stay +0
    ss = fmaf(v[u], v[u], ss);
  }
  if (SPACE == CRS_SPACE_COSINE) {
    const float den = fmaxf(sqrtf(wsum(ss)), 1e-12f);
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (lane + 64 * u < dim) v[u] = v[u] / den;
  }
  if (SPACE == CRS_SPACE_L2) {      // element `dim` is t; lane dim % 64 owns it in slot dim / 64
    const float t = wsum(ss);
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (lane + 64 * u == dim) v[u] = t;
  }
  float err2 = 0.f;
  if (I8) {
    float amax = 0.f;
#pragma unroll
    for (int u = 0; u < 16; ++u) amax = fmaxf(amax, fabsf(v[u]));
    amax = wmax(amax);
    const float sc = amax / 127.0f;
    const float safe = sc > 0.f ? sc : 1.0f;
    int8_t* dst = reinterpret_cast<int8_t*>(slab) + dr * pdim;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = lane + 64 * u;
      if (c >= pdim) continue;
      const float x = v[u];
      float qv = rintf(x / safe);
      qv = fminf(fmaxf(qv, -127.f), 127.f);
      dst[c] = (int8_t)qv;
      if (shadow && c < sdim) shadow[dr * sdim + c] = x;
      const float d = x - qv * sc;            // the row as the scan sees it: int8 * scale
      err2 = fmaf(d, d, err2);
    }
    if (lane == 0) scales[dr] = sc;
  } else {
    _Float16* dst = reinterpret_cast<_Float16*>(slab) + dr * pdim;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int c = lane + 64 * u;
      if (c >= pdim) continue;
      const float x = v[u];
      const _Float16 h = (_Float16)x;
      dst[c] = h;
      if (shadow && c < sdim) shadow[dr * sdim + c] = x;
      const float d = x - (float)h;
      err2 = fmaf(d, d, err2);
    }
  }
  // |stored row - fp32 row|_2, maximum over the shard's rows: the row term of the exactness certificate (exact.hip).
  // Non-negative floats order like their bit patterns; the plain read first keeps the atomics to the few rows that raise it.
  if (row_err_max) {
    const float err = sqrtf(wsum(err2)) * 1.0001f;
    if (lane == 0) {
      int* p = reinterpret_cast<int*>(row_err_max);
      if (__float_as_int(err) > __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p, __float_as_int(err));
    }
  }
}

}  // namespace
}  // namespace crs
