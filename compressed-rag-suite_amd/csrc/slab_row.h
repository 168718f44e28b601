// slab_row.h -- one fp32 embedding row -> one slab row (+ scale, + fp32 shadow row, + the row-error maximum).
//
// The ONE definition of how a row is stored.  crs_slab_append_f32 (convert.hip) calls it with dr = row0 + r,
// crs_slab_write_rows_f32 (mutate.hip) with dr = rows[r]: an updated row therefore equals the same vector appended, bit for bit.
// One wave64 per row; rows are <= 1024 elements so a lane owns <= 16 strided elements.
#pragma once
#include "tail_steps.h"

namespace crs {
namespace {

template <bool I8>
__device__ __forceinline__ void slab_store_row(const float* __restrict__ src, int dim, int pdim, void* __restrict__ slab,
                                               float* __restrict__ scales, float* __restrict__ shadow, int64_t dr,
                                               float* __restrict__ row_err_max, int lane) {
  float ss = 0.f;
  for (int c = lane; c < dim; c += 64) {
    const float x = src[c];
    ss += x * x;
  }
  ss = wsum(ss);
  const float inv_den = fmaxf(sqrtf(ss), 1e-12f);
  float err2 = 0.f;
  if (I8) {
    float amax = 0.f;
    for (int c = lane; c < dim; c += 64) amax = fmaxf(amax, fabsf(src[c] / inv_den));
    amax = wmax(amax);
    const float sc = amax / 127.0f;
    const float safe = sc > 0.f ? sc : 1.0f;
    int8_t* dst = reinterpret_cast<int8_t*>(slab) + dr * pdim;
    for (int c = lane; c < pdim; c += 64) {
      float x = 0.f;
      if (c < dim) x = src[c] / inv_den;
      float qv = rintf(x / safe);
      qv = fminf(fmaxf(qv, -127.f), 127.f);
      dst[c] = (int8_t)qv;
      if (shadow && c < dim) shadow[dr * dim + c] = x;
      const float d = x - qv * sc;            // the row as the scan sees it: int8 * scale
      err2 = fmaf(d, d, err2);
    }
    if (lane == 0) scales[dr] = sc;
  } else {
    _Float16* dst = reinterpret_cast<_Float16*>(slab) + dr * pdim;
    for (int c = lane; c < pdim; c += 64) {
      float x = 0.f;
      if (c < dim) x = src[c] / inv_den;
      const _Float16 h = (_Float16)x;
      dst[c] = h;
      if (shadow && c < dim) shadow[dr * dim + c] = x;
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
