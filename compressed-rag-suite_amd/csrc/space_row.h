// space_row.h -- one fp32 vector -> one slab row of an inner-product or squared-L2 store.  The twin of slab_row.h
// for hnsw:space 'ip' / 'l2'; slab_row.h and the cosine path are not touched.
//
// The ONE definition of how such a row is stored.  Every caller hands it `dim` source floats and a multiplier that is an exact
// power of two:
//   crs_slab_append_space_f32      src = the caller's vector x,          mul = 1/R (ip) or 1/(2R) (l2),  dr = row0 + r
//   crs_slab_write_rows_space_f32  likewise,                                                             dr = rows[r]
//   crs_slab_rescale_space         src = the row's own fp32 shadow row,  mul = 2^-j (R grew to R 2^j),   dr = r
// The row is v = src * mul (exact); it is NOT normalised.  SPACE == L2 appends one coordinate t = fl(sum v_i^2), summed in one
// fixed order (the lane's strided fmaf chain, then the xor butterfly): a power of two scales every term and every partial sum of
// that order exactly, so a rescaled row equals the same vector stored under the new R bit for bit, t included.  The shadow row
// (stride sdim = dim, or dim + 1 for l2) receives v (and t), the slab row their fp16 / int8 image, zero padded to pdim, and
// row_err_max is raised over all sdim coordinates.  src may be the shadow row itself (the rescale): a lane reads only the
// elements it writes, and reads them first.
// One wave64 per row; rows are <= 1024 elements so a lane owns <= 16 strided elements.
#pragma once
#include "tail_steps.h"

namespace crs {
namespace {

constexpr int kSpaceIP = 1;    // CRS_SPACE_IP
constexpr int kSpaceL2 = 2;    // CRS_SPACE_L2

template <bool I8, int SPACE>
__device__ __forceinline__ void slab_store_row_space(const float* src, int dim, float mul, int pdim, void* __restrict__ slab,
                                                     float* __restrict__ scales, float* shadow, int64_t dr,
                                                     float* __restrict__ row_err_max, int lane) {
  const int sdim = dim + (SPACE == kSpaceL2 ? 1 : 0);
  float v[16];
  float tt = 0.f, amax = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int c = lane + 64 * u;
    v[u] = c < dim ? src[c] * mul : 0.f;
    tt = fmaf(v[u], v[u], tt);
    amax = fmaxf(amax, fabsf(v[u]));
  }
  const float t = SPACE == kSpaceL2 ? wsum(tt) : 0.f;
  // element `dim` is t (l2); lane dim % 64 owns it in slot dim / 64
  if (SPACE == kSpaceL2) {
#pragma unroll
    for (int u = 0; u < 16; ++u)
      if (lane + 64 * u == dim) v[u] = t;
    amax = fmaxf(amax, t);
  }
  float err2 = 0.f;
  if (I8) {
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
  // as slab_row.h: |stored row - fp32 row|_2, maximum over the shard's rows (the row term of the exactness certificate)
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
