// row_build_mxfp4.hip -- fp32 vectors -> rows of an MXFP4 slab (gfx950; layout: mxfp4.h).
// Declared in include/crs_hip.h: crs_slab_append_mxfp4_f32 (dr = row0 + r) and crs_slab_write_rows_mxfp4_f32 (dr = rows[r]); one
// kernel behind both, so a scattered row equals the same vector appended, bit for bit.
//
// One wave64 per row, 4 waves per block; a lane owns the strided elements lane + 64 u like the other builds, so the unit row v
// (and with it the fp32 shadow) carries the bits of the fp16 / int8 builds: v = x / max(|x|_2, 1e-12).  An MX block of 32
// elements is then the slot u of one half wave: block 2 u in lanes 0..31, block 2 u + 1 in lanes 32..63.
//
// The OCP MX rule, in integer and float arithmetic a numpy restatement reproduces bit for bit (tests/test_mxfp4_gpu.py):
//   scale byte  E = clamp(floor(log2(max|v|)) - 2 + 127, 0, 254) read from the maximum's exponent field (a subnormal maximum
//               has floor(log2) < -126, which clamps to 0 like the all-zero block)
//   element     y = |v| * 2^(127 - E) (a power of two: exact); code = the count of the rounding boundaries at or below y,
//               {0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5}, a boundary itself counted only when that lands on the even code:
//               round to nearest e2m1, ties to even, saturating at 6 (code 7); the sign bit is v's
// The row error |v - v^|_2 is summed in the lanes' strided order and written per row.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "mxfp4.h"
#include "scan.h"
#include "tail_steps.h"

namespace crs {
namespace {

struct MxRowJob {
  const float* emb;       // [n, dim]
  const int64_t* rows;    // scatter: [n] destination rows, else null
  int64_t n, row0, n_rows;
  int dim, pdim;
  uint8_t* data;
  uint8_t* scales;
  float* shadow;          // [*, dim] or null
  float* row_err;         // [*] or null
};

__device__ __forceinline__ int e2m1_code(float y) {
  return (y > 0.25f) + (y >= 0.75f) + (y > 1.25f) + (y >= 1.75f) + (y > 2.5f) + (y >= 3.5f) + (y > 5.0f);
}

__global__ __launch_bounds__(256) void mx_rows_kernel(const MxRowJob j) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= j.n) return;
  int64_t dr = j.row0 + r;
  if (j.rows) {
    dr = j.rows[r];
    if (dr < 0 || dr >= j.n_rows) return;     // never write outside the slab, whatever the caller passed
  }
  const float* src = j.emb + r * j.dim;
  float v[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int c = lane + 64 * u;
    v[u] = c < j.dim ? src[c] : 0.f;
  }
  float ss = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) ss = fmaf(v[u], v[u], ss);
  const float den = fmaxf(sqrtf(wsum(ss)), 1e-12f);
#pragma unroll
  for (int u = 0; u < 16; ++u)
    if (lane + 64 * u < j.dim) v[u] = v[u] / den;

  const int64_t tile = dr >> 4;
  const int rr = (int)(dr & 15);
  const int ksteps = j.pdim >> 7, sp = mx_scale_stride(j.pdim);
  float err2 = 0.f;
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const int c = lane + 64 * u;
    if (64 * u >= j.pdim) break;              // (uniform)
    const float x = v[u];
    float amax = fabsf(x);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));     // the half wave's block
    int E = (int)((__float_as_uint(amax) >> 23) & 0xff) - 2;                       // biased floor(log2 amax) - 2
    E = E < 0 ? 0 : E;
    const float inv = __uint_as_float((unsigned)(254 - E) << 23);                  // 2^(127 - E), E <= 253 here
    const float scale = E > 0 ? __uint_as_float((unsigned)E << 23) : __uint_as_float(0x00400000u);   // 2^(E - 127)
    const int code = e2m1_code(fabsf(x) * inv);
    const int nib = code | ((__float_as_uint(x) >> 31) << 3);
    const int other = __shfl_xor(nib, 1);
    const int b = c >> 5;                     // block of the row
    const int s = b >> 2, ml = rr + 16 * (b & 3);
    if (!(lane & 1)) j.data[(((size_t)tile * ksteps + s) * 64 + ml) * 16 + ((c & 31) >> 1)] = (uint8_t)(nib | (other << 4));
    if (!(lane & 31)) j.scales[((size_t)tile * 64 + ml) * sp + s] = (uint8_t)E;
    if (j.shadow && c < j.dim) j.shadow[dr * j.dim + c] = x;
    const float mag = (code < 4 ? 0.5f * code : code == 4 ? 2.f : code == 5 ? 3.f : code == 6 ? 4.f : 6.f) * scale;
    const float d = x - ((nib & 8) ? -mag : mag);
    err2 = fmaf(d, d, err2);
  }
  if (j.row_err) {
    const float err = sqrtf(wsum(err2));
    if (lane == 0) j.row_err[dr] = err;
  }
}

int store_rows(const char* what, MxRowJob j, void* stream) {
  if (j.n < 0 || j.dim <= 0 || j.dim > 1024 || j.row0 < 0 || j.n_rows < 0) return set_error(CRS_EINVAL, "bad row count / dim / row0 / n_rows");
  if (j.n == 0) return CRS_OK;
  if (!j.emb || !j.data || !j.scales) return set_error(CRS_EINVAL, "null pointer (emb, slab data or slab scales)");
  j.pdim = mx_pdim(j.dim);
  hipLaunchKernelGGL(mx_rows_kernel, dim3((unsigned)((j.n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, j);
  return launch_status(what);
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_mxfp4_row_bytes(int dim) { return dim >= 1 && dim <= 1024 ? crs::mx_row_bytes(crs::mx_pdim(dim)) : 0; }

int crs_mxfp4_slab_bytes(int64_t rows, int dim, size_t* data_bytes, size_t* scale_bytes) {
  if (rows < 0 || dim < 1 || dim > 1024 || !data_bytes || !scale_bytes) return crs::set_error(CRS_EINVAL, "bad rows / dim / null pointer");
  *data_bytes = crs::mx_data_bytes(rows, crs::mx_pdim(dim));
  *scale_bytes = crs::mx_scale_bytes(rows, crs::mx_pdim(dim));
  return CRS_OK;
}

int crs_slab_append_mxfp4_f32(const float* emb_dev, int64_t n, int dim, void* data_dev, void* scales_dev, float* shadow_f32_dev,
                              int64_t row0, float* row_err_dev, void* stream) {
  const crs::MxRowJob j{emb_dev, nullptr, n, row0, 0, dim, 0, (uint8_t*)data_dev, (uint8_t*)scales_dev, shadow_f32_dev, row_err_dev};
  return crs::store_rows("slab_append_mxfp4", j, stream);
}

int crs_slab_write_rows_mxfp4_f32(const float* emb_dev, const int64_t* rows_dev, int64_t m, int dim, void* data_dev, void* scales_dev,
                                  float* shadow_f32_dev, int64_t n_rows, float* row_err_dev, void* stream) {
  if (m > 0 && !rows_dev) return crs::set_error(CRS_EINVAL, "null pointer (rows)");
  const crs::MxRowJob j{emb_dev, rows_dev, m, 0, n_rows, dim, 0, (uint8_t*)data_dev, (uint8_t*)scales_dev, shadow_f32_dev, row_err_dev};
  return crs::store_rows("slab_write_rows_mxfp4", j, stream);
}

}  // extern "C"
