// row_build.hip -- every way a slab row is written (gfx950, HBM-bound): one kernel template, one launcher, one argument check.
// Declared in include/crs_hip.h; DESIGN 3.3 / 3.12.
//
// A job is (where a row comes from, where it goes, what multiplies it); slab_store_row (slab_row.h) does the rest.
//   append   crs_slab_append_f32 / crs_slab_append_space_f32          src = emb[r]                   dr = row0 + r
//            crs_queries_to_f16: the fp16 cosine append without shadow, scales or row error
//            Replaces collection.add(embeddings=embeddings.tolist(), ...) (reference rag/indexing.py:114-119): no Python lists, no
//            sqlite, one pass; the query side is rag/indexing.py:156-168 flatten + ChromaDB's cosine-space normalisation.
//   scatter  crs_slab_write_rows_f32 / crs_slab_write_rows_space_f32  src = emb[r]                   dr = rows[r], skipped when outside [0, n_rows)
//   rescale  crs_slab_rescale_space (R grew to R 2^j)                 src = the row's own shadow row  dr = r
// The multiplier of ip / l2 is 1/R or 1/(2R) from the store's device scalar R (append, scatter) or 2^-j (rescale): always an exact
// power of two.  Cosine rows are normalised instead.
// One wave64 per row, 4 waves per block; rows are <= 1024 elements so a lane owns <= 16 strided elements.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"
#include "slab_row.h"

namespace crs {
namespace {

enum RowDest { kAppend, kScatter, kRescale };

struct RowJob {
  int dest;                 // RowDest
  const float* emb;         // [n, dim] (append, scatter)
  const int64_t* rows;      // [n] (scatter)
  int64_t n;                // rows of this job
  int64_t row0;             // append: first destination row
  int64_t n_rows;           // scatter: rows of the shard
  int dim;                  // the caller's dimension
  const float* norm_scale;  // ip / l2 append and scatter: the store's R
  float factor;             // rescale: 2^-j
  void* slab;
  float* scales;            // int8 rows
  float* shadow;            // may be null (never in a rescale: it is the source)
  float* row_err_max;       // may be null
  int pdim = 0;             // the padded slab row (store_rows fills it in)
};

template <bool I8, int SPACE>
__global__ __launch_bounds__(256) void slab_rows_kernel(const RowJob j) {
  const int lane = threadIdx.x & 63;
  const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= j.n) return;
  int64_t dr = j.row0 + r;
  if (j.dest == kScatter) {
    dr = j.rows[r];
    if (dr < 0 || dr >= j.n_rows) return;     // never write outside the shard, whatever the caller passed
  }
  const int sdim = j.dim + (SPACE == CRS_SPACE_L2 ? 1 : 0);
  const float* src = j.dest == kRescale ? j.shadow + dr * sdim : j.emb + r * j.dim;
  float mul = j.factor;
  if (SPACE != CRS_SPACE_COSINE && j.dest != kRescale) mul = (SPACE == CRS_SPACE_L2 ? 0.5f : 1.0f) / *j.norm_scale;
  slab_store_row<I8, SPACE>(src, j.dim, mul, j.pdim, j.slab, j.scales, j.shadow, dr, j.row_err_max, lane);
}

using RowKernel = void (*)(const RowJob);
// [rows are int8][space]
constexpr RowKernel kRowKernels[2][3] = {
    {slab_rows_kernel<false, CRS_SPACE_COSINE>, slab_rows_kernel<false, CRS_SPACE_IP>, slab_rows_kernel<false, CRS_SPACE_L2>},
    {slab_rows_kernel<true, CRS_SPACE_COSINE>, slab_rows_kernel<true, CRS_SPACE_IP>, slab_rows_kernel<true, CRS_SPACE_L2>}};

// The one argument check and launch behind every entry point below.  `first_space` is the lowest space the entry point accepts
// (the *_space functions reject cosine, which has entry points of its own); `f16_rows` writes fp16 rows under either slab type's
// padding (queries).
int store_rows(const char* what, RowJob j, int space, int first_space, int slab_type, void* stream, bool f16_rows = false) {
  if (space < first_space || space > CRS_SPACE_L2) return set_error(CRS_EINVAL, "bad space (CRS_SPACE_IP or CRS_SPACE_L2)");
  const int sdim = crs_space_row_dim(j.dim, space);      // 1 .. 1024: l2 stores one more coordinate than the caller's dim
  if (j.n < 0 || sdim <= 0 || sdim > 1024 || j.row0 < 0 || j.n_rows < 0) return set_error(CRS_EINVAL, "bad row count / dim / row0 / n_rows");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return set_error(CRS_EINVAL, "bad slab_type");
  if (j.n == 0 || (j.dest == kRescale && j.factor == 1.0f)) return CRS_OK;      // no rows, or a rescale by 2^0
  const bool no_src = j.dest == kRescale ? !j.shadow : !j.emb || (space != CRS_SPACE_COSINE && !j.norm_scale);
  if (no_src || !j.slab || (j.dest == kScatter && !j.rows))
    return set_error(CRS_EINVAL, "null pointer (emb, rows, norm_scale or slab; the rescale reads the fp32 shadow)");
  const bool i8 = slab_type == CRS_SLAB_I8 && !f16_rows;
  if (i8 && !j.scales) return set_error(CRS_EINVAL, "int8 slab needs scales");
  j.pdim = crs_row_elems(sdim, slab_type);
  hipLaunchKernelGGL(kRowKernels[i8][space], dim3((unsigned)((j.n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, j);
  return launch_status(what);
}

}  // namespace
}  // namespace crs

extern "C" {

using crs::RowJob;
using crs::store_rows;

int crs_slab_append_f32(const float* emb_dev, int64_t n, int dim, int slab_type, void* slab_dev, float* scales_dev, float* shadow_f32_dev,
                        int64_t row0, float* row_err_max_dev, void* stream) {
  const RowJob j{crs::kAppend, emb_dev, nullptr, n, row0, 0, dim, nullptr, 1.0f, slab_dev, scales_dev, shadow_f32_dev, row_err_max_dev};
  return store_rows("slab_append", j, CRS_SPACE_COSINE, CRS_SPACE_COSINE, slab_type, stream);
}

// the fp16 cosine row, padded like the rows of the slab it will be searched against
int crs_queries_to_f16(const float* q_dev, int nq, int dim, int slab_type, void* q16_dev, void* stream) {
  const RowJob j{crs::kAppend, q_dev, nullptr, nq, 0, 0, dim, nullptr, 1.0f, q16_dev, nullptr, nullptr, nullptr};
  return store_rows("queries_to_f16", j, CRS_SPACE_COSINE, CRS_SPACE_COSINE, slab_type, stream, true);
}

int crs_slab_write_rows_f32(const float* emb_dev, const int64_t* rows_dev, int64_t m, int dim, int slab_type, void* slab_dev,
                            float* scales_dev, float* shadow_f32_dev, int64_t n_rows, float* row_err_max_dev, void* stream) {
  const RowJob j{crs::kScatter, emb_dev, rows_dev, m, 0, n_rows, dim, nullptr, 1.0f, slab_dev, scales_dev, shadow_f32_dev, row_err_max_dev};
  return store_rows("slab_write_rows", j, CRS_SPACE_COSINE, CRS_SPACE_COSINE, slab_type, stream);
}

int crs_slab_append_space_f32(const float* emb_dev, int64_t n, int dim, int space, int slab_type, const float* norm_scale_dev,
                              void* slab_dev, float* scales_dev, float* shadow_f32_dev, int64_t row0, float* row_err_max_dev,
                              void* stream) {
  const RowJob j{crs::kAppend, emb_dev, nullptr, n, row0, 0, dim, norm_scale_dev, 1.0f, slab_dev, scales_dev, shadow_f32_dev, row_err_max_dev};
  return store_rows("slab_append_space", j, space, CRS_SPACE_IP, slab_type, stream);
}

int crs_slab_write_rows_space_f32(const float* emb_dev, const int64_t* rows_dev, int64_t m, int dim, int space, int slab_type,
                                  const float* norm_scale_dev, void* slab_dev, float* scales_dev, float* shadow_f32_dev, int64_t n_rows,
                                  float* row_err_max_dev, void* stream) {
  const RowJob j{crs::kScatter, emb_dev, rows_dev, m, 0, n_rows, dim, norm_scale_dev, 1.0f, slab_dev, scales_dev, shadow_f32_dev, row_err_max_dev};
  return store_rows("slab_write_rows_space", j, space, CRS_SPACE_IP, slab_type, stream);
}

int crs_slab_rescale_space(int64_t n_rows, int dim, int space, int slab_type, int shift, void* slab_dev, float* scales_dev,
                           float* shadow_f32_dev, float* row_err_max_dev, void* stream) {
  if (shift < 0 || shift > 126) return crs::set_error(CRS_EINVAL, "shift must be in 0..126");
  const RowJob j{crs::kRescale, nullptr, nullptr, n_rows, 0, 0, dim, nullptr, __builtin_ldexpf(1.0f, -shift), slab_dev, scales_dev,
                 shadow_f32_dev, row_err_max_dev};
  return store_rows("slab_rescale_space", j, space, CRS_SPACE_IP, slab_type, stream);
}

}  // extern "C"
