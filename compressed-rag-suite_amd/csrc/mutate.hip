// mutate.hip -- in-place mutation of a shard's arrays (gfx950, HBM-bound): stable compaction after a delete.  Declared in
// include/crs_hip.h (additive to ABI 3).  (The scatter update of rows is a job of row_build.hip.)
//
//   compact    : remove the sorted rows dead[0..m) and close the gaps, keeping the order of the survivors.  Destination
//                row d is filled from source row s = d + j, j = #{i : dead[i] - i <= d} (dead[i] - i, the number of
//                survivors below dead[i], is non-decreasing: one binary search per wave, then one probe per row).
//
// Ordering of the compaction.  A workgroup's destination rows are other workgroups' source rows, so nothing inside one
// launch may depend on another workgroup.  The destination is cut into windows of W rows and every window takes TWO launches on
// the stream: GATHER copies the window's source rows into the bounce buffer (reads the arrays, writes only the bounce buffer),
// SCATTER copies the bounce buffer to the window (reads only the bounce buffer, writes rows [d0, d0 + w) of the arrays).  Window
// i reads sources >= its own first row i W; windows 0 .. i - 1 wrote rows < i W.  Hence every source row is read before any launch
// that overwrites it is started, by stream order alone: no flags, no tickets, no cooperative launch, no waiting.
// Rows below dead[0] have j = 0 (source == destination): both kernels leave them alone.
//
// Byte model: every moved byte is read and written twice (array -> bounce -> array): 4 x moved bytes of HBM traffic.
// Both kernels are one wave64 per kRowsPerWave consecutive destination rows, 16 bytes per lane per access.  Slab rows are whole
// 256-byte groups and always 16-byte aligned.  A shadow row is 4 dim bytes and starts wherever row x 4 dim falls: the bounce copy
// of window [d0, ..) is placed at the same offset mod 16 as shadow row d0, so SCATTER always moves 16-byte-aligned bodies with a
// scalar head and tail; GATHER does the same for rows whose source and bounce addresses agree mod 16 (every row when dim % 4 == 0)
// and falls back to 4-byte lanes for the others (dim % 4 != 0: three rows in four).
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"
#include "tail_steps.h"   // f32x4

namespace crs {
namespace {

constexpr int kRowsPerWave = 8;
constexpr int kWavesPerBlock = 4;
constexpr int kRowsPerBlock = kRowsPerWave * kWavesPerBlock;
constexpr int64_t kMinWindowRows = 1024;
constexpr size_t kSectionAlign = 256;

// The bounce buffer of one window: four sections, each kSectionAlign-aligned (the shadow section has 16 bytes of room for
// the mod-16 placement).
struct Bounce {
  char* slab;
  char* shadow;
  float* scales;
  int64_t* rows_global;
};

struct CompactArgs {
  const int64_t* dead;
  int64_t m, n_rows;
  int64_t d0;          // first destination row of the window
  int w;               // rows in the window
  int row_bytes;       // slab row, a multiple of 256
  int dim;             // shadow row = dim floats
  char* slab;
  float* shadow;       // may be null
  float* scales;       // may be null
  int64_t* rows_global;  // may be null
  Bounce b;
};

__device__ __forceinline__ void copy_row_16(char* __restrict__ dst, const char* __restrict__ src, int bytes, int lane) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  for (int c = lane; c < (bytes >> 4); c += 64) d[c] = s[c];
}

// n floats, both pointers 4-byte aligned.  Same offset mod 16: scalar head up to the boundary, 16-byte body, scalar tail.
__device__ __forceinline__ void copy_row_f32(float* __restrict__ dst, const float* __restrict__ src, int n, int lane) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(src), b = reinterpret_cast<uintptr_t>(dst);
  if (((a ^ b) & 15) == 0) {
    int head = (int)(((16 - (a & 15)) & 15) >> 2);
    if (head > n) head = n;
    if (lane < head) dst[lane] = src[lane];
    const int body = (n - head) >> 2;
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src + head);
    f32x4* d4 = reinterpret_cast<f32x4*>(dst + head);
    for (int c = lane; c < body; c += 64) d4[c] = s4[c];
    const int done = head + 4 * body;
    if (lane < n - done) dst[done + lane] = src[done + lane];
  } else {
    for (int c = lane; c < n; c += 64) dst[c] = src[c];
  }
}

// j = #{i < m : dead[i] - i <= d}: the dead rows below the survivor that lands on destination d
__device__ __forceinline__ int64_t dead_below(const int64_t* __restrict__ dead, int64_t m, int64_t d, int64_t lo) {
  int64_t hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (dead[mid] - mid <= d) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// GATHER == true : arrays[source rows of the window] -> bounce[0, w)      (writes the bounce buffer only)
// GATHER == false: bounce[0, w) -> arrays[d0, d0 + w)                     (reads the bounce buffer only)
template <bool GATHER>
__global__ __launch_bounds__(256) void compact_window_kernel(const CompactArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r0 = (blockIdx.x * kWavesPerBlock + wave) * kRowsPerWave;   // first window row of this wave
  if (r0 >= a.w) return;
  const int r1 = min(r0 + kRowsPerWave, a.w);
  const int64_t first_dead = a.dead[0];
  if (a.d0 + r1 <= first_dead) return;       // every row of this wave stays where it is
  // the bounce copy of the shadow window sits at the offset mod 16 of shadow row d0 (scatter: aligned bodies)
  const size_t sh_row = (size_t)a.dim * 4;
  char* bshadow = a.b.shadow + ((size_t)a.d0 * sh_row & 15);
  int64_t j = 0;
  if (GATHER) j = dead_below(a.dead, a.m, a.d0 + r0, 0);
  for (int r = r0; r < r1; ++r) {
    const int64_t d = a.d0 + r;
    if (GATHER) {
      // one probe when no dead row lies between this survivor and the last; a search (not a walk: a dead block can be long) otherwise
      if (j < a.m && a.dead[j] - j <= d) j = dead_below(a.dead, a.m, d, j + 1);
      const int64_t s = d + j;
      if (j == 0 || s >= a.n_rows) continue;        // not moved / a malformed dead list: never read past the shard
      copy_row_16(a.b.slab + (size_t)r * a.row_bytes, a.slab + (size_t)s * a.row_bytes, a.row_bytes, lane);
      if (a.shadow) copy_row_f32(reinterpret_cast<float*>(bshadow + (size_t)r * sh_row), a.shadow + (size_t)s * a.dim, a.dim, lane);
      if (lane == 0) {
        if (a.scales) a.b.scales[r] = a.scales[s];
        if (a.rows_global) a.b.rows_global[r] = a.rows_global[s];
      }
    } else {
      if (d < first_dead) continue;
      copy_row_16(a.slab + (size_t)d * a.row_bytes, a.b.slab + (size_t)r * a.row_bytes, a.row_bytes, lane);
      if (a.shadow) copy_row_f32(a.shadow + (size_t)d * a.dim, reinterpret_cast<const float*>(bshadow + (size_t)r * sh_row), a.dim, lane);
      if (lane == 0) {
        if (a.scales) a.scales[d] = a.b.scales[r];
        if (a.rows_global) a.rows_global[d] = a.b.rows_global[r];
      }
    }
  }
}

size_t align_up(size_t x, size_t al) { return (x + al - 1) / al * al; }

// bytes of the four sections for a window of w rows (all four are always laid out: a caller's buffer fits every shard of a store)
size_t bounce_bytes_for(int64_t w, int row_bytes, int dim, bool has_shadow) {
  return align_up((size_t)w * row_bytes, kSectionAlign) + (has_shadow ? align_up((size_t)w * dim * 4 + 16, kSectionAlign) : 0) +
         align_up((size_t)w * 4, kSectionAlign) + align_up((size_t)w * 8, kSectionAlign);
}

int64_t window_rows(int row_bytes, int dim, bool has_shadow, size_t bounce_bytes) {
  const size_t per_row = (size_t)row_bytes + (has_shadow ? (size_t)dim * 4 : 0) + 12;
  const size_t slack = 4 * kSectionAlign + 16;
  if (bounce_bytes < slack) return 0;
  int64_t w = (int64_t)((bounce_bytes - slack) / per_row);
  if (w > (int64_t)1 << 24) w = (int64_t)1 << 24;       // keeps window row indices and the grid in int range
  w = w / kRowsPerBlock * kRowsPerBlock;
  return w >= kMinWindowRows ? w : 0;
}

}  // namespace

}  // namespace crs

extern "C" {

size_t crs_slab_compact_bounce_bytes(int dim, int slab_type, int has_shadow) {
  if (dim <= 0 || dim > 1024 || (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8)) return 0;
  const int row_bytes = crs_row_elems(dim, slab_type) * (slab_type == CRS_SLAB_I8 ? 1 : 2);
  // the smallest size whose window holds kMinWindowRows rows (window_rows rounds down to whole workgroups)
  const size_t per_row = (size_t)row_bytes + (has_shadow ? (size_t)dim * 4 : 0) + 12;
  return crs::kMinWindowRows * per_row + 4 * crs::kSectionAlign + 16;
}

int64_t crs_slab_compact_window_rows(int dim, int slab_type, int has_shadow, size_t bounce_bytes) {
  if (dim <= 0 || dim > 1024 || (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8)) return 0;
  const int row_bytes = crs_row_elems(dim, slab_type) * (slab_type == CRS_SLAB_I8 ? 1 : 2);
  return crs::window_rows(row_bytes, dim, has_shadow != 0, bounce_bytes);
}

int crs_slab_compact(const int64_t* dead_dev, int64_t m, int64_t n_rows, int64_t first_row, int dim, int slab_type, void* slab_dev,
                     float* scales_dev, float* shadow_f32_dev, int64_t* rows_global_dev, void* bounce_dev, size_t bounce_bytes,
                     void* stream) {
  if (m < 0 || n_rows < 0 || m > n_rows || first_row < 0 || dim <= 0 || dim > 1024) return crs::set_error(CRS_EINVAL, "bad m/n_rows/first_row/dim");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return crs::set_error(CRS_EINVAL, "bad slab_type");
  if (m == 0 || m == n_rows) return CRS_OK;          // nothing removed / nothing survives: no row moves
  if (!dead_dev || !slab_dev || !bounce_dev) return crs::set_error(CRS_EINVAL, "null pointer");
  if (reinterpret_cast<uintptr_t>(bounce_dev) % crs::kSectionAlign) return crs::set_error(CRS_EINVAL, "bounce buffer must be 256-byte aligned");
  const int row_bytes = crs_row_elems(dim, slab_type) * (slab_type == CRS_SLAB_I8 ? 1 : 2);
  const bool has_shadow = shadow_f32_dev != nullptr;
  const int64_t W = crs::window_rows(row_bytes, dim, has_shadow, bounce_bytes);
  if (W <= 0) return crs::set_error(CRS_EINVAL, "bounce buffer too small (crs_slab_compact_bounce_bytes)");
  const int64_t n_out = n_rows - m;
  crs::CompactArgs a;
  a.dead = dead_dev; a.m = m; a.n_rows = n_rows;
  a.row_bytes = row_bytes; a.dim = dim;
  a.slab = reinterpret_cast<char*>(slab_dev); a.shadow = shadow_f32_dev; a.scales = scales_dev; a.rows_global = rows_global_dev;
  char* p = reinterpret_cast<char*>(bounce_dev);
  a.b.slab = p;            p += crs::align_up((size_t)W * row_bytes, crs::kSectionAlign);
  a.b.shadow = p;          if (has_shadow) p += crs::align_up((size_t)W * dim * 4 + 16, crs::kSectionAlign);
  a.b.scales = reinterpret_cast<float*>(p);        p += crs::align_up((size_t)W * 4, crs::kSectionAlign);
  a.b.rows_global = reinterpret_cast<int64_t*>(p); p += crs::align_up((size_t)W * 8, crs::kSectionAlign);
  if ((size_t)(p - reinterpret_cast<char*>(bounce_dev)) > bounce_bytes) return crs::set_error(CRS_EINVAL, "bounce buffer too small");
  // windows start at a multiple of W at or below first_row, so the windows (and the proof above) do not depend on the hint
  for (int64_t d0 = first_row / W * W; d0 < n_out; d0 += W) {
    a.d0 = d0;
    a.w = (int)(n_out - d0 < W ? n_out - d0 : W);
    const unsigned blocks = (unsigned)((a.w + crs::kRowsPerBlock - 1) / crs::kRowsPerBlock);
    hipLaunchKernelGGL((crs::compact_window_kernel<true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL((crs::compact_window_kernel<false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, a);
  }
  return crs::launch_status("slab_compact");
}

}  // extern "C"
