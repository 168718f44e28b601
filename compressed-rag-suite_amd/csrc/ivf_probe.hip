// ivf_probe.hip -- top-k' of gathered slab rows, a different set of lists per query, on the matrix cores.
// Declared in include/crs_hip.h: crs_ivf_topk, crs_ivf_workspace_bytes, crs_ivf_plan_describe.  Layout and limits: ivf.h.
//
// Grouping (ivf_group_kernel, one workgroup).  Every (query, slot) pair becomes the key list << 14 | pair (no list: all ones);
// the keys are sorted in LDS (bitonic, ascending), so the pairs that probe one list are neighbours and ascend.  A key starts a
// work item when its distance to the first key of its list is a multiple of 16; a prefix sum over those heads numbers the items.
// Sorted keys, item starts, item count and valid-key count stay on the device: the probe kernel is launched with the upper
// bound nq * nprobe of workgroups and those past the count exit at once.
//
// Probe (ivf_probe_kernel, one workgroup per item).  v_mfma_f32_16x16x32_f16 with A = 16 gathered slab rows and B = the item's
// <= 16 queries.  The order of k inside the dot product is free as long as both operands agree: lane r + 16 g holds elements
// g pdim / 4 + 8 s .. + 7 of row r in k-step s, so a lane walks one contiguous quarter of its row (16 bytes per step, global ->
// VGPR -> matrix pipe, no LDS) and the queries are loaded once in the same order and stay in registers for the whole list.
// The waves split the list's 16-row tiles (wave w: tiles w, w + 4, ...), `ring` tiles in flight per wave.
//
// Selection runs in the sweep, as in scan_mxfp4.hip: D leaves the pipe as lane = query + 16 g holding rows 4 g .. 4 g + 3 of the
// tile; a score above the query's threshold tau joins the query's buffer in LDS (2 k' keys of ordered score << 32 | ~row); a
// buffer that could not take another tile is sorted by the wave, cut to k', and tau becomes its last score.  A list's rows ascend
// and so do a wave's tiles, so a later row that ties tau ranks behind the buffer and `>` is exact.  At the end every wave leaves
// k' sorted keys per query in LDS and the waves' lists are joined there: wave w sorts the 4 k' keys of queries w, w + 4, ...
// and writes the best k' to the pair's slot of the static [nq, nprobe, k'] output, (-inf, -1) in the empty places.  The
// workgroup whose number is a pair without a list fills that pair's slot, so no slot is left unwritten and none is written twice.
// merge.hip (stage-2 layout) reduces the nprobe lists of a query to its k best.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "ivf.h"
#include "scan.h"
#include "scan_common.h"
#include "wave_sort.h"

namespace crs {
namespace {

constexpr unsigned kNoKey = 0xffffffffu;
constexpr unsigned kPairMask = (1u << kIvfPairBits) - 1u;

// ---------------------------------------------------------------- grouping
// LDS: keys [n] | scan [threads].  n is a power of two >= pairs and a multiple of the thread count.
__global__ __launch_bounds__(1024) void ivf_group_kernel(const int* __restrict__ probes, int pairs, int nlist, int n,
                                                         unsigned* __restrict__ keys_out, int* __restrict__ item_start,
                                                         int* __restrict__ header) {
  extern __shared__ unsigned grp_lds[];
  unsigned* keys = grp_lds;
  int* scan = reinterpret_cast<int*>(grp_lds + n);
  __shared__ int n_valid_sh;
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) n_valid_sh = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < n; i += nt) {
    const int l = i < pairs ? probes[i] : -1;
    const bool in = l >= 0 && l < nlist;
    keys[i] = in ? ((unsigned)l << kIvfPairBits) | (unsigned)i : kNoKey;
    mine += in ? 1 : 0;
  }
  if (mine) atomicAdd(&n_valid_sh, mine);
  __syncthreads();
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n / 2; i += nt) {
        const int lo = 2 * i - (i & (j - 1)), hi = lo + j;
        const unsigned a = keys[lo], b = keys[hi];
        const bool up = (lo & k) == 0;
        if ((a > b) == up) { keys[lo] = b; keys[hi] = a; }
      }
      __syncthreads();
    }
  }
  // valid keys are the first n_valid: an all-ones key of list 2^18 - 1 and pair 2^14 - 1 equals the filler, and is told apart by position
  const int n_valid = n_valid_sh;
  const int per = n / nt, first = tid * per;
  unsigned heads = 0;      // bit e: key first + e starts an item (per <= 16)
  for (int e = 0; e < per; ++e) {
    const int i = first + e;
    if (i >= n_valid) break;
    const unsigned key = keys[i];
    keys_out[i] = key;
    const unsigned base = key & ~kPairMask;
    int lo = 0, hi = i;      // first key of this list: the smallest index whose key >= base
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (keys[mid] >= base) hi = mid; else lo = mid + 1;
    }
    if (((i - lo) & (kIvfItemPairs - 1)) == 0) heads |= 1u << e;
  }
  const int c = __popc(heads);
  scan[tid] = c;
  __syncthreads();
  for (int o = 1; o < nt; o <<= 1) {      // inclusive prefix sum over the threads
    const int v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  int at = scan[tid] - c;
  for (int e = 0; e < per; ++e)
    if ((heads >> e) & 1u) item_start[at++] = first + e;
  if (tid == nt - 1) { header[0] = scan[tid]; header[1] = n_valid; }
}

// ---------------------------------------------------------------- probe
struct IvfArgs {
  const _Float16* q16;        // [nq, pdim]
  const _Float16* slab;       // [n_rows, pdim]
  const int* list_offsets;    // [nlist + 1]
  const int* list_rows;       // [n_list_rows]
  const int* probes;          // [pairs]
  const unsigned* keys;       // sorted, [header[1]]
  const int* item_start;      // [header[0]]
  const int* header;
  float* part_s;              // [pairs, kp]
  int* part_r;
  int n_rows, n_list_rows, nlist, nprobe, pairs, pdim;
};

template <int KS>
struct IvfTile {
  f16x8 d[KS];
  int row;      // lanes 0..15: the slab row of tile row `lane`, -1 past the list's end (or for a row number outside the slab)
};

template <int KS>
__device__ __forceinline__ void load_tile(IvfTile<KS>& t, const IvfArgs& a, const int* rows, int len, int tile, int lane) {
  const int idx = tile * 16 + (lane & 15);
  const int row = rows[idx < len ? idx : len - 1];      // past the end: the list's last row again, its scores are dropped
  const bool ok = idx < len && (unsigned)row < (unsigned)a.n_rows;
  const _Float16* p = a.slab + (size_t)(ok ? row : 0) * (size_t)a.pdim + (size_t)(lane >> 4) * (KS * 8);
#pragma unroll
  for (int s = 0; s < KS; ++s) t.d[s] = *reinterpret_cast<const f16x8*>(p + 8 * s);
  t.row = ok ? row : -1;
}

// Sort query q's buffer and keep its KP best in place (slots past the count hold the empty key 0).
template <int E>
__device__ __forceinline__ void compact_query(u64* buf, int q, int lane, int& cnt, float& tau) {
  constexpr int CAP = 64 * E, KP = 32 * E;
  const int n = __shfl(cnt, q);
  u64 key[E];
#pragma unroll
  for (int u = 0; u < E; ++u) key[u] = (lane + 64 * u < n) ? buf[q * CAP + lane + 64 * u] : 0;
  wave_sort_keys<E>(key, lane);
#pragma unroll
  for (int u = 0; u < E; ++u)
    if (lane + 64 * u < KP) buf[q * CAP + lane + 64 * u] = key[u];
  const u64 kth = __shfl(key[(KP - 1) >> 6], (KP - 1) & 63);
  if ((lane & 15) == q) {
    if (n >= KP) tau = float_of_ord((unsigned)(kth >> 32));
    cnt = n < KP ? n : KP;
  }
}

template <int KS, int E, int PF>
__global__ __launch_bounds__(64 * kIvfWaves) void ivf_probe_kernel(const IvfArgs a) {
  constexpr int CAP = 64 * E, KP = 32 * E, W = kIvfWaves;
  extern __shared__ u64 ivf_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qb = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;

  // pair b has no list: its slot is nobody's work, fill it
  {
    const int l = a.probes[b];
    if (!(l >= 0 && l < a.nlist))
      for (int e = threadIdx.x; e < KP; e += 64 * W) {
        a.part_s[(size_t)b * KP + e] = kNegInf;
        a.part_r[(size_t)b * KP + e] = -1;
      }
  }
  if (b >= a.header[0]) return;
  const int n_valid = a.header[1];
  const int start = a.item_start[b];
  const unsigned list = a.keys[start] >> kIvfPairBits;

  // this lane's query: pair start + qb while it still probes `list`
  int pair = -1;
  if (start + qb < n_valid) {
    const unsigned key = a.keys[start + qb];
    if ((key >> kIvfPairBits) == list) pair = (int)(key & kPairMask);
  }
  f16x8 qreg[KS];
  {
    const _Float16* qp = a.q16 + (size_t)(pair >= 0 ? pair / a.nprobe : 0) * a.pdim + g * (KS * 8);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      qreg[s] = *reinterpret_cast<const f16x8*>(qp + 8 * s);
      if (pair < 0) qreg[s] = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  int off = a.list_offsets[list], end = a.list_offsets[list + 1];
  off = off < 0 ? 0 : (off > a.n_list_rows ? a.n_list_rows : off);
  end = end < off ? off : (end > a.n_list_rows ? a.n_list_rows : end);
  const int len = end - off, n_tiles = (len + 15) >> 4;
  const int* rows = a.list_rows + off;

  u64* buf = ivf_lds + (size_t)wave * 16 * CAP;
  float tau = kNegInf;
  int cnt = 0;      // entries in this lane's query's buffer (the same value in the four lanes of the query)

  IvfTile<KS> ring[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    const int tile = wave + p * W;
    if (tile < n_tiles) load_tile<KS>(ring[p], a, rows, len, tile, lane);
  }
  for (int base = wave; base < n_tiles; base += PF * W) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int tile = base + p * W;
      if (tile >= n_tiles) break;      // (uniform)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(ring[p].d[s], qreg[s], acc, 0, 0, 0);
      int rowj[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) rowj[j] = __shfl(ring[p].row, 4 * g + j);
      const int next = tile + PF * W;
      if (next < n_tiles) load_tile<KS>(ring[p], a, rows, len, next, lane);

      float sc[4];
      unsigned pass = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[j] = acc[j] + 0.f;      // -0 -> +0: equal scores share one key image
        pass |= (pair >= 0 && rowj[j] >= 0 && sc[j] > tau) ? 1u << j : 0u;
      }
      if (__any(pass != 0)) {
        const int c = __popc(pass);
        const int c0 = __shfl(c, qb), c1 = __shfl(c, qb + 16), c2 = __shfl(c, qb + 32), c3 = __shfl(c, qb + 48);
        int pos = cnt + (g > 0 ? c0 : 0) + (g > 1 ? c1 : 0) + (g > 2 ? c2 : 0);      // <= cnt + 16 <= CAP: see below
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((pass >> j) & 1u) buf[qb * CAP + pos++] = ((u64)ord_of(sc[j]) << 32) | (0xffffffffu - (unsigned)rowj[j]);
        cnt += c0 + c1 + c2 + c3;
        if (__any(cnt > CAP - 16)) {      // a buffer that could not take 16 more: cut it to KP <= CAP - 16
          lds_wave_sync();
          for (int q = 0; q < 16; ++q)
            if (__shfl(cnt, q) > CAP - 16) compact_query<E>(buf, q, lane, cnt, tau);
          lds_wave_sync();
        }
      }
    }
  }
  // every wave leaves KP sorted keys per query (0 = empty) ...
  lds_wave_sync();
  for (int q = 0; q < 16; ++q) compact_query<E>(buf, q, lane, cnt, tau);
  __syncthreads();
  // ... and wave w joins the W lists of queries w, w + W, ...
  constexpr int EJ = W * KP / 64;
  for (int q = wave; q < 16; q += W) {
    const int qpair = __shfl(pair, q);
    if (qpair < 0) continue;      // (uniform)
    u64 key[EJ];
#pragma unroll
    for (int u = 0; u < EJ; ++u) {
      const int e = lane + 64 * u;
      key[u] = ivf_lds[((size_t)(e / KP) * 16 + q) * CAP + (e % KP)];
    }
    wave_sort_keys<EJ>(key, lane);
#pragma unroll
    for (int u = 0; u < EJ; ++u) {
      const int e = lane + 64 * u;
      if (e < KP) {
        const bool in = key[u] != 0;
        a.part_s[(size_t)qpair * KP + e] = in ? float_of_ord((unsigned)(key[u] >> 32)) : kNegInf;
        a.part_r[(size_t)qpair * KP + e] = in ? (int)(0xffffffffu - (unsigned)key[u]) : -1;
      }
    }
  }
}

using ProbeKernel = void (*)(const IvfArgs);
template <int KS>
constexpr ProbeKernel kernel_of(int kp) {
  constexpr int PF = KS <= 8 ? 4 : 2;      // IvfPlan::ring
  return kp == 32 ? ivf_probe_kernel<KS, 1, PF> : ivf_probe_kernel<KS, 2, PF>;
}
ProbeKernel probe_kernel(int ksteps, int kp) {
  switch (ksteps) {
    case 4: return kernel_of<4>(kp);
    case 8: return kernel_of<8>(kp);
    case 12: return kernel_of<12>(kp);
    case 16: return kernel_of<16>(kp);
    case 20: return kernel_of<20>(kp);
    case 24: return kernel_of<24>(kp);
    case 28: return kernel_of<28>(kp);
    default: return kernel_of<32>(kp);
  }
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_ivf_workspace_bytes(int nq, int dim, int nprobe, int kp, size_t* bytes) {
  crs::IvfPlan p;
  const char* why = "";
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer (bytes)");
  if (crs::ivf_make_plan(nq, dim, nprobe, 1, kp, 1, 1, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  *bytes = crs::ivf_ws_layout(p).bytes;
  return CRS_OK;
}

int crs_ivf_plan_describe(int nq, int dim, int nprobe, int kp, char* buf, size_t cap) {
  crs::IvfPlan p;
  const char* why = "";
  if (!buf || cap == 0) return crs::set_error(CRS_EINVAL, "null buffer");
  if (crs::ivf_make_plan(nq, dim, nprobe, 1, kp, 1, 1, &p, &why)) return crs::set_error(CRS_EINVAL, why);
  crs::ivf_plan_describe(p, buf, cap);
  return CRS_OK;
}

int crs_ivf_topk(const void* q16_dev, int nq, int dim, const void* slab_dev, int64_t n_rows, const int32_t* list_offsets_dev,
                 int64_t nlist, const int32_t* list_rows_dev, int64_t n_list_rows, const int32_t* probes_dev, int nprobe, int k, int kp,
                 void* workspace_dev, size_t workspace_bytes, float* out_scores_dev, int64_t* out_rows_dev, void* stream) {
  using namespace crs;
  IvfPlan p;
  const char* why = "";
  if (ivf_make_plan(nq, dim, nprobe, k, kp, n_rows, nlist, &p, &why)) return set_error(CRS_EINVAL, why);
  if (n_list_rows < 0 || n_list_rows >= ((int64_t)1 << 31)) return set_error(CRS_EINVAL, "n_list_rows must be in 0..2^31 - 1");
  if (!q16_dev) return set_error(CRS_EINVAL, "null pointer (q16_dev)");
  if (!slab_dev) return set_error(CRS_EINVAL, "null pointer (slab_dev)");
  if (!list_offsets_dev) return set_error(CRS_EINVAL, "null pointer (list_offsets_dev)");
  if (!list_rows_dev && n_list_rows > 0) return set_error(CRS_EINVAL, "null pointer (list_rows_dev)");
  if (!probes_dev) return set_error(CRS_EINVAL, "null pointer (probes_dev)");
  if (!workspace_dev) return set_error(CRS_EINVAL, "null pointer (workspace_dev)");
  if (!out_scores_dev || !out_rows_dev) return set_error(CRS_EINVAL, "null pointer (out_scores_dev / out_rows_dev)");
  const IvfWs w = ivf_ws_layout(p);
  if (workspace_bytes < w.bytes) return set_error(CRS_ENOSPC, "workspace too small (crs_ivf_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace_dev);
  int* header = reinterpret_cast<int*>(ws + w.header);
  unsigned* keys = reinterpret_cast<unsigned*>(ws + w.keys);
  int* items = reinterpret_cast<int*>(ws + w.items);
  float* part_s = reinterpret_cast<float*>(ws + w.part_s);
  int* part_r = reinterpret_cast<int*>(ws + w.part_r);
  if (p.group_lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)ivf_group_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, p.group_lds) != hipSuccess)
    return launch_status("ivf_topk (grouping LDS size)");
  hipLaunchKernelGGL(ivf_group_kernel, dim3(1), dim3(p.group_threads), (size_t)p.group_lds, st, probes_dev, p.pairs, (int)nlist, p.sort_n,
                     keys, items, header);
  const IvfArgs a{(const _Float16*)q16_dev, (const _Float16*)slab_dev, list_offsets_dev, list_rows_dev, probes_dev, keys, items, header,
                  part_s, part_r, (int)n_rows, (int)n_list_rows, (int)nlist, nprobe, p.pairs, p.pdim};
  const ProbeKernel kern = probe_kernel(p.ksteps, kp);
  if (p.probe_lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.probe_lds) != hipSuccess)
    return launch_status("ivf_topk (probe LDS size)");
  hipLaunchKernelGGL(kern, dim3(p.pairs), dim3(64 * p.waves), (size_t)p.probe_lds, st, a);
  merge_launch_i32(part_s, part_r, nprobe, nq, kp, k, 0, out_scores_dev, out_rows_dev, nullptr, nullptr, st);
  return launch_status("ivf_topk");
}

}  // extern "C"
