// scan_mxfp4.hip -- top-k' of <= 64 queries over an MXFP4 slab with the block-scaled MFMA of gfx950.
// Declared in include/crs_hip.h: crs_mxfp4_topk, crs_mxfp4_workspace_bytes, crs_mxfp4_plan_describe.
//
// Operands.  v_mfma_scale_f32_16x16x128_f8f6f4 with A = 16 slab rows (fp4, cbsz 4) and B = 16 queries (fp8 e4m3, blgp 0), each
// with one e8m0 scale per 32 elements, fp32 accumulation.  A tile's k-step is 1 KB in lane order (mxfp4.h): one 16-byte load per
// lane IS the A operand, no LDS and no shuffle between HBM and the matrix pipe.  The queries are quantised once per call by
// mx_queries_kernel (the MX rule with e4m3's range) into the B operand's lane order; a wave keeps its 16-query group resident
// in registers for the whole sweep (8 VGPRs per k-step: 48 at 768 elements, 64 at 1024).
//
// Work split.  One workgroup per tile stream, one wave per 16-query group (1..4 waves).  Stream w walks tiles w, w + nwg, ...;
// every wave of the workgroup loads the same tile, so a sweep serves up to 64 queries (where the three repeated loads are served
// from is not measured: DESIGN 3.19).  Four tiles per wave are in flight in a register ring.
//
// Selection runs in the sweep.  D leaves the pipe as lane = query % 16 + 16 g holding rows 4 g .. 4 g + 3 of the tile.  A score
// above the query's threshold tau is appended to the query's buffer in LDS (2 k' keys of (ordered score << 32 | ~row), the
// four lanes of a query take their slots by a prefix over the quad); a buffer that could not take another tile is sorted by
// the wave (bitonic over 64 lanes x k'/32 registers, descending key = score desc, row asc), cut to k' and tau becomes its last
// score.  Rows arrive in ascending order, so a later row that ties tau ranks behind the list and `>` is exact.  The stream
// ends with the same sort and leaves k' sorted (score, 64-bit id) pairs per query: merge_sorted.hip merges them.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "e4m3.h"
#include "mxfp4.h"
#include "scan.h"
#include "scan_common.h"
#include "wave_sort.h"

namespace crs {
int device_cus();   // capi.hip
namespace {

typedef int v8i __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------- query prologue: fp32 -> MX e4m3 in B-operand lane order
// One wave per query slot of the 16-query groups; slots past nq are zeroed (their columns of D are never read).
// (e4m3_code: e4m3.h)
__global__ __launch_bounds__(256) void mx_queries_kernel(const float* __restrict__ q, int nq, int dim, int pdim, uint8_t* __restrict__ qop,
                                                         uint8_t* __restrict__ qsc) {
  const int lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int group = qi >> 4, qq = qi & 15, ksteps = pdim >> 7;
  unsigned Eu[16];      // scale byte of this half wave's block in slot u: block 2 u + lane / 32
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    Eu[u] = 0;
    if (64 * u >= pdim) continue;      // (uniform)
    const int c = lane + 64 * u;
    const float x = (qi < nq && c < dim) ? q[(size_t)qi * dim + c] : 0.f;
    float amax = fabsf(x);
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
    int E = (int)((__float_as_uint(amax) >> 23) & 0xff) - 8;
    E = E < 0 ? 0 : E;
    const unsigned code = e4m3_code(fabsf(x) * __uint_as_float((unsigned)(254 - E) << 23)) | ((__float_as_uint(x) >> 31) << 7);
    const int s = c >> 7, w = c & 127;
    const int g = (w & 63) >> 4, i = 16 * (w >> 6) + (w & 15);
    qop[(((size_t)group * ksteps + s) * 64 + qq + 16 * g) * 32 + i] = (uint8_t)code;
    Eu[u] = (unsigned)E;
  }
  // lane kb < 4 assembles the 8 scale bytes of (query, block kb): k-step s is block 4 s + kb = slot 2 s + kb / 2 of half kb % 2
  u64 word = 0;
#pragma unroll
  for (int s = 0; s < 8; ++s) {
    const unsigned a = __shfl(Eu[2 * s], 32 * (lane & 1)), b = __shfl(Eu[2 * s + 1], 32 * (lane & 1));
    word |= (u64)((lane & 2) ? b : a) << (8 * s);
  }
  if (lane < 4) *reinterpret_cast<u64*>(qsc + ((size_t)group * 64 + qq + 16 * lane) * 8) = word;
}

// ---------------------------------------------------------------- the sweep
struct MxScanArgs {
  const uint8_t* data;
  const uint8_t* scales;
  const uint8_t* qop;
  const uint8_t* qsc;
  float* part_s;       // [nwg, nq, kp]
  int64_t* part_i;
  int64_t id_base;
  int n_rows, n_tiles, nq, nwg;
};

// Sort query q's buffer, keep its kp best; FINAL writes them out instead (empty slots (-inf, -1)).
template <int E, bool FINAL>
__device__ __forceinline__ void compact_query(u64* buf, int q, int lane, int& cnt, float& tau, float* out_s, int64_t* out_i,
                                              int64_t id_base) {
  constexpr int CAP = 64 * E, KP = 32 * E;
  const int n = __shfl(cnt, q);
  u64 key[E];
#pragma unroll
  for (int u = 0; u < E; ++u) key[u] = (lane + 64 * u < n) ? buf[q * CAP + lane + 64 * u] : 0;
  wave_sort_keys<E>(key, lane);
  if (FINAL) {
#pragma unroll
    for (int u = 0; u < E; ++u) {
      const int e = lane + 64 * u;
      if (e < KP) {
        const bool in = e < n;
        out_s[e] = in ? float_of_ord((unsigned)(key[u] >> 32)) : kNegInf;
        out_i[e] = in ? id_base + (int64_t)(0xffffffffu - (unsigned)key[u]) : (int64_t)-1;
      }
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < E; ++u)
    if (lane + 64 * u < KP) buf[q * CAP + lane + 64 * u] = key[u];
  const u64 kth = __shfl(key[(KP - 1) >> 6], (KP - 1) & 63);
  if ((lane & 15) == q) {
    if (n >= KP) tau = float_of_ord((unsigned)(kth >> 32));
    cnt = n < KP ? n : KP;
  }
}

template <int KS>
struct MxTile {
  uint4 d[KS];
  unsigned s0, s1;
};

template <int KS>
__device__ __forceinline__ void load_tile(MxTile<KS>& t, const MxScanArgs& a, int64_t tile, int lane) {
  const uint8_t* p = a.data + (((size_t)tile * KS) * 64 + lane) * 16;
#pragma unroll
  for (int s = 0; s < KS; ++s) t.d[s] = *reinterpret_cast<const uint4*>(p + (size_t)s * 1024);
  if (KS <= 4) {
    t.s0 = *reinterpret_cast<const unsigned*>(a.scales + ((size_t)tile * 64 + lane) * 4);
    t.s1 = 0;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(a.scales + ((size_t)tile * 64 + lane) * 8);
    t.s0 = v.x;
    t.s1 = v.y;
  }
}

template <int KS, int E>
__global__ __launch_bounds__(256) void scan_mxfp4_kernel(const MxScanArgs a) {
  constexpr int CAP = 64 * E, KP = 32 * E, PF = 4;
  extern __shared__ u64 mx_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qb = lane & 15, g = lane >> 4;
  const int stream = blockIdx.x;
  u64* buf = mx_lds + (size_t)wave * 16 * CAP;

  // the wave's query group: B operand and scales, resident for the sweep
  v8i qreg[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const uint4* p = reinterpret_cast<const uint4*>(a.qop + (((size_t)wave * KS + s) * 64 + lane) * 32);
    const uint4 lo = p[0], hi = p[1];
    qreg[s] = v8i{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
  }
  const uint2 qsv = *reinterpret_cast<const uint2*>(a.qsc + ((size_t)wave * 64 + lane) * 8);
  const int qs0 = (int)qsv.x, qs1 = (int)qsv.y;

  float tau = kNegInf;
  int cnt = 0;      // entries in this lane's query's buffer (the same value in the four lanes of the query)

  MxTile<KS> ring[PF];
#pragma unroll
  for (int p = 0; p < PF; ++p) {
    const int64_t tile = stream + (int64_t)p * a.nwg;
    if (tile < a.n_tiles) load_tile<KS>(ring[p], a, tile, lane);
  }
  for (int64_t base = stream; base < a.n_tiles; base += (int64_t)PF * a.nwg) {
#pragma unroll
    for (int p = 0; p < PF; ++p) {
      const int64_t tile = base + (int64_t)p * a.nwg;
      if (tile >= a.n_tiles) break;      // (uniform)
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const uint4 d = ring[p].d[s];
        const v8i av = v8i{(int)d.x, (int)d.y, (int)d.z, (int)d.w, 0, 0, 0, 0};
        const int sa = s < 4 ? (int)ring[p].s0 : (int)ring[p].s1, sb = s < 4 ? qs0 : qs1;
        switch (s & 3) {      // op_sel is an immediate
          case 0: acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, qreg[s], acc, 4, 0, 0, sa, 0, sb); break;
          case 1: acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, qreg[s], acc, 4, 0, 1, sa, 1, sb); break;
          case 2: acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, qreg[s], acc, 4, 0, 2, sa, 2, sb); break;
          default: acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(av, qreg[s], acc, 4, 0, 3, sa, 3, sb); break;
        }
      }
      const int64_t next = tile + (int64_t)PF * a.nwg;
      if (next < a.n_tiles) load_tile<KS>(ring[p], a, next, lane);

      // selection: this lane's query, rows 16 tile + 4 g + j
      const int row0 = (int)(tile * 16) + 4 * g;
      float sc[4];
      unsigned pass = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        sc[j] = acc[j] + 0.f;      // -0 -> +0: equal scores share one key image
        pass |= (row0 + j < a.n_rows && sc[j] > tau) ? 1u << j : 0u;
      }
      if (__any(pass != 0)) {
        const int c = __popc(pass);
        const int c0 = __shfl(c, qb), c1 = __shfl(c, qb + 16), c2 = __shfl(c, qb + 32), c3 = __shfl(c, qb + 48);
        int pos = cnt + (g > 0 ? c0 : 0) + (g > 1 ? c1 : 0) + (g > 2 ? c2 : 0);      // <= cnt + 16 <= CAP: see below
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if ((pass >> j) & 1u) buf[qb * CAP + pos++] = ((u64)ord_of(sc[j]) << 32) | (0xffffffffu - (unsigned)(row0 + j));
        cnt += c0 + c1 + c2 + c3;
        if (__any(cnt > CAP - 16)) {      // a buffer that could not take 16 more: cut it to KP <= CAP - 16
          lds_wave_sync();
          for (int q = 0; q < 16; ++q)
            if (__shfl(cnt, q) > CAP - 16) compact_query<E, false>(buf, q, lane, cnt, tau, nullptr, nullptr, 0);
          lds_wave_sync();
        }
      }
    }
  }
  lds_wave_sync();
  for (int q = 0; q < 16; ++q) {
    const int qi = wave * 16 + q;
    if (qi >= a.nq) break;
    const size_t at = ((size_t)stream * a.nq + qi) * KP;
    compact_query<E, true>(buf, q, lane, cnt, tau, a.part_s + at, a.part_i + at, a.id_base);
  }
}

using ScanKernel = void (*)(const MxScanArgs);
template <int KS>
constexpr ScanKernel kernel_of(int kp) {
  return kp == 32 ? scan_mxfp4_kernel<KS, 1> : kp == 64 ? scan_mxfp4_kernel<KS, 2> : scan_mxfp4_kernel<KS, 4>;
}
ScanKernel scan_kernel(int ksteps, int kp) {
  switch (ksteps) {
    case 1: return kernel_of<1>(kp);
    case 2: return kernel_of<2>(kp);
    case 3: return kernel_of<3>(kp);
    case 4: return kernel_of<4>(kp);
    case 5: return kernel_of<5>(kp);
    case 6: return kernel_of<6>(kp);
    case 7: return kernel_of<7>(kp);
    default: return kernel_of<8>(kp);
  }
}

}  // namespace
}  // namespace crs

extern "C" {

int crs_mxfp4_workspace_bytes(int nq, int dim, int kp, int64_t n_rows, size_t* bytes) {
  crs::MxPlan p;
  const char* why = "";
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer (bytes)");
  if (crs::mx_make_plan(nq, dim, kp, n_rows, crs::device_cus(), &p, &why)) return crs::set_error(CRS_EINVAL, why);
  *bytes = crs::mx_ws_layout(p).bytes;
  return CRS_OK;
}

int crs_mxfp4_plan_describe(int nq, int dim, int kp, int64_t n_rows, int cus, char* buf, size_t cap) {
  crs::MxPlan p;
  const char* why = "";
  if (!buf || cap == 0) return crs::set_error(CRS_EINVAL, "null buffer");
  if (crs::mx_make_plan(nq, dim, kp, n_rows, cus > 0 ? cus : crs::device_cus(), &p, &why)) return crs::set_error(CRS_EINVAL, why);
  crs::mx_plan_describe(p, buf, cap);
  return CRS_OK;
}

int crs_mxfp4_topk(const float* q32_dev, int nq, int dim, const void* data_dev, const void* scales_dev, int64_t n_rows, int kp,
                   int64_t id_base, void* workspace_dev, size_t workspace_bytes, float* out_scores_dev, int64_t* out_ids_dev,
                   void* stream) {
  using namespace crs;
  MxPlan p;
  const char* why = "";
  if (mx_make_plan(nq, dim, kp, n_rows, device_cus(), &p, &why)) return set_error(CRS_EINVAL, why);
  if (id_base < 0 || id_base > INT64_MAX - n_rows) return set_error(CRS_EINVAL, "id_base must be >= 0 and id_base + n_rows must fit int64");
  if (!q32_dev || !data_dev || !scales_dev || !workspace_dev || !out_scores_dev || !out_ids_dev) return set_error(CRS_EINVAL, "null pointer");
  const MxWs w = mx_ws_layout(p);
  if (workspace_bytes < w.bytes) return set_error(CRS_ENOSPC, "workspace too small (crs_mxfp4_workspace_bytes)");
  hipStream_t st = (hipStream_t)stream;
  uint8_t* ws = reinterpret_cast<uint8_t*>(workspace_dev);
  hipLaunchKernelGGL(mx_queries_kernel, dim3(p.groups * 4), dim3(256), 0, st, q32_dev, nq, dim, p.pdim, ws + w.q, ws + w.qs);
  float* part_s = reinterpret_cast<float*>(ws + w.part_s);
  int64_t* part_i = reinterpret_cast<int64_t*>(ws + w.part_i);
  const MxScanArgs a{(const uint8_t*)data_dev, (const uint8_t*)scales_dev, ws + w.q, ws + w.qs, part_s, part_i, id_base,
                     (int)n_rows, (int)p.n_tiles, nq, p.nwg};
  const ScanKernel kern = scan_kernel(p.ksteps, kp);
  if (p.lds > 48 * 1024 && hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds) != hipSuccess)
    return launch_status("mxfp4_topk (LDS size)");
  hipLaunchKernelGGL(kern, dim3(p.nwg), dim3(64 * p.groups), (size_t)p.lds, st, a);
  const size_t list = (size_t)nq * kp;
  if (p.levels == 1) {
    merge_sorted_launch_i64(part_s, part_i, p.nwg, nq, kp, kp, out_scores_dev, out_ids_dev, st);
  } else {
    float* inter_s = reinterpret_cast<float*>(ws + w.inter_s);
    int64_t* inter_i = reinterpret_cast<int64_t*>(ws + w.inter_i);
    const int ng = (p.nwg + kMxMergeFan - 1) / kMxMergeFan;
    for (int gi = 0; gi < ng; ++gi) {
      const int nl = p.nwg - gi * kMxMergeFan < kMxMergeFan ? p.nwg - gi * kMxMergeFan : kMxMergeFan;
      merge_sorted_launch_i64(part_s + (size_t)gi * kMxMergeFan * list, part_i + (size_t)gi * kMxMergeFan * list, nl, nq, kp, kp,
                              inter_s + (size_t)gi * list, inter_i + (size_t)gi * list, st);
    }
    merge_sorted_launch_i64(inter_s, inter_i, ng, nq, kp, kp, out_scores_dev, out_ids_dev, st);
  }
  return launch_status("mxfp4_topk");
}

}  // extern "C"
