// token_compress.hip -- fp16 unit token vectors to the 2-bit residual format (gfx950): crs_token_compress.
//
//     cid[j]    = argmax_c <x_j, centroid_c>, ties to the lowest c          (fp16 products, fp32 accumulation on the matrix pipe)
//     code[j,d] = #{i : x_j[d] - centroid_cid[d] >= cutoffs[i]}             (fp32 subtraction of two fp16 values: exact)
//     scale[j]  = fp16(1 / sqrt(sum_{d < dim} (centroid_cid[d] + weights[code[j,d]])^2))     (fp32)
//
// With codes_dev and scale_dev absent only the first stage runs: that is the assignment step of the codec's k-means.
//
// Stage 1, nearest centroid.  A workgroup of four waves owns 64 tokens, 16 per wave, held as MFMA A fragments for the whole
// kernel (KS registers quads per lane).  The centroid table streams through LDS in tiles of 64 centroids, two buffers, LDS-DMA,
// one barrier per tile (tile n + 1 is issued right after the barrier that publishes tile n, into the buffer tile n - 1 was read
// from).  A wave multiplies its tokens against the four 16-centroid column blocks of a tile with v_mfma_f32_16x16x32_f16;
// accumulator register e of lane (c, g) is <token 4 g + e, centroid 16 cb + c>, so a lane meets centroids in ascending order and a
// strict > keeps the lowest id; the 16 lanes of a token are reduced at the end by an xor butterfly on (dot, id) with the same rule.
// A centroid at or past K (the ragged last tile re-reads centroid K - 1) is never a candidate.
//   Swizzle.  A tile row is kCpr = dimp / 8 chunks of 16 bytes; the 16 lanes of a ds_read_b128 pass read one chunk column of 16
//   consecutive rows.  Chunk c of row p is stored at c ^ ((p >> sh) & (m - 1)), m the lowest set bit of kCpr (16, 8, 4, 4 for
//   dimp 128, 64, 32, 96) and sh = log2(16 / m): the bank group (kCpr p + c') mod 16 is then a bijection of p mod 16 -- the low
//   log2(m) bits come from the xor term, the rest from (kCpr / m) p, kCpr / m odd.  The transfer is linear on the LDS side, so the
//   (self-inverse) map is applied to the source address.
// Stage 2, residual codes.  The winning ids go back to the lane layout of the A fragments by four shuffles: lane (r, h) holds
// coordinates 32 s + 8 h .. + 7 of token r for every k-step s, re-reads exactly those of the winning centroid row (KS 16-byte
// loads), buckets the 8 residuals of a k-step into one 16-bit word -- coordinate d in bits 2 (d % 4) of byte d / 4 -- stores it,
// and adds its share of the norm; the four lanes of a token are reduced by two xor steps and lane h = 0 stores cid and scale.
// No scratch, no atomics.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "lds_dma.h"
#include "scan.h"

namespace crs {
namespace {

typedef __attribute__((address_space(3))) void* tc_lds_ptr_t;
typedef _Float16 tc_f16x8 __attribute__((ext_vector_type(8)));
typedef float tc_f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTcThreads = 256;
constexpr int kTcTile = 64;           // centroids of a staged tile

template <int KS>
__device__ __forceinline__ int tc_swz(int c, int p) {
  constexpr int kCpr = 4 * KS, m = kCpr & -kCpr, sh = m == 16 ? 0 : (m == 8 ? 1 : 2);
  return c ^ ((p >> sh) & (m - 1));
}

template <int KS>   // dimp = 32 KS
__global__ __launch_bounds__(kTcThreads) void token_compress_kernel(const _Float16* __restrict__ tok16, long long n_tok, int dim,
                                                                    const _Float16* __restrict__ cent, int K,
                                                                    const float* __restrict__ cutoffs, const float* __restrict__ weights,
                                                                    int* __restrict__ cid_out, unsigned char* __restrict__ codes_out,
                                                                    unsigned short* __restrict__ scale_out) {
  constexpr int kDimp = 32 * KS, kCpr = 4 * KS, kTileB = kTcTile * kDimp * 2, kPasses = kTcTile * kCpr / kTcThreads;
  static_assert(kPasses * kTcThreads == kTcTile * kCpr, "a tile is a whole number of passes");
  __shared__ __attribute__((aligned(16))) char tc_lds[2 * kTileB];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 15, h = lane >> 4;
  const unsigned lds_base = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(tc_lds_ptr_t)tc_lds);
  const long long tok0 = (long long)blockIdx.x * 64 + wave * 16;      // blockIdx.x * 64 < n_tok; a wave past the end idles through the barriers
  const float ninf = -__builtin_huge_valf();

  // ---- the wave's tokens: lane (r, h) holds coordinates 32 s + 8 h .. + 7 of token tok0 + r (past the end: the last token again)
  long long tr = tok0 + r;
  tr = tr < n_tok ? tr : n_tok - 1;
  tc_f16x8 af[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) af[s] = *reinterpret_cast<const tc_f16x8*>(tok16 + (size_t)tr * kDimp + 32 * s + 8 * h);

  // tile `tile` into buffer `buf`: LDS chunk P = pass * 256 + tid <- chunk swz(P % kCpr) of centroid min(64 tile + P / kCpr, K - 1)
  auto issue = [&](int tile, int buf) {
#pragma unroll
    for (int pass = 0; pass < kPasses; ++pass) {
      const int P = pass * kTcThreads + tid;
      const int p = P / kCpr, c = P % kCpr;
      int row = tile * kTcTile + p;
      row = row < K ? row : K - 1;
      lds_dma16(__builtin_amdgcn_readfirstlane(lds_base + (unsigned)(buf * kTileB + pass * kTcThreads * 16 + wave * 1024)),
                cent + ((size_t)row * kCpr + tc_swz<KS>(c, p)) * 8);
    }
  };

  float bd[4] = {ninf, ninf, ninf, ninf};
  int bi[4] = {0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
  const int tiles = (K + kTcTile - 1) / kTcTile;
  issue(0, 0);
  for (int tile = 0; tile < tiles; ++tile) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                  // my transfers of this tile have landed
    __syncthreads();                                                  // everybody's have; everybody is done with tile - 1
    if (tile + 1 < tiles) issue(tile + 1, (tile + 1) & 1);
    const char* buf = tc_lds + (tile & 1) * kTileB;
#pragma unroll
    for (int cb = 0; cb < kTcTile / 16; ++cb) {
      const int p = 16 * cb + r;
      tc_f32x4 acc = tc_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const tc_f16x8 bf = *reinterpret_cast<const tc_f16x8*>(buf + (p * kCpr + tc_swz<KS>(4 * s + h, p)) * 16);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s], bf, acc, 0, 0, 0);
      }
      const int id = tile * kTcTile + 16 * cb + r;                    // this lane's column
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool better = id < K && acc[e] > bd[e];
        bd[e] = better ? acc[e] : bd[e];
        bi[e] = better ? id : bi[e];
      }
    }
  }
  // ---- the 16 lanes of a token: larger dot, then lower id
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
      const float od = __shfl_xor(bd[e], o);
      const int oi = __shfl_xor(bi[e], o);
      const bool take = od > bd[e] || (od == bd[e] && oi < bi[e]);
      bd[e] = take ? od : bd[e];
      bi[e] = take ? oi : bi[e];
    }
  }
  // token r's winner sits in register r & 3 of the lanes of group r >> 2
  int cid = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int v = __shfl(bi[e], 16 * (r >> 2));
    cid = (r & 3) == e ? v : cid;
  }
  cid = (unsigned)cid < (unsigned)K ? cid : 0;                        // every dot a NaN: centroid 0
  const bool live = tok0 + r < n_tok;
  if (live && h == 0) cid_out[tok0 + r] = cid;
  if (!codes_out) return;                                             // (uniform) assignment only

  // ---- stage 2: residual codes and the scale
  const float c0 = cutoffs[0], c1 = cutoffs[1], c2 = cutoffs[2];
  const float w0 = weights[0], w1 = weights[1], w2 = weights[2], w3 = weights[3];
  float ss = 0.f;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const tc_f16x8 cf = *reinterpret_cast<const tc_f16x8*>(cent + (size_t)cid * kDimp + 32 * s + 8 * h);
    unsigned word = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float c = (float)cf[i], res = (float)af[s][i] - c;
      const unsigned code = (unsigned)(res >= c0) + (unsigned)(res >= c1) + (unsigned)(res >= c2);
      word |= code << (2 * i);
      const float v = c + (code == 0 ? w0 : (code == 1 ? w1 : (code == 2 ? w2 : w3)));
      ss += 32 * s + 8 * h + i < dim ? v * v : 0.f;
    }
    if (live) *reinterpret_cast<unsigned short*>(codes_out + (size_t)(tok0 + r) * (kDimp / 4) + 8 * s + 2 * h) = (unsigned short)word;
  }
  ss += __shfl_xor(ss, 16);
  ss += __shfl_xor(ss, 32);
  if (live && h == 0) {
    const _Float16 sc = (_Float16)(ss > 0.f ? 1.f / sqrtf(ss) : 0.f);
    scale_out[tok0 + r] = __builtin_bit_cast(unsigned short, sc);
  }
}

}  // namespace
}  // namespace crs

extern "C" int crs_token_compress(const void* tok16_dev, int64_t n_tok, int dimp, int dim, const void* centroids_dev, int n_centroids,
                                  const float* cutoffs_dev, const float* weights_dev, int32_t* cid_dev, void* codes_dev, void* scale_dev,
                                  void* stream) {
  using namespace crs;
  if (dimp != 32 && dimp != 64 && dimp != 96 && dimp != 128) return set_error(CRS_EINVAL, "dimp must be 32, 64, 96 or 128");
  if (dim < 1 || dim > dimp) return set_error(CRS_EINVAL, "dim must be in 1..dimp");
  if (n_centroids < CRS_RC_MIN_CENTROIDS || n_centroids > CRS_RC_MAX_CENTROIDS)
    return set_error(CRS_EINVAL, "n_centroids must be in CRS_RC_MIN_CENTROIDS..CRS_RC_MAX_CENTROIDS");
  if (n_tok < 0 || n_tok > ((int64_t)1 << 36)) return set_error(CRS_EINVAL, "n_tok must be in 0..2^36");
  if (!centroids_dev) return set_error(CRS_EINVAL, "centroids_dev is null");
  if ((codes_dev == nullptr) != (scale_dev == nullptr)) return set_error(CRS_EINVAL, "codes_dev and scale_dev go together");
  if (codes_dev && (!cutoffs_dev || !weights_dev)) return set_error(CRS_EINVAL, "cutoffs_dev / weights_dev is null");
  if (n_tok == 0) return CRS_OK;
  if (!tok16_dev) return set_error(CRS_EINVAL, "tok16_dev is null");
  if (!cid_dev) return set_error(CRS_EINVAL, "cid_dev is null");
  if (((uintptr_t)tok16_dev | (uintptr_t)centroids_dev) & 15) return set_error(CRS_EINVAL, "tok16_dev / centroids_dev must be 16-byte aligned");
  if (((uintptr_t)codes_dev | (uintptr_t)scale_dev) & 1) return set_error(CRS_EINVAL, "codes_dev / scale_dev must be 2-byte aligned");
  const dim3 grid((unsigned)((n_tok + 63) / 64)), block(kTcThreads);
#define CRS_TC_LAUNCH(KS)                                                                                                          \
  hipLaunchKernelGGL(token_compress_kernel<KS>, grid, block, 0, (hipStream_t)stream, static_cast<const _Float16*>(tok16_dev),      \
                     (long long)n_tok, dim, static_cast<const _Float16*>(centroids_dev), n_centroids, cutoffs_dev, weights_dev,    \
                     cid_dev, static_cast<unsigned char*>(codes_dev), static_cast<unsigned short*>(scale_dev))
  switch (dimp) {
    case 32: CRS_TC_LAUNCH(1); break;
    case 64: CRS_TC_LAUNCH(2); break;
    case 96: CRS_TC_LAUNCH(3); break;
    default: CRS_TC_LAUNCH(4); break;
  }
#undef CRS_TC_LAUNCH
  return launch_status("token_compress");
}
