// maxsim_rc.h -- the 2-bit residual token format ('res2'): its one decode, the operand layout and the matrix step of
// the two kernels that read it (maxsim_rc.hip, maxsim_scan_rc.hip).  Both take their fragments, their decode and their products
// from here, which is what makes a swept score bit for bit the re-rank kernel's.  Device code only.
//
// The decoded value of coordinate d of token j is an fp16 number, three individually rounded IEEE operations:
//     w16  = fp16(weights[code(j, d)])                       (round to nearest even, once per launch and weight)
//     t    = fp16_add(centroids[cid[j]][d], w16)             (v_pk_add_f16)
//     v    = fp16_mul(t, scale[j])                           (v_pk_mul_f16)
// fp16 subnormals are kept (the default mode of a gfx9 kernel).  An add followed by a multiply is no FMA candidate, and the function
// is compiled with contraction off all the same.  Why packed fp16 and not fp32: a k-step of a lane is 8 coordinates; in fp32
// that is 8 conversions, 8 adds, 8 multiplies and 4 packing conversions beside the weight selects, in packed fp16 4 adds and 4
// multiplies beside 4 byte permutes, and the sweep's decode is VALU work that competes with nothing but the MFMA issue slots.
// A token whose cid is outside [0, n_centroids) decodes to zeros: its cid is replaced by 0 and its scale by +0 before any read.
//
// Layout.  A row is dimp = 32 KS coordinates.  Lane (r = lane & 15, h = lane >> 4) of a fragment holds the 8 KS CONSECUTIVE
// coordinates [8 KS h, 8 KS (h + 1)) of token r, 8 per k-step -- so its codes are 2 KS consecutive bytes of the token's code row
// and its share of a centroid row is KS consecutive 16-byte loads.  The queries are cut the same way, which is all a dot product
// needs.  k-steps are accumulated in ascending order from a zero accumulator by v_mfma_f32_16x16x32_f16: exact products, fp32
// accumulation.
#pragma once
#include <hip/hip_runtime.h>

#include "maxsim_f8.h"      // f8_f32x4, f8_row_sum: maxsim.hip's step 4, shared by every MaxSim kernel that came after it

namespace crs {
namespace {

typedef _Float16 rc_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 rc_f16x2 __attribute__((ext_vector_type(2)));

struct RcCodec {                      // what a kernel needs of a codec
  const _Float16* centroids;          // [n_centroids, dimp] unit rows, zeros past dim
  const float* weights;               // [4]
  int n_centroids;
};
struct RcPlanes {                     // the token index: three planes in token order
  const int* cid;                     // [n_tokens]
  const unsigned char* codes;         // [n_tokens, dimp / 4]: coordinate d in bits 2 (d % 4) of byte d / 4
  const unsigned short* scale;        // [n_tokens] fp16 bits
};

// the weight table as fp16 pairs {w0, w1}, {w2, w3}: the byte table of the decode's permutes
struct RcWeights { unsigned lo, hi; };
__device__ __forceinline__ RcWeights rc_weights(const float* w) {
  const rc_f16x2 a = rc_f16x2{(_Float16)w[0], (_Float16)w[1]}, b = rc_f16x2{(_Float16)w[2], (_Float16)w[3]};
  return RcWeights{__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b)};
}

// the 2 KS code bytes of lane h's coordinates, from a token's code row (global memory or LDS), in the low bits
template <int KS>
__device__ __forceinline__ unsigned long long rc_load_codes(const unsigned char* row, int h) {
  const unsigned char* p = row + 2 * KS * h;
  if constexpr (KS == 4) {
    const uint2 v = *reinterpret_cast<const uint2*>(p);
    return ((unsigned long long)v.y << 32) | v.x;
  } else if constexpr (KS == 2) {
    return *reinterpret_cast<const unsigned*>(p);
  } else if constexpr (KS == 3) {
    const unsigned short* s = reinterpret_cast<const unsigned short*>(p);      // 6 h: two-byte aligned only
    return ((unsigned long long)s[2] << 32) | ((unsigned)s[1] << 16) | s[0];
  } else {
    return *reinterpret_cast<const unsigned short*>(p);
  }
}

template <int KS>
struct RcRaw {                        // one lane's share of a token, as stored
  uint4 cent[KS];                     // its 8 KS coordinates of the token's centroid
  unsigned long long codes;
  unsigned scale2;                    // the token's scale in both halves
};
template <int KS>
struct RcFrag { rc_f16x8 v[KS]; };    // the same, decoded: one f16x8 per k-step

// lane h's share of the centroid row of a token (cid already inside the table)
template <int KS>
__device__ __forceinline__ void rc_gather(RcRaw<KS>& raw, const RcCodec& c, int cid, int h) {
  const uint4* row = reinterpret_cast<const uint4*>(c.centroids + (size_t)cid * (32 * KS)) + KS * h;
#pragma unroll
  for (int s = 0; s < KS; ++s) raw.cent[s] = row[s];
}
// cid and scale as stored -> what the decode uses: a cid outside the table reads centroid 0 and scales by +0
__device__ __forceinline__ void rc_checked(int& cid, unsigned& scale, int n_centroids) {
  const bool in = (unsigned)cid < (unsigned)n_centroids;
  cid = in ? cid : 0;
  scale = in ? scale : 0u;
}

// THE decode: two coordinates (codes a, b in bits 0..1 and 2..3 of `nib`) of a centroid pair c2
__device__ __forceinline__ unsigned rc_decode2(unsigned c2, unsigned a, unsigned b, const RcWeights w, unsigned scale2) {
#pragma clang fp contract(off)
  const unsigned sel = (a | (b << 16)) * 0x0202u + 0x01000100u;      // bytes 2a, 2a + 1, 2b, 2b + 1 of the table
  const rc_f16x2 wv = __builtin_bit_cast(rc_f16x2, __builtin_amdgcn_perm(w.hi, w.lo, sel));
  const rc_f16x2 t = __builtin_bit_cast(rc_f16x2, c2) + wv;
  const rc_f16x2 v = t * __builtin_bit_cast(rc_f16x2, scale2);
  return __builtin_bit_cast(unsigned, v);
}
template <int KS>
__device__ __forceinline__ RcFrag<KS> rc_decode(const RcRaw<KS>& raw, const RcWeights w) {
  RcFrag<KS> out;
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    typedef unsigned u4 __attribute__((ext_vector_type(4)));
    const unsigned c16 = (unsigned)(raw.codes >> (16 * s)) & 0xffffu;
    const uint4 c = raw.cent[s];
    const u4 d = u4{rc_decode2(c.x, c16 & 3u, (c16 >> 2) & 3u, w, raw.scale2), rc_decode2(c.y, (c16 >> 4) & 3u, (c16 >> 6) & 3u, w, raw.scale2),
                    rc_decode2(c.z, (c16 >> 8) & 3u, (c16 >> 10) & 3u, w, raw.scale2), rc_decode2(c.w, (c16 >> 12) & 3u, (c16 >> 14) & 3u, w, raw.scale2)};
    out.v[s] = __builtin_bit_cast(rc_f16x8, d);
  }
  return out;
}

// lane (r, h)'s fragment of an fp16 query row (global memory, 16-byte aligned)
template <int KS>
__device__ __forceinline__ RcFrag<KS> rc_load_query(const _Float16* row, int h) {
  RcFrag<KS> out;
  const rc_f16x8* p = reinterpret_cast<const rc_f16x8*>(row) + KS * h;
#pragma unroll
  for (int s = 0; s < KS; ++s) out.v[s] = p[s];
  return out;
}
template <int KS>
__device__ __forceinline__ RcFrag<KS> rc_zero() {
  RcFrag<KS> out;
#pragma unroll
  for (int s = 0; s < KS; ++s) out.v[s] = rc_f16x8{0, 0, 0, 0, 0, 0, 0, 0};
  return out;
}

// <16 query tokens, 16 document tokens> from a zero accumulator, k-steps in ascending order
template <int KS>
__device__ __forceinline__ f8_f32x4 rc_mfma(const RcFrag<KS>& a, const RcFrag<KS>& b) {
  f8_f32x4 acc = f8_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.v[s], b.v[s], acc, 0, 0, 0);
  return acc;
}

}  // namespace
}  // namespace crs
