// e4m3.h -- the OCP e4m3 (e4m3fn) encoder shared by the MXFP4 query prologue (scan_mxfp4.hip) and the fp8 token index
// (token_project.hip), and that index's number format.  Device code only.
//
// An fp8 token vector is the unit vector times 2^CRS_F8_TOKEN_SHIFT, rounded once to e4m3: 1.0 becomes 256 <= 448, and a
// coordinate keeps three mantissa bits down to 2^-6 / 256 of the vector's length (subnormals below that, in steps of 2^-17).
// Documents and queries share the shift; a MaxSim score is 2^(-2 S) times the sum over the stored values.
#pragma once
#include <hip/hip_runtime.h>

#define CRS_F8_TOKEN_SHIFT 8

namespace crs {
namespace {

// e4m3 code of y >= 0: round to nearest even on the float's bits, subnormals (below 2^-6) in steps of 2^-9, saturating at 448
// (a NaN saturates too: e4m3's own NaN code 0x7f is never produced).
__device__ __forceinline__ unsigned e4m3_code(float y) {
  unsigned code;
  if (y < 0.015625f) {
    code = (unsigned)rintf(y * 512.0f);
  } else {
    const unsigned b = __float_as_uint(y);
    code = ((b + 0x7ffffu + ((b >> 20) & 1u)) >> 20) - (120u << 3);
  }
  return code > 0x7eu ? 0x7eu : code;
}
// the signed code of x (sign bit 7; -0 keeps its sign bit, which the matrix pipe treats as 0)
__device__ __forceinline__ unsigned e4m3_signed_code(float x) { return e4m3_code(fabsf(x)) | ((__float_as_uint(x) >> 31) << 7); }

}  // namespace
}  // namespace crs
