// token_project.hip -- hidden states to packed unit-length fp16 token vectors (gfx950): crs_token_project.  The
// kernel itself is in token_project.h, which token_project_f8.hip instantiates for the fp8 token index.
//
// The index-time half of late interaction: for every token with dst >= 0, v = W h (+ b), y = v / |v| (0 when |v| is 0), written as
// fp16 to row dst of the token array, zeros in [dim, dimp).  A row-complete MFMA tile, as enc_rowln.hip's: one wave owns 16 tokens
// and ALL dimp output columns (dimp / 16 accumulator tiles of v_mfma_f32_16x16x32_f16, at most 8 = 32 VGPRs), so the norm of a row
// is formed inside the wave that produced it and the projection never round-trips through memory.  Four waves per workgroup, 64
// tokens.
//   A operand: lane (r = lane & 15, h = lane >> 4) reads coordinates k0 + 8 h .. + 7 of token r's hidden row -- two 16-byte fp32
//     loads, rounded to fp16 (round to nearest even) in registers.  A token with dst < 0, or past n_tok, is NEVER read: it is a
//     padding position whose hidden state is undefined; its fragment is zeros and nothing is stored for it.
//   B operand: the same coordinates of row 16 j + r of W, one 16-byte load per column tile j, straight from global memory -- W is
//     at most 128 x 1024 fp16 = 256 KB and stays in L2 for the whole launch.  Rows at or past dim are zeros and are not read.
//     Every wave reads the whole of W for its 16 tokens and the four waves of a workgroup share nothing: about four times the L2
//     traffic of the hidden block itself (96 KB of W against 24 KB of hidden states per wave at 128 x 384).  Staging W through LDS
//     once per workgroup would remove three quarters of it; whether that matters has NOT been measured -- the index build is
//     bound by the encoder forward in front of this kernel.
//   Epilogue: accumulator register e of lane (c = lane & 15, g = lane >> 4), tile j is column 16 j + c of token 4 g + e.  Bias in
//     fp32, squares summed over the lane's tiles in j order, then an xor butterfly over the 16 lanes of the row; 1 / sqrt in fp32;
//     the scaled value is rounded to fp16 once.  The 16 lanes of a row store 32 contiguous bytes per tile.
//   F8: the same kernel up to the last rounding -- y 2^S (an exact scaling) is encoded as e4m3 instead of fp16, one byte per
//     (token, column): the 16 lanes of a row store 16 contiguous bytes per tile, zeros (code 0) in [dim, dimp).
// A token's arithmetic involves its own row of A alone: its output does not depend on what else is in the launch.  No scratch, no
// LDS, no atomics.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"
#include "token_project.h"

namespace crs {

int token_project_launch(const float* hidden, const void* w16, const float* bias, const int64_t* dst, void* out16, int64_t n_tok,
                         int H, int dim, hipStream_t stream) {
  const int dimp = (dim + 31) / 32 * 32;
  const dim3 grid((unsigned)((n_tok + 63) / 64)), block(kTpThreads);
#define CRS_TP_LAUNCH(NJ)                                                                                                          \
  hipLaunchKernelGGL((token_project_kernel<NJ, false>), grid, block, 0, stream, hidden, static_cast<const _Float16*>(w16), bias,   \
                     reinterpret_cast<const long long*>(dst), out16, (long long)n_tok, H, dim)
  switch (dimp) {
    case 32: CRS_TP_LAUNCH(2); break;
    case 64: CRS_TP_LAUNCH(4); break;
    case 96: CRS_TP_LAUNCH(6); break;
    case 128: CRS_TP_LAUNCH(8); break;
    default: return -1;
  }
#undef CRS_TP_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace crs
