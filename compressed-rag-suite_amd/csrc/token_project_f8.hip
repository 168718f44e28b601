// token_project_f8.hip -- hidden states to packed e4m3 token vectors (gfx950): crs_token_project_f8.  The kernel
// is token_project.h's, instantiated for the fp8 output: the same projection, bias and fp32 normalisation as crs_token_project,
// then y 2^S (e4m3.h) encoded as one byte per coordinate, code 0 in [dim, dimp).
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>

#include "scan.h"
#include "token_project.h"

namespace crs {

int token_project_f8_launch(const float* hidden, const void* w16, const float* bias, const int64_t* dst, void* out8, int64_t n_tok,
                            int H, int dim, hipStream_t stream) {
  const int dimp = (dim + 31) / 32 * 32;
  const dim3 grid((unsigned)((n_tok + 63) / 64)), block(kTpThreads);
#define CRS_TP8_LAUNCH(NJ)                                                                                                         \
  hipLaunchKernelGGL((token_project_kernel<NJ, true>), grid, block, 0, stream, hidden, static_cast<const _Float16*>(w16), bias,    \
                     reinterpret_cast<const long long*>(dst), out8, (long long)n_tok, H, dim)
  switch (dimp) {
    case 32: CRS_TP8_LAUNCH(2); break;
    case 64: CRS_TP8_LAUNCH(4); break;
    case 96: CRS_TP8_LAUNCH(6); break;
    case 128: CRS_TP8_LAUNCH(8); break;
    default: return -1;
  }
#undef CRS_TP8_LAUNCH
  return (int)hipGetLastError();
}

}  // namespace crs
