// mlm_plan.cpp -- make_mlm_plan (mlm_plan.h): plain C++17, no HIP.
#include "mlm_plan.h"

namespace crs {

int make_mlm_plan(int batch, int seq, int hidden, int vocab, crs_mlm_plan* p, const char** why) {
  static const int kHidden[] = {64, 128, 256, 384, 512, 768, 1024};
  bool h_ok = false;
  for (int h : kHidden) h_ok = h_ok || h == hidden;
  if (!h_ok) { *why = "hidden must be one of 64, 128, 256, 384, 512, 768, 1024"; return 1; }
  if (batch < 1) { *why = "bad batch (batch >= 1)"; return 1; }
  if (seq < 1) { *why = "bad seq (seq >= 1)"; return 1; }
  if (vocab < 1 || vocab > (1 << 20)) { *why = "bad vocab (1 <= vocab <= 2^20)"; return 1; }
  const long long tokens = (long long)batch * seq;
  if (tokens > (1ll << 22)) { *why = "too many tokens (batch * seq <= 2^22)"; return 1; }

  p->tile_m = kMlmTileM;
  p->tile_n = kMlmTileN;
  p->tile_k = kMlmTileK;
  p->tokens = (int)tokens;
  p->grid_m = (int)((tokens + kMlmTileM - 1) / kMlmTileM);
  p->grid_n = (vocab + kMlmTileN - 1) / kMlmTileN;
  p->tokens_padded = p->grid_m * kMlmTileM;
  p->pool_grid = p->grid_m * p->grid_n;
  p->pool_threads = kMlmThreads;
  p->pool_lds_bytes = 2 * kMlmTileM * kMlmLdsRow * 2;          // A and B tiles, fp16 (kMlmTileM == kMlmTileN)
  p->xform_grid = p->tokens_padded / kMlmXformRows;
  p->xform_threads = kMlmThreads;
  p->xform_lds_bytes = 2 * 4 * kMlmXformRows * 4;              // LayerNorm partial sums: two passes x four waves x rows, fp32
  p->ew_threads = kMlmThreads;
  p->ew_grid_x = (vocab + kMlmThreads - 1) / kMlmThreads;      // zeroing and log1p: grid (ew_grid_x, batch)
  p->t16_bytes = (size_t)p->tokens_padded * hidden * 2;        // the transform's output, fp16 [tokens_padded, hidden]
  p->workspace_bytes = (p->t16_bytes + 255) / 256 * 256;
  return 0;
}

}  // namespace crs
