// mlm_plan.h -- the launch plan of crs_mlm_sparse_pool (mlm_pool.hip): grids, workgroup sizes, LDS and the workspace of the four
// launches, as a pure function of the sizes (mlm_plan.cpp: plain C++17, no HIP), so tests/test_sparse_cpu.py checks the geometry
// without a device.  The launcher reads the plan and decides nothing.
#pragma once
#include <stddef.h>

#include "../../include/crs_encoder.h"

namespace crs {

constexpr int kMlmTileM = 128;      // token rows of a vocabulary-projection tile
constexpr int kMlmTileN = 128;      // vocabulary columns of a tile
constexpr int kMlmTileK = 64;       // contraction elements staged per step
constexpr int kMlmLdsRow = kMlmTileK + 8;   // halves per staged row: 128 bytes + one 16-byte access of padding
constexpr int kMlmThreads = 256;    // four waves, 2 x 2, 64 x 64 outputs each
constexpr int kMlmXformRows = 32;   // token rows of a transform workgroup
constexpr int kMlmGroupM = 16;      // row tiles that consecutive workgroups share before moving along the vocabulary

// 0 and *p filled in, or a message in *why and a nonzero return (the sizes are not crs_mlm_sparse_pool's)
int make_mlm_plan(int batch, int seq, int hidden, int vocab, crs_mlm_plan* p, const char** why);

}  // namespace crs
