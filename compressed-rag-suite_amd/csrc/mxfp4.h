// mxfp4.h -- the MXFP4 slab: layout arithmetic and the plan of its scan.  Plain C++ (no HIP), so the planner
// (mxfp4_plan.cpp), the row build (row_build_mxfp4.hip), the scan (scan_mxfp4.hip) and tools share one definition.
//
// A slab row is pdim = dim rounded up to 128 OCP e2m1 elements and one e8m0 scale per 32 of them.  Rows are stored in tiles of
// 16 rows, a tile in k-steps of 128 elements, and a (tile, k-step) as the 1 KB that one wave64 loads as the fp4 operand of
// v_mfma_scale_f32_16x16x128_f8f6f4, in lane order:
//     data byte  ((tile * ksteps + s) * 64 + lane) * 16 + e / 2,  lane = row % 16 + 16 * kb:  elements 128 s + 32 kb + e, e = 0..31,
//                even e in the low nibble -- the lane's 32 elements are exactly the MX block kb of k-step s
//     scale byte (tile * 64 + lane) * sp + s,  sp = 4 (ksteps <= 4) or 8: one 32- or 64-bit load per lane feeds every k-step, the
//                k-step's byte is picked by the instruction's op_sel
// The fp8 (e4m3) query operand of the same instruction holds other elements per lane (measured with one-hot operands): byte i of
// lane q + 16 g is element 128 s + 64 (i / 16) + 16 g + i % 16, while the scale of MX block kb still comes from lane q + 16 kb.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace crs {

constexpr int kMxTileRows = 16;
constexpr int kMxBlock = 32;         // elements per shared scale
constexpr int kMxMaxQ = 64;          // queries per sweep, in groups of 16

constexpr int mx_pdim(int dim) { return (dim + 127) / 128 * 128; }
constexpr int mx_scale_stride(int pdim) { return pdim <= 512 ? 4 : 8; }                  // scale bytes per (row, kb) lane
inline int64_t mx_tiles(int64_t rows) { return (rows + kMxTileRows - 1) / kMxTileRows; }
inline size_t mx_data_bytes(int64_t rows, int pdim) { return (size_t)mx_tiles(rows) * kMxTileRows * (pdim / 2); }
inline size_t mx_scale_bytes(int64_t rows, int pdim) { return (size_t)mx_tiles(rows) * 64 * mx_scale_stride(pdim); }
inline int mx_row_bytes(int pdim) { return pdim / 2 + 4 * mx_scale_stride(pdim); }

// The plan of one crs_mxfp4_topk call: pure function of the sizes and the CU count.
struct MxPlan {
  int nq, kp, pdim, ksteps;
  int groups;          // 16-query groups = waves per workgroup (1..4)
  int64_t n_tiles;
  int nwg;             // tile streams = workgroups: stream w walks tiles w, w + nwg, ...
  int cap;             // entries of a (query, stream) candidate buffer in LDS: 2 kp
  int lds;             // dynamic LDS bytes of the launch
  int levels;          // 1: one sorted merge of the nwg lists; 2: groups of kMxMergeFan lists first
  size_t q_bytes, qs_bytes, part_elems, inter_elems;
};
constexpr int kMxMergeFan = 16;
// returns 0, or -1 with *why set
int mx_make_plan(int nq, int dim, int kp, int64_t n_rows, int cus, MxPlan* p, const char** why);
int mx_plan_describe(const MxPlan& p, char* buf, size_t cap);
// workspace: [fp8 query operand | query scales | partial scores | partial ids | level-1 scores | level-1 ids], 256-byte aligned
struct MxWs {
  size_t q, qs, part_s, part_i, inter_s, inter_i, bytes;
};
MxWs mx_ws_layout(const MxPlan& p);

}  // namespace crs
