// scan_forms.h -- the forms of the scan kernels that exist, stated once: geometry per kernel family (tile rows, resident
// workgroups per CU, queries per workgroup), chain slots for a k, and one predicate per family that says which template
// instantiations the launch ladders of the scan_*.hip files hold.  The planner (plan.cpp) chooses among these and the ladders take
// their `if constexpr` conditions from the same predicates, so a plan the planner returns is a kernel the launcher has.
// Plain constexpr C++: no HIP, no environment.
#pragma once

namespace crs {

// Kernel families of a search, in the planner's order of preference from last to first (plan.cpp: make_plan).
//   Classic   threshold / compaction scan (scan.hip; int8 slabs: scan_i8.hip with slots = -1): exact lists of rows, any k <= 64
//   TileBest  one representative per tile, dumped (slots = 0) or kept in a register chain (scan_tb.hip; int8 slabs: scan_i8.hip)
//   Wide      65+ queries per launch on fp16 rows of <= 512 elements, register chain (scan_wide.hip)
//   W1        65+ queries per launch on 768-element fp16 rows, dump (scan_w1.hip)
enum class Family { Classic, TileBest, Wide, W1 };

constexpr int kSlabF16 = 0, kSlabI8 = 1;   // CRS_SLAB_F16 / CRS_SLAB_I8 (include/crs_hip.h)

// elements per slab row: dim padded to the MFMA k-step of the slab type
constexpr int row_elems(int dim, int slab_type) {
  const int g = slab_type == kSlabI8 ? 256 : 128;
  return dim <= 0 ? 0 : (dim + g - 1) / g * g;
}
constexpr bool f16_row(int pdim) { return pdim >= 128 && pdim <= 1024 && pdim % 128 == 0; }

// ---- Classic (scan.hip) and its int8 twin -------------------------------------------------------------------------------------
// staging variant (CRS_SCAN_VARIANT): 0 register-staged double buffer, 3 the same with asm early loads, 2 LDS-DMA double buffer
// (two workgroups per CU each); 1 LDS-DMA ring, one workgroup per CU
constexpr int classic_wg_per_cu(int variant) { return variant == 1 ? 1 : 2; }
constexpr int classic_tile_rows(int pdim) { return pdim <= 512 ? 32 : 16; }
constexpr int classic_list_slots(int k) { return k <= 16 ? 16 : 32; }   // the L of scan_f16_kernel / scan_i8_kernel
constexpr int kClassicQueries = 64;
constexpr bool classic_form_exists(int pdim, int list_slots) { return f16_row(pdim) && (list_slots == 16 || list_slots == 32); }

// ---- TileBest on fp16 rows (scan_tb.hip) -------------------------------------------------------------------------------------
constexpr int tb_tile_rows(int pdim) { return classic_tile_rows(pdim); }
// 8 waves need a tile that splits into whole 16-byte loads over 512 threads (not 640- / 896-element rows)
constexpr bool scan_tb_has_8_waves(int pdim) { return pdim != 640 && pdim != 896; }
// resident workgroups per CU the kernel is built for (LDS and a 512 / waves-per-SIMD register budget): one look-ahead tile per
// workgroup and two workgroups per CU -- 48 KB in flight per CU is where a plain sweep of HBM peaks as well; a second look-ahead
// tile or a third workgroup only lengthen the memory queues (C4: 5.6-5.8 TB/s against 6.05).  128-element rows (8 KB tiles) take
// three.
constexpr int tb_wg_per_cu(int pdim, int nw) { return nw == 8 ? (pdim <= 384 ? 2 : 1) : (pdim <= 128 ? 3 : 2); }
constexpr int tb_queries(int nw) { return 16 * nw; }
// list slots per lane a chain is instantiated for (>= k), k <= 32; the wide kernel's partial lists are 2 * this wide
constexpr int scan_wide_slots(int k) { return k <= 4 ? 4 : k <= 10 ? 10 : k <= 16 ? 16 : k <= 24 ? 24 : 32; }
// chain length for 16 < k <= 64 on long streams (0: none -- the threshold kernels take the search).  Register budgets checked by
// tools/check_resources.py (no plan-selectable instantiation may touch scratch): 32 slots (64 registers) fit beside the query
// fragments of every row length at two waves per SIMD; 64 slots fit 256-element rows only (384: 20 bytes / lane of scratch),
// 56 / 48 slots 384-element rows, 48 slots 512 / 640, 40 slots (the reference's 2 k = 40 with rerank on) 768
constexpr int scan_tb_long_chain_slots(int pdim, int nw, int k) {
  if (nw != 4 || k <= 16 || k > 64) return 0;
  if (k <= 24) return 24;
  if (k <= 32) return 32;
  if (pdim == 256) return 64;
  if (pdim == 384) return k <= 48 ? 48 : (k <= 56 ? 56 : 0);
  if (pdim == 512 || pdim == 640) return k <= 48 ? 48 : 0;
  if (pdim == 768) return k <= 40 ? 40 : 0;
  return 0;
}
// slots: 0 dump, 4 / 10 / 16 chain (either wave count), 24 .. 64 long chain (4 waves, where scan_tb_long_chain_slots gives it)
constexpr bool tb_form_exists(int pdim, int nw, int slots) {
  if (!f16_row(pdim) || !(nw == 4 || (nw == 8 && scan_tb_has_8_waves(pdim)))) return false;
  if (slots == 0 || slots == 4 || slots == 10 || slots == 16) return true;
  return slots > 16 && scan_tb_long_chain_slots(pdim, nw, slots) == slots;
}

// ---- TileBest on int8 rows (scan_i8.hip; slots = -1 is its Classic form) -----------------------------------------------------
constexpr int i8_tile_rows() { return 32; }
constexpr int kI8Queries = 64;
// (a 64-slot chain spills at these row lengths; 48 covers the reference's 2 k = 40)
constexpr int scan_i8_long_chain_slots(int pdim, int k) { return (k <= 16 || k > 48) ? 0 : k <= 32 ? 32 : (pdim <= 768 ? 48 : 0); }
constexpr bool i8_form_exists(int pdim, int slots) {
  if (!(pdim == 256 || pdim == 512 || pdim == 768 || pdim == 1024)) return false;
  if (slots == -1 || slots == 0 || slots == 4 || slots == 10 || slots == 16) return true;
  return slots > 16 && scan_i8_long_chain_slots(pdim, slots) == slots;
}

// ---- Wide (scan_wide.hip) ----------------------------------------------------------------------------------------------------
// k <= 16 on rows of <= 512 elements, k <= 32 on rows of <= 384 (no scratch in any of them: profiles/r07_wide_resources.txt)
constexpr bool wide_serves(int k, int pdim) { return k <= 32 && pdim <= 512 && !(k > 16 && pdim > 384); }
// rows per tile: the 8-wave kernel takes 64-row tiles where the registers allow
constexpr int scan_wide_tile_rows(int nw, int pdim) { return (nw == 8 && pdim <= 384) ? 64 : 32; }
// resident workgroups per CU: the query fragments cost D/4 registers per lane -> two waves per SIMD
constexpr int scan_wide_wg_per_cu(int nw) { return nw == 8 ? 1 : 2; }
constexpr int wide_queries(int nw) { return 32 * nw; }
// the 24- / 32-slot forms carry the non-temporal slab stream and the ticketed tile schedule (ScanArgs::nt / ticket)
constexpr bool scan_wide_streamed(int k) { return scan_wide_slots(k) > 16; }
// The forms that exist in both MFMA shapes (scan_wide.hip header: "16x16x32 form"): the split-list forms of the 8-wave kernel on
// 256- and 384-element rows, i.e. what a sweep group launches.
constexpr bool wide_has_16(int pdim, int nw, int slots) { return nw == 8 && (pdim == 256 || pdim == 384) && slots > 16; }
// MFMA shape of a form that exists in both: what measured faster by wall time on random data, the shapes alternated on one
// device, every run of the one ahead of every run of the other and the medians at least 5 x the larger spread apart
// (profiles/r13_bench_c4_ab.jsonl, profiles/r13_forms_ab.jsonl).  384-element rows cleared that at
// both chain lengths; 256-element rows were 5 - 8 % faster on 16x16x32 but within 1.4 - 3.2 x the spread, and stay.
constexpr int wide_default_mfma(int pdim, int slots) { return (pdim == 384 && (slots == 24 || slots == 32)) ? 16 : 32; }
// mfma: 32 (32x32x16, every form) or 16 (16x16x32, where wide_has_16)
constexpr bool wide_form_exists(int pdim, int nw, int slots, int mfma) {
  if (!(pdim == 128 || pdim == 256 || pdim == 384 || pdim == 512) || !(nw == 4 || nw == 8)) return false;
  if (!(slots == 4 || slots == 10 || slots == 16 || ((slots == 24 || slots == 32) && pdim <= 384))) return false;
  return mfma == 32 || (mfma == 16 && wide_has_16(pdim, nw, slots));
}

// Ring form (scan_wide.hip header: "Ring form"; the kernels live in scan_wide_ring.hip): three tile buffers, the transfer of the
// tile after next issued off-phase per wave half, a raw barrier.  On for the forms measured faster with it by the rule of DESIGN.md
// section 7 item 6 -- none so far beyond the flagship's; -DCRS_WIDE_RING_ALL=1 compiles it into every 8-wave split form (A/B builds).
#ifndef CRS_WIDE_RING_ALL
#define CRS_WIDE_RING_ALL 0
#endif
constexpr bool wide_ring_form(int pdim, int nw, int slots, int mfma) {
  if (!wide_form_exists(pdim, nw, slots, mfma) || nw != 8 || slots <= 16) return false;
  if (CRS_WIDE_RING_ALL) return true;
  return pdim == 384 && slots == 24 && mfma == 16;
}
// dynamic LDS of a launch: the tile buffers (two; ring: three), the last of which also stages the prologue's query transpose
// (4 KB per wave) while it is still idle
constexpr int scan_wide_lds_bytes(int pdim, int nw, bool ring) {
  const int tile = scan_wide_tile_rows(nw, pdim) * pdim * 2, qstage = nw * 4096, nbuf = ring ? 3 : 2;
  return nbuf * tile > (nbuf - 1) * tile + qstage ? nbuf * tile : (nbuf - 1) * tile + qstage;
}

// ---- W1 (scan_w1.hip): 256 queries per workgroup, 8 waves, one workgroup per CU ---------------------------------------------
constexpr int kW1TileRows = 32, kW1WgPerCu = 1, kW1Queries = 256;
constexpr bool w1_form_exists(int pdim) { return pdim == 768; }

}  // namespace crs
