// plan.h -- the plan of a search's scan: which kernel family and form sweeps the slab, its geometry and every launch argument
// that does not depend on a pointer.  make_plan is a pure function of the sizes, the CU count and the knobs (plan.cpp: plain
// C++17, no HIP), so tools/plan_table.cpp and tests/test_plan_cpu.py run it without a device.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "scan_forms.h"

namespace crs {

// Every CRS_* knob that planning or launching a scan reads; knobs_from_env() is the only reader.
// "once": read at the first plan of the process and kept; "per call": read at every plan (tests flip these inside one process).
struct Knobs {
  // knob = default           variable               read      meaning
  bool scan_tb = true;      // CRS_SCAN_TB            once      0: threshold / compaction kernels for every search
  bool long_chain = true;   // CRS_SCAN_LONG_CHAIN    once      0: 16 < k <= 64 on long streams back on the threshold kernels
  bool scan_wide = true;    // CRS_SCAN_WIDE          once      0: no scan_wide.hip (65+ queries go to scan_tb.hip)
  bool scan_w1 = true;      // CRS_SCAN_W1            once      0: no scan_w1.hip (768-element rows go to scan_tb.hip)
  int scan_variant = 3;     // CRS_SCAN_VARIANT       once      staging of scan.hip, 0..3 (scan_forms.h: classic_wg_per_cu)
  bool share_tau = false;   // CRS_SCAN_SHARE_TAU     once      1: cross-workgroup threshold sharing (measured slower)
  bool scan_boot = true;    // CRS_SCAN_BOOT          once      0: no threshold bootstrap on short streams (scan.hip)
  int scan_sched = 2;       // CRS_SCAN_SCHED         once      synchronous-compaction schedule 0..2 (ScanArgs::sched)
  int tb_dyn = 85;          // CRS_TB_DYN             per call  percent of a chain stream's tiles drawn from the ticket; 0: static
  int tb_dyn_g = 8;         // CRS_TB_DYN_G           per call  tiles per ticket: 1, 2, 4, 8 or 16
  int tb_dyn_min = 96;      // CRS_TB_DYN_MIN         per call  shortest stream (rounds) that gets a ticket, never below 4 (76 rounds measured no gain)
  bool wide_dyn = true;     // CRS_WIDE_DYN           per call  0: the wide kernel's 24- / 32-slot forms keep the static stride
  int scan_nt = -1;         // CRS_SCAN_NT            per call  0 / 1: non-temporal slab stream off / on; -1: by slab size
  bool fused_tail = true;   // CRS_FUSED_TAIL         per call  0: crs_cosine_topk_cert always takes the three-kernel chain
  bool wide_stagger = true; // CRS_WIDE_STAGGER       per call  0: waves 4..7 of the wide split forms select in step with 0..3
  bool wide_defer = true;   // CRS_WIDE_DEFER         per call  0: the wide split forms insert every tile at once (no pending slot)
  int wide_mfma = 0;        // CRS_WIDE_MFMA          per call  16 / 32: MFMA shape where a wide form has both; 0: the measured one
  bool wide_ring = true;    // CRS_WIDE_RING          per call  0: the wide forms of wide_ring_form() run their two-buffer kernel
};
Knobs knobs_from_env();

constexpr int kW1MaxDump = 256;      // W1 dumps at most this many tiles per (query, stream)

struct Plan {
  Family family;
  int slab_type;     // CRS_SLAB_F16 / CRS_SLAB_I8: with TileBest and Classic, which file launches
  int nq, k;
  int pdim, tile_rows, n_tiles;
  int nwg;           // tile streams (workgroups per query block)
  int nqb;           // query blocks; the grid is nqb * nwg workgroups
  int kp;            // slots per (query, stream) partial list: k (Classic), tiles per stream (dump), chain slots
  int waves;         // waves per workgroup
  int slots;         // TileBest: 0 dump, else chain length; Wide: chain slots per lane pair; Classic: -1
  int variant;       // Classic on fp16 rows: scan.hip's staging variant
  bool share_tau;    // Classic: ScanArgs::tau_shared is used (zeroed ahead of the launch)
  int nt;            // 1: slab tiles streamed non-temporal (TileBest, Wide's streamed forms)
  bool ticket;       // tiles >= t_dyn are handed out through a counter, zeroed ahead of the launch
  int t_dyn, dyn_mask;
  int boot, sched;   // ScanArgs::boot / sched (scan.hip)
  int no_stagger;    // Wide: ScanArgs::no_stagger
  int no_defer;      // Wide: ScanArgs::no_defer
  int mfma;          // Wide: 16 or 32, the MFMA shape launched; else 0
  bool ring;         // Wide: the ring kernel of the form is launched (scan_forms.h: wide_ring_form)
  int lds;           // Wide: dynamic LDS bytes of the launch; else 0
  size_t part_elems; // nwg * nq * kp
  // every family but Classic leaves tile representatives: merge, then scan_refine.hip re-opens the winning tiles
  bool group_best() const { return family != Family::Classic; }
  bool form_exists() const;   // the family's predicate of scan_forms.h on this plan
};

// returns CRS_OK, or the error code with *why set to the message
int make_plan(int nq, int dim, int k, int64_t n_rows, int slab_type, int cus, const Knobs& kn, Plan* p, const char** why);
// "<kernel> streams=.. qblocks=.. kp=..[ nt] + merge[ + refine]"; returns the length written (snprintf)
int plan_describe(const Plan& p, char* buf, size_t cap);

// scan workspace: [shared thresholds (or the tile ticket) | partial scores | partial rows | stage-1 winners (scores, ids) |
// two-level merge scratch (scores, ids): one k-entry list per 8192 candidates of a query (merge.hip)], each 256-byte aligned
struct WsLayout {
  size_t tau, part_s, part_r, win_s, win_i, inter_s, inter_i;   // byte offsets
  size_t tau_bytes, bytes;                                      // of the first block, of all of them
};
size_t inter_lists(size_t part_elems, int nq);   // >= merge_slices(nwg, kp)
WsLayout ws_layout(size_t part_elems, int nq, int k);
// what crs_scan_workspace_bytes answers: covers the plans of both slab types and the largest Classic grid
int plan_workspace_bytes(int nq, int dim, int k, int64_t n_rows, int cus, const Knobs& kn, size_t* bytes, const char** why);

}  // namespace crs
