// maxsim_scan.h -- the exact late-interaction sweep: limits and the plan of one crs_maxsim_topk call.  Plain C++ (no
// HIP), so the planner (maxsim_scan_plan.cpp) and the kernel (maxsim_scan.hip) share one definition.
//
// A call scores every row of [row_first, row_first + row_count) of a token-vector CSR against nq queries by MaxSim and keeps the k
// best per query.  Queries are served in groups of 8 (one 256-thread workgroup, two queries per wave); the rows are cut into items
// of CRS_MAXSIM_SCAN_ITEM_ROWS consecutive rows and the G workgroups of a query group walk items w, w + G, w + 2 G, ...  Every
// (workgroup, query) leaves a sorted list of kp pairs in the workspace, [G][nq][kp], and merge.hip reduces the G lists to k.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace crs {

constexpr int kMsScanGroupQ = 8;           // queries of a workgroup: two per wave
constexpr int kMsScanThreads = 256;
constexpr int kMsScanCus = 256;            // the CUs G is sized for (MI355X); a fixed number keeps the plan a pure function
constexpr int kMsScanFill = 2;             // workgroups per CU over all query groups (one is resident: two 64 KB buffers at dimp 128)
constexpr int64_t kMsScanMaxRows = ((int64_t)1 << 32) - 1;   // a list entry names its row by 32 bits relative to row_first

struct MaxsimScanPlan {
  int nq, lq_max, dimp, ksteps, k, kp;
  int qgroups;          // ceil(nq / 8): gridDim.y
  int64_t items;        // ceil(row_count / 64)
  int g;                // workgroups per query group: gridDim.x, the merge's nlists
  int lds_bytes;        // two window buffers of 256 tokens
  size_t part_s, part_r, bytes;   // workspace actually used: scores fp32 [g][nq][kp] | rows int64 [g][nq][kp]
};
// returns 0, or -1 with *why naming the argument
int maxsim_scan_make_plan(int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p, const char** why);
int maxsim_scan_plan_describe(const MaxsimScanPlan& p, char* buf, size_t cap);
// An upper bound of plan.bytes that depends on (nq, k, row_count) alone and grows with each of them (g falls as nq grows, so the
// exact size does not): lists = g nq <= min(items nq, 8 * kMsScanFill * kMsScanCus + nq).
size_t maxsim_scan_workspace_bound(int nq, int k, int64_t row_count);

// ---- the same sweep over an fp8 (e4m3) token index (crs_maxsim_topk_f8, maxsim_scan_f8.hip).  The rows are decoded
// to fp16 in registers (maxsim_f8.h), so a query's A fragments take what they take in fp16 and a wave keeps two queries, as the
// fp16 sweep does: 237 VGPRs at dimp 128, no scratch.  A window buffer is 256 rows of dimp BYTES, two of them 64 KB at dimp 128,
// so TWO workgroups share a CU where the fp16 sweep has one.  The plan has the same fields.
constexpr int kMsF8WaveQ = 2;                              // queries resident per wave
constexpr int kMsF8GroupQ = 4 * kMsF8WaveQ;                // queries of a workgroup
int maxsim_scan_f8_make_plan(int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p, const char** why);
int maxsim_scan_f8_plan_describe(const MaxsimScanPlan& p, char* buf, size_t cap);
size_t maxsim_scan_f8_workspace_bound(int nq, int k, int64_t row_count);

// ---- the same sweep over a 2-bit residual token index (crs_maxsim_topk_rc, maxsim_scan_rc.hip).  Queries are fp16
// and a wave keeps two, as above.  A window buffer holds 256 code rows of dimp / 4 bytes, 256 cids and 256 scales -- dimp / 4 + 6
// bytes a token, 9.5 KB at dimp 128, two of them 19 KB; the centroid rows are gathered from global memory into registers and
// never staged.  LDS would let eight workgroups share a CU; the registers (two queries a wave) allow three, two, two and one at
// dimp 32, 64, 96 and 128, so kMsScanFill stays what it is.  The plan has the same fields.
constexpr int kMsRcWaveQ = 2;                              // queries resident per wave
constexpr int kMsRcGroupQ = 4 * kMsRcWaveQ;                // queries of a workgroup
constexpr int kMsRcTokenLdsBytes(int dimp) { return dimp / 4 + 6; }
int maxsim_scan_rc_make_plan(int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p, const char** why);
int maxsim_scan_rc_plan_describe(const MaxsimScanPlan& p, char* buf, size_t cap);
size_t maxsim_scan_rc_workspace_bound(int nq, int k, int64_t row_count);

// ---- the pruned centroid-interaction sweep of a 2-bit residual index (crs_centroid_maxsim_topk, centroid_scan.hip).
// Nothing is multiplied: the sweep streams the cid plane, tests each token's centroid against a per-query keep bitmap held in LDS
// and gathers a row of precomputed centroid scores for the kept tokens only.  A workgroup of kCsThreads threads serves qg queries,
// qg = min(8, kCsBitmapLds / bitmap bytes of a query), and loads their bitmaps once; each of its WAVES walks items of 64 rows
// (wave v of the grid takes items v, v + waves, ...) for all qg queries, and the workgroup's waves merge their lists in LDS
// (where the bitmaps were), so the workspace is [g][nq][kp] as for the other sweeps.
constexpr int kCsThreads = 1024;
constexpr int kCsWaves = kCsThreads / 64;
constexpr int kCsBitmapLds = 128 * 1024;   // of the 160 KB of a CU; one workgroup is resident where the bitmaps fill it
constexpr int kCsCus = 256;

struct CentroidScanPlan {
  int nq, lq_max, lqp, ch;      // lqp = lq_max rounded up to 8; ch = 16-byte chunks of a score row rounded up to a power of two
  int n_centroids, words;       // words = ceil(n_centroids / 32): uint32 words of one query's bitmap
  int k, kp;
  int qg, qgroups;              // queries of a workgroup; ceil(nq / qg): gridDim.y
  int64_t items;                // ceil(row_count / 64)
  int g;                        // workgroups per query group: gridDim.x, the merge's nlists
  int lds_bytes;                // max(qg bitmaps, qg * kCsWaves lists of 64 keys)
  size_t part_s, part_r, bytes;
};
int centroid_scan_make_plan(int nq, int lq_max, int n_centroids, int k, int64_t row_count, CentroidScanPlan* p, const char** why);
int centroid_scan_plan_describe(const CentroidScanPlan& p, char* buf, size_t cap);
// an upper bound of plan.bytes that depends on (nq, k, row_count) alone and grows with each: g nq <= min(items nq, 8 kCsCus + nq)
size_t centroid_scan_workspace_bound(int nq, int k, int64_t row_count);

}  // namespace crs
