// maxsim_scan_plan.cpp -- the plan of a late-interaction sweep (maxsim_scan.h): plain C++17, no HIP, runs without a device.
#include "maxsim_scan.h"

#include <stdio.h>

#include "../../include/crs_hip.h"

namespace crs {

static size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
static int kp_of(int k) { return k <= 32 ? 32 : 64; }

// group_q queries per workgroup, token_lds bytes of a window buffer per token
static int make_plan(int group_q, int token_lds, int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p,
                     const char** why) {
  if (lq_max < 1 || lq_max > CRS_MAXSIM_MAX_QUERY) { *why = "lq_max must be in 1..CRS_MAXSIM_MAX_QUERY"; return -1; }
  if (dimp != 32 && dimp != 64 && dimp != 96 && dimp != 128) { *why = "dimp must be 32, 64, 96 or 128"; return -1; }
  if (k < 1 || k > CRS_MAX_K) { *why = "k must be in 1..CRS_MAX_K"; return -1; }
  if (nq < 0 || nq > 65535) { *why = "nq must be in 0..65535"; return -1; }
  if (row_count < 0 || row_count > kMsScanMaxRows) { *why = "row_count must be in 0..2^32 - 1"; return -1; }
  p->nq = nq;
  p->lq_max = lq_max;
  p->dimp = dimp;
  p->ksteps = dimp / 32;
  p->k = k;
  p->kp = kp_of(k);
  p->qgroups = (nq + group_q - 1) / group_q;
  p->items = (row_count + CRS_MAXSIM_SCAN_ITEM_ROWS - 1) / CRS_MAXSIM_SCAN_ITEM_ROWS;
  const int want = p->qgroups ? (kMsScanFill * kMsScanCus + p->qgroups - 1) / p->qgroups : 1;
  p->g = (int)(p->items < want ? p->items : want);
  p->lds_bytes = 2 * CRS_MAXSIM_SCAN_WINDOW * token_lds;
  const size_t lists = (size_t)p->g * nq;
  p->part_s = 0;
  p->part_r = up256(lists * p->kp * 4);
  p->bytes = p->part_r + up256(lists * p->kp * 8);
  return 0;
}

static size_t workspace_bound(int group_q, int nq, int k, int64_t row_count) {
  const size_t items = (size_t)((row_count + CRS_MAXSIM_SCAN_ITEM_ROWS - 1) / CRS_MAXSIM_SCAN_ITEM_ROWS);
  const size_t a = items * (size_t)nq, b = (size_t)group_q * kMsScanFill * kMsScanCus + (size_t)nq;
  const size_t lists = a < b ? a : b;
  return up256(lists * kp_of(k) * 4) + up256(lists * kp_of(k) * 8) + 256;
}

int maxsim_scan_make_plan(int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p, const char** why) {
  return make_plan(kMsScanGroupQ, 2 * dimp, nq, lq_max, dimp, k, row_count, p, why);
}
int maxsim_scan_f8_make_plan(int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p, const char** why) {
  return make_plan(kMsF8GroupQ, dimp, nq, lq_max, dimp, k, row_count, p, why);
}
int maxsim_scan_rc_make_plan(int nq, int lq_max, int dimp, int k, int64_t row_count, MaxsimScanPlan* p, const char** why) {
  return make_plan(kMsRcGroupQ, kMsRcTokenLdsBytes(dimp), nq, lq_max, dimp, k, row_count, p, why);
}

int maxsim_scan_plan_describe(const MaxsimScanPlan& p, char* buf, size_t cap) {
  return snprintf(buf, cap, "maxsim_scan<ksteps=%d> grid=%dx%d threads=%d queries/wave=2 window=%d item_rows=%d items=%lld kp=%d lds=%d + merge x1 (nlists=%d)",
                  p.ksteps, p.g, p.qgroups, kMsScanThreads, CRS_MAXSIM_SCAN_WINDOW, CRS_MAXSIM_SCAN_ITEM_ROWS, (long long)p.items, p.kp,
                  p.lds_bytes, p.g);
}

int maxsim_scan_f8_plan_describe(const MaxsimScanPlan& p, char* buf, size_t cap) {
  return snprintf(buf, cap, "maxsim_scan_f8<dimp=%d> grid=%dx%d threads=%d queries/wave=%d window=%d item_rows=%d items=%lld kp=%d lds=%d + merge x1 (nlists=%d)",
                  p.dimp, p.g, p.qgroups, kMsScanThreads, kMsF8WaveQ, CRS_MAXSIM_SCAN_WINDOW, CRS_MAXSIM_SCAN_ITEM_ROWS,
                  (long long)p.items, p.kp, p.lds_bytes, p.g);
}

int maxsim_scan_rc_plan_describe(const MaxsimScanPlan& p, char* buf, size_t cap) {
  return snprintf(buf, cap, "maxsim_scan_rc<dimp=%d> grid=%dx%d threads=%d queries/wave=%d window=%d item_rows=%d items=%lld kp=%d lds=%d + merge x1 (nlists=%d)",
                  p.dimp, p.g, p.qgroups, kMsScanThreads, kMsRcWaveQ, CRS_MAXSIM_SCAN_WINDOW, CRS_MAXSIM_SCAN_ITEM_ROWS,
                  (long long)p.items, p.kp, p.lds_bytes, p.g);
}

int centroid_scan_make_plan(int nq, int lq_max, int n_centroids, int k, int64_t row_count, CentroidScanPlan* p, const char** why) {
  if (lq_max < 1 || lq_max > CRS_MAXSIM_MAX_QUERY) { *why = "lq_max must be in 1..CRS_MAXSIM_MAX_QUERY"; return -1; }
  if (n_centroids < CRS_RC_MIN_CENTROIDS || n_centroids > CRS_RC_MAX_CENTROIDS) {
    *why = "n_centroids must be in CRS_RC_MIN_CENTROIDS..CRS_RC_MAX_CENTROIDS";
    return -1;
  }
  if (k < 1 || k > CRS_MAX_K) { *why = "k must be in 1..CRS_MAX_K"; return -1; }
  if (nq < 0 || nq > 65535) { *why = "nq must be in 0..65535"; return -1; }
  if (row_count < 0 || row_count > kMsScanMaxRows) { *why = "row_count must be in 0..2^32 - 1"; return -1; }
  p->nq = nq;
  p->lq_max = lq_max;
  p->lqp = (lq_max + 7) & ~7;
  p->ch = 1;
  while (p->ch * 8 < p->lqp) p->ch *= 2;
  p->n_centroids = n_centroids;
  p->words = (n_centroids + 31) / 32;
  p->k = k;
  p->kp = kp_of(k);
  const int fit = kCsBitmapLds / (p->words * 4);      // words <= 2^15: at least one
  p->qg = fit < 8 ? fit : 8;
  p->qgroups = (nq + p->qg - 1) / p->qg;
  p->items = (row_count + CRS_MAXSIM_SCAN_ITEM_ROWS - 1) / CRS_MAXSIM_SCAN_ITEM_ROWS;
  const int64_t want = p->qgroups ? (kCsCus + p->qgroups - 1) / p->qgroups : 1, need = (p->items + kCsWaves - 1) / kCsWaves;
  p->g = (int)(need < want ? need : want);
  const int bitmaps = p->qg * p->words * 4, lists = p->qg * kCsWaves * 64 * 8;
  p->lds_bytes = bitmaps > lists ? bitmaps : lists;
  const size_t n = (size_t)p->g * nq;
  p->part_s = 0;
  p->part_r = up256(n * p->kp * 4);
  p->bytes = p->part_r + up256(n * p->kp * 8);
  return 0;
}

int centroid_scan_plan_describe(const CentroidScanPlan& p, char* buf, size_t cap) {
  return snprintf(buf, cap, "centroid_scan<ch=%d> grid=%dx%d threads=%d Qg=%d bitmap_words=%d lqp=%d item_rows=%d items=%lld kp=%d lds=%d + merge x1 (nlists=%d)",
                  p.ch, p.g, p.qgroups, kCsThreads, p.qg, p.words, p.lqp, CRS_MAXSIM_SCAN_ITEM_ROWS, (long long)p.items, p.kp,
                  p.lds_bytes, p.g);
}

size_t centroid_scan_workspace_bound(int nq, int k, int64_t row_count) {
  const size_t items = (size_t)((row_count + CRS_MAXSIM_SCAN_ITEM_ROWS - 1) / CRS_MAXSIM_SCAN_ITEM_ROWS);
  const size_t a = items * (size_t)nq, b = (size_t)8 * kCsCus + (size_t)nq;
  const size_t lists = a < b ? a : b;
  return up256(lists * kp_of(k) * 4) + up256(lists * kp_of(k) * 8) + 256;
}

size_t maxsim_scan_workspace_bound(int nq, int k, int64_t row_count) { return workspace_bound(kMsScanGroupQ, nq, k, row_count); }
size_t maxsim_scan_f8_workspace_bound(int nq, int k, int64_t row_count) { return workspace_bound(kMsF8GroupQ, nq, k, row_count); }
size_t maxsim_scan_rc_workspace_bound(int nq, int k, int64_t row_count) { return workspace_bound(kMsRcGroupQ, nq, k, row_count); }

}  // namespace crs
