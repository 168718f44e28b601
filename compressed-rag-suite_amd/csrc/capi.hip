// capi.hip -- the extern "C" surface declared in include/crs_hip.h.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "scan.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, const char* detail = "") {
  snprintf(g_err, sizeof g_err, fmt, detail);
  return code;
}
int hip_fail(hipError_t e, const char* where) {
  snprintf(g_err, sizeof g_err, "%s: %s", where, hipGetErrorString(e));
  return CRS_EHIP;
}

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

int device_cus() {
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  if (dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return 0;
    cus[dev] = p.multiProcessorCount > 0 ? p.multiProcessorCount : 256;
  }
  return cus[dev];
}

constexpr int kW1MaxDump = 256;
// streams shorter than this many tiles keep the static stride (1.25 M x 384 rows = 76 tiles per stream measured no gain)
constexpr int kDynMinRounds = 96;

struct Plan {
  int pdim, tile_rows, n_tiles, nwg, kp;   // nwg = tile streams (workgroups per query block)
  int nqb;                                 // query blocks (64 queries each; 32 * wide_nw for the wide kernel)
  int wide_nw;                             // > 0: scan_wide.hip with this many waves per workgroup
  int w1_qg;                               // > 0: scan_w1.hip, this many queries per workgroup (dump selection)
  int i8_tb;                               // 1: scan_i8.hip in a tile-best mode (tb_slots: 0 dump, else chain)
  int tb_nw;                               // > 0: scan_tb.hip with this many waves per workgroup
  int tb_slots;                            //   its chain length (0: dump mode)
  int group_best;                          // 1: the scan leaves tile representatives (scan_refine.hip finishes)
  int nt;                                  // 1: slab tiles streamed non-temporal (scan_tb / scan_i8; scan_nt_policy)
  size_t part_elems;  // nwg * nq * kp
};

// slots per (query, workgroup) partial list: k, or 16 when threshold sharing is on (lists may then be
// dumped unselected)
int partial_width(int k) { return (crs::scan_share_tau() && k <= 16) ? 16 : k; }

bool tb_long_chain() {   // CRS_SCAN_LONG_CHAIN=0: 16 < k <= 64 on long streams back on the threshold kernels (A/B, tests)
  static int v = -1;
  if (v < 0) { const char* e = getenv("CRS_SCAN_LONG_CHAIN"); v = (e && e[0] == '0') ? 0 : 1; }
  return v == 1;
}
// Dynamic tile schedule of the chain-mode tile-best scan (scan_tb.hip): percent of the tiles handed out through the counter and
// tiles per ticket.  Defaults 85 % in granules of 8 (C4 beside the encoder lanes: 44.9 -> 47.2 k q/s on one box; 20 / 50 / 95 / 100 %
// and granules of 4 / 16 measured within 1 % of that or worse; a ticket per tile is bound by the ~90 M atomics/s one address
// takes).  CRS_TB_DYN=0 restores the static stride.  Read per call: tools/tb_dyn_check.py switches it inside one process.
int tb_dyn_percent() {
  const char* e = getenv("CRS_TB_DYN");
  const int v = e ? atoi(e) : 85;
  return v < 0 ? 0 : v > 100 ? 100 : v;
}
int tb_dyn_granule() {
  const char* e = getenv("CRS_TB_DYN_G");
  const int v = e ? atoi(e) : 8;
  return v >= 16 ? 16 : v >= 8 ? 8 : v >= 4 ? 4 : v >= 2 ? 2 : 1;
}
// The same schedule in scan_wide.hip's 24- / 32-slot forms.  CRS_WIDE_DYN=0 keeps their static stride (A/B runs).  Read per call.
bool wide_dyn_enabled() {
  const char* e = getenv("CRS_WIDE_DYN");
  return !(e && e[0] == '0');
}
bool tb_enabled() {   // CRS_SCAN_TB=0: always use the threshold/compaction kernel for <= 64 queries (A/B runs, tests)
  static int v = -1;
  if (v < 0) { const char* e = getenv("CRS_SCAN_TB"); v = (e && e[0] == '0') ? 0 : 1; }
  return v == 1;
}

// The search tail after the scan: finish.hip's one kernel (merge + tile re-score + fp32 re-rank + certificate) where the plan
// fits it, else the three-kernel chain.  CRS_FUSED_TAIL=0 forces the chain (tests compare the two); read per call.
bool fused_tail(const Plan& p, int slab_type, int k_in) {
  return slab_type == CRS_SLAB_F16 && p.group_best && crs::finish_fits(p.nwg, p.kp, k_in, p.tile_rows, p.pdim);
}
bool fused_tail_enabled() {
  const char* e = getenv("CRS_FUSED_TAIL");
  return !(e && e[0] == '0');
}

// scan workspace: [shared thresholds (or the tile ticket) | partial scores | partial rows | stage-1 winners (scores, ids) |
// two-level merge scratch (scores, ids): one k-entry list per 8192 candidates of a query (merge.hip)], each 256-byte aligned
size_t inter_lists(size_t part_elems, int nq) { return part_elems / ((size_t)nq * 4096) + 2; }   // >= merge_slices(nwg, kp)
struct ScanWs {
  unsigned* tau;
  float* part_s;
  int* part_r;
  float* win_s;
  int64_t* win_i;
  float* inter_s;
  int64_t* inter_i;
  size_t tau_bytes, bytes;   // of the first block, of all of them
};
ScanWs scan_ws(void* base, size_t part_elems, int nq, int k) {
  const size_t inter = (size_t)nq * inter_lists(part_elems, nq) * k;
  size_t off = 0;
  auto take = [&](size_t bytes) { const uintptr_t at = (uintptr_t)base + off; off += align_up(bytes, 256); return at; };
  ScanWs w;
  w.tau = reinterpret_cast<unsigned*>(take((size_t)nq * 4));
  w.tau_bytes = off;
  w.part_s = reinterpret_cast<float*>(take(part_elems * 4));
  w.part_r = reinterpret_cast<int*>(take(part_elems * 4));
  w.win_s = reinterpret_cast<float*>(take((size_t)nq * k * 4));
  w.win_i = reinterpret_cast<int64_t*>(take((size_t)nq * k * 8));
  w.inter_s = reinterpret_cast<float*>(take(inter * 4));
  w.inter_i = reinterpret_cast<int64_t*>(take(inter * 8));
  w.bytes = off;
  return w;
}
size_t ws_bytes(size_t part_elems, int nq, int k) { return scan_ws(nullptr, part_elems, nq, k).bytes; }

int make_plan(int nq, int dim, int k, int64_t n_rows, int slab_type, Plan* p) {
  if (nq <= 0 || dim <= 0 || dim > 1024) return fail(CRS_EINVAL, "nq must be > 0 and 0 < dim <= 1024");
  if (k <= 0 || k > CRS_MAX_K) return fail(CRS_EINVAL, "k must be in 1..CRS_MAX_K");
  if (n_rows <= 0 || n_rows > 0x7fffffffLL - 64) return fail(CRS_EINVAL, "n_rows must be in 1..2^31-65");
  const int cus = device_cus();
  if (cus <= 0) return fail(CRS_EHIP, "no HIP device available%s");
  p->pdim = crs_row_elems(dim, slab_type);
  // kernel family: one of the tile-best kernels, or the classic threshold/compaction scan.  The register-chain forms
  // hold k <= 16; the dump form (short streams) has no such limit and serves k <= 64.  For k > 16 the family is
  // therefore only known once the stream length is: plan for tile-best first, fall back to classic if it has to chain.
  bool allow_w1 = true;
  for (int attempt = 0; attempt < 3; ++attempt) {
    const bool allow_tb = attempt < 2 && tb_enabled();
    p->w1_qg = (allow_tb && allow_w1 && slab_type == CRS_SLAB_F16) ? crs::scan_w1_queries_per_wg(nq, k, p->pdim) : 0;
    // (16 < k <= 32 on rows of <= 384 elements too: one launch then serves up to 256 queries per sweep at the re-rank's over-fetch)
    p->wide_nw = (allow_tb && !p->w1_qg && slab_type == CRS_SLAB_F16 && k <= 32) ? crs::scan_wide_waves(nq, k, p->pdim) : 0;
    p->tb_nw = 0;
    if (allow_tb && !p->w1_qg && !p->wide_nw && slab_type == CRS_SLAB_F16)
      p->tb_nw = (nq > 64 && k <= 16 && crs::scan_tb_has_8_waves(p->pdim)) ? 8 : 4;
    p->i8_tb = (allow_tb && slab_type == CRS_SLAB_I8) ? 1 : 0;   // scan_i8.hip's tile-best modes
    p->tile_rows = p->w1_qg ? 32 : p->wide_nw ? crs::scan_wide_tile_rows(p->wide_nw, p->pdim) : slab_type == CRS_SLAB_I8 ? crs::scan_i8_tile_rows() : crs::scan_tile_rows(p->pdim);
    p->n_tiles = (int)((n_rows + p->tile_rows - 1) / p->tile_rows);
    const int cap = cus * (p->w1_qg ? 1 : p->wide_nw ? crs::scan_wide_wg_per_cu(p->wide_nw, p->pdim)
                           : p->tb_nw ? crs::scan_tb_wg_per_cu(p->pdim, p->tb_nw) : crs::scan_wg_per_cu());
    // all query blocks of a tile stream must be co-resident: streams = resident slots / query blocks
    const int qpb = p->w1_qg ? p->w1_qg : p->wide_nw ? 32 * p->wide_nw : p->tb_nw ? 16 * p->tb_nw : 64;
    const int nqb = (nq + qpb - 1) / qpb;
    p->nqb = nqb;
    int streams = cap / nqb;
    if (streams < 1) streams = 1;
    if (nqb > 1 && streams >= 8) streams &= ~7;   // whole rounds over the 8 XCDs (scan_common.h: grid mapping)
    p->nwg = p->n_tiles < streams ? p->n_tiles : streams;
    if (nqb > 1 && p->nwg >= 8) p->nwg &= ~7;
    p->kp = partial_width(k);
    p->group_best = 0;
    p->tb_slots = 0;
    if (p->w1_qg) {                          // dump: every tile's representative goes to the partial list
      p->kp = (p->n_tiles + p->nwg - 1) / p->nwg;
      p->group_best = 1;
      // the dump's workspace and merge input grow with the shard (nq * n_rows / 32 entries): past kW1MaxDump entries per
      // (query, stream) -- 1 M rows x 768 at 256 queries is 123 -- the bounded 8-wave chain kernels take over
      // (10 M x 768 at 256 queries would otherwise be 640 MB of workspace and 312 k candidates per query)
      if (p->kp > kW1MaxDump) { allow_w1 = false; continue; }
    } else if (p->wide_nw) {   // register chain of the K best tile representatives per lane
      p->kp = 2 * crs::scan_wide_slots(k);
      p->group_best = 1;
    } else if (p->tb_nw || p->i8_tb) {
      // short streams: every tile's representative goes straight to the partial list ("dump"; merge.hip's
      // single-pass path takes <= 8192 candidates per query); longer ones keep the K best in registers
      const int tps = (p->n_tiles + p->nwg - 1) / p->nwg;
      p->group_best = 1;
      if ((size_t)tps * p->nwg <= 8192 && tps <= 2 * crs::scan_wide_slots(k)) {
        p->kp = tps;
      } else if (k <= 16) {
        p->tb_slots = crs::scan_wide_slots(k);
        p->kp = p->tb_slots;
      } else if (tb_long_chain() && (p->i8_tb ? crs::scan_i8_long_chain_slots(p->pdim, k) : crs::scan_tb_long_chain_slots(p->pdim, p->tb_nw, k)) > 0) {
        // 16 < k <= 64 on a long stream: the same kernels with a 32- / 64-slot chain instead of the threshold kernels,
        // where that chain fits the register file (CRS_SCAN_LONG_CHAIN=0 restores the threshold kernels)
        p->tb_slots = p->i8_tb ? crs::scan_i8_long_chain_slots(p->pdim, k) : crs::scan_tb_long_chain_slots(p->pdim, p->tb_nw, k);
        p->kp = p->tb_slots;
      } else {
        continue;                            // the threshold kernels
      }
    }
    break;
  }
  p->part_elems = (size_t)p->nwg * nq * p->kp;
  // Non-temporal slab stream: a shard's slab far larger than the 256 MB Infinity Cache is read once per launch and replays
  // from nowhere, so its tiles go nt and stop evicting what the encoder lanes beside the sweep re-read; one query block only
  // (several blocks of a launch read every tile several times).  A 77 MB slab (C2) replays from the cache and keeps the default.
  // CRS_SCAN_NT=0 / 1 forces the policy off / on; read per call.
  const size_t slab_bytes = (size_t)n_rows * p->pdim * (slab_type == CRS_SLAB_I8 ? 1 : 2);
  const char* ne = getenv("CRS_SCAN_NT");
  const bool streamed = p->tb_nw || p->i8_tb || (p->wide_nw && crs::scan_wide_streamed(k));
  p->nt = streamed ? ((ne && ne[0] == '0') ? 0 : (ne && ne[0] == '1') ? 1 : (slab_bytes >= ((size_t)1 << 30) && p->nqb == 1)) : 0;
  return CRS_OK;
}

}  // namespace

namespace crs {
int set_error(int code, const char* msg) {  // shared with enc_capi.hip
  snprintf(g_err, sizeof g_err, "%s", msg);
  return code;
}
}  // namespace crs

extern "C" {

const char* crs_last_error(void) { return g_err; }
int crs_abi_version(void) { return 3; }
int crs_row_elems(int dim, int slab_type) {
  if (dim <= 0) return 0;
  const int g = slab_type == CRS_SLAB_I8 ? 256 : 128;
  return (dim + g - 1) / g * g;
}
int crs_padded_dim(int dim) { return crs_row_elems(dim, CRS_SLAB_F16); }

int crs_slab_append_f32(const float* emb_dev, int64_t n, int dim, int slab_type, void* slab_dev,
                        float* scales_dev, float* shadow_f32_dev, int64_t row0, float* row_err_max_dev, void* stream) {
  if (n < 0 || dim <= 0 || dim > 1024 || row0 < 0) return fail(CRS_EINVAL, "bad n/dim/row0");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  if (n == 0) return CRS_OK;
  if (!emb_dev || !slab_dev) return fail(CRS_EINVAL, "null pointer");
  if (slab_type == CRS_SLAB_I8 && !scales_dev) return fail(CRS_EINVAL, "int8 slab needs scales");
  const int e = crs::slab_append_launch(emb_dev, n, dim, crs_row_elems(dim, slab_type), slab_type, slab_dev,
                                        scales_dev, shadow_f32_dev, row0, row_err_max_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "slab_append") : CRS_OK;
}

int crs_queries_to_f16(const float* q_dev, int nq, int dim, int slab_type, void* q16_dev, void* stream) {
  if (nq < 0 || dim <= 0 || dim > 1024) return fail(CRS_EINVAL, "bad nq/dim");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  if (nq == 0) return CRS_OK;
  if (!q_dev || !q16_dev) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::queries_to_f16_launch(q_dev, nq, dim, crs_row_elems(dim, slab_type),
                                           reinterpret_cast<_Float16*>(q16_dev), (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "queries_to_f16") : CRS_OK;
}

int crs_scan_workspace_bytes(int nq, int dim, int k, int64_t n_rows, size_t* bytes) {
  if (!bytes) return fail(CRS_EINVAL, "null pointer");
  Plan p, p8;
  int rc = make_plan(nq, dim, k, n_rows, CRS_SLAB_F16, &p);
  if (rc) return rc;
  rc = make_plan(nq, dim, k, n_rows, CRS_SLAB_I8, &p8);
  if (rc) return rc;
  // the call does not say which slab type will be searched: cover the plans of both, and the largest grid the
  // threshold kernels can use (resident workgroups), which does not depend on n_rows
  const size_t cap = (size_t)device_cus() * crs::scan_wg_per_cu();
  const size_t classic = ws_bytes(cap * nq * partial_width(k), nq, k);
  size_t planned = ws_bytes(p.part_elems, nq, k);
  const size_t planned8 = ws_bytes(p8.part_elems, nq, k);
  if (planned8 > planned) planned = planned8;
  *bytes = classic > planned ? classic : planned;
  return CRS_OK;
}

static int run_scan(const Plan& p, const void* q16, int nq, int slab_type, const void* slab,
                    const float* scales, int64_t n_rows, int k, const ScanWs& ws, hipStream_t st) {
  const bool share = crs::scan_share_tau();
  if (share) {
    const hipError_t me = hipMemsetAsync(ws.tau, 0, ws.tau_bytes, st);
    if (me != hipSuccess) return (int)me;
  }
  crs::ScanArgs a;
  a.q = reinterpret_cast<const _Float16*>(q16);
  a.slab = slab;
  a.scales = scales;
  a.part_scores = ws.part_s;
  a.part_rows = ws.part_r;
  a.stamps = nullptr;
  a.tau_shared = share ? ws.tau : nullptr;
  a.kp = p.kp;
  {
    static int boot = -1;
    if (boot < 0) { const char* e = getenv("CRS_SCAN_BOOT"); boot = (e && e[0] == '0') ? 0 : 1; }
    {
      static int sched = -1;
      if (sched < 0) { const char* e = getenv("CRS_SCAN_SCHED"); sched = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 2; }
      a.sched = sched;
    }
    // short streams only: the bootstrap pays when a workgroup sees few tiles (see scan.hip)
    a.boot = (boot && p.n_tiles / (p.nwg > 0 ? p.nwg : 1) < 24) ? 1 : 0;
  }
  a.n_rows = (int)n_rows;
  a.n_tiles = p.n_tiles;
  a.nq = nq;
  a.k = k;
  a.nwg = p.nwg;
  a.nqb = p.nqb;
  a.ticket = nullptr;
  a.t_dyn = p.n_tiles;
  a.dyn_mask = 0;
  a.nt = p.nt;
  const bool tb_chain = ((slab_type == CRS_SLAB_F16 && p.tb_nw) || (slab_type == CRS_SLAB_I8 && p.i8_tb && p.pdim <= 768)) && p.tb_slots > 0;
  const bool wide_chain = p.wide_nw && crs::scan_wide_streamed(k) && wide_dyn_enabled();   // scan_wide.hip's 24- / 32-slot forms
  if ((tb_chain || wide_chain) && p.nqb == 1 && !share) {
    // (int8 rows of 1024 elements stay static: those instantiations spill, and the ticket's register must not travel through scratch
    // while its value is in flight)
    // long chain-mode streams: the last tb_dyn_percent() of the tiles are drawn from a counter (scan_tb.hip, scan_i8.hip), which lives in the
    // (otherwise unused) shared-threshold words at the head of the workspace and is zeroed in stream order ahead of the scan
    const int rounds = p.n_tiles / p.nwg, pct = tb_dyn_percent();
    const char* me = getenv("CRS_TB_DYN_MIN");   // tests: dynamic schedule on short streams too
    const int min_rounds = me ? atoi(me) : kDynMinRounds;
    if (pct > 0 && rounds >= (min_rounds < 4 ? 4 : min_rounds)) {
      int stat = (int)((int64_t)rounds * (100 - pct) / 100);
      if (stat < 2) stat = 2;
      a.t_dyn = stat * p.nwg;
      a.ticket = ws.tau;
      a.dyn_mask = tb_dyn_granule() - 1;
      const int ze = crs::scan_ticket_zero(a.ticket, st);
      if (ze) return ze;
    }
  }
  const int e = p.w1_qg ? crs::scan_launch_w1(a, p.pdim, st)
                : p.wide_nw ? crs::scan_launch_wide(a, p.pdim, p.wide_nw, st)
                : (slab_type == CRS_SLAB_I8) ? crs::scan_launch_i8(a, p.pdim, p.i8_tb ? p.tb_slots : -1, st)
                : p.tb_nw ? crs::scan_launch_tb(a, p.pdim, p.tb_nw, p.tb_slots, st)
                               : crs::scan_launch_f16(a, p.pdim, p.nwg, st);
  return e;
}

// the argument checks of a search (scan + tail into out_scores / out_ids) once its plan is made
static int search_args_ok(const Plan& p, const void* q16_dev, int nq, int slab_type, const void* slab_dev, const float* scales_dev, int k,
                          const void* workspace_dev, size_t workspace_bytes, const void* out_scores_dev, const void* out_ids_dev) {
  if (!q16_dev || !slab_dev || !workspace_dev || !out_scores_dev || !out_ids_dev)
    return fail(CRS_EINVAL, "null pointer");
  if (slab_type == CRS_SLAB_I8 && !scales_dev) return fail(CRS_EINVAL, "int8 slab needs scales");
  if (((uintptr_t)q16_dev | (uintptr_t)slab_dev) & 15) return fail(CRS_EINVAL, "q/slab must be 16-byte aligned");
  if (workspace_bytes < ws_bytes(p.part_elems, nq, k)) return fail(CRS_ENOSPC, "workspace too small");
  return CRS_OK;
}

int crs_cosine_topk(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                    const float* scales_dev, int64_t n_rows, int k, int64_t id_base,
                    void* workspace_dev, size_t workspace_bytes, float* out_scores_dev,
                    int64_t* out_ids_dev, void* stream) {
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  Plan p;
  int rc = make_plan(nq, dim, k, n_rows, slab_type, &p);
  if (rc) return rc;
  rc = search_args_ok(p, q16_dev, nq, slab_type, slab_dev, scales_dev, k, workspace_dev, workspace_bytes, out_scores_dev, out_ids_dev);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  ScanWs w = scan_ws(workspace_dev, p.part_elems, nq, k);
  int e = run_scan(p, q16_dev, nq, slab_type, slab_dev, scales_dev, n_rows, k, w, st);
  if (e == -1) return fail(CRS_EINVAL, "unsupported padded dimension");
  if (e) return hip_fail((hipError_t)e, "scan launch");
  if ((size_t)crs::merge_slices(p.nwg, p.kp) > inter_lists(p.part_elems, nq)) w.inter_s = nullptr;   // (cannot happen: see inter_lists)
  if (!p.group_best) {
    e = crs::merge_launch_i32(w.part_s, w.part_r, p.nwg, nq, p.kp, k, id_base, out_scores_dev, out_ids_dev, w.inter_s, w.inter_i, st);
    if (e) return hip_fail((hipError_t)e, "merge launch");
    return CRS_OK;
  }
  // group-best variants: k best representatives (local rows) -> their row groups re-scored and ranked
  e = crs::merge_launch_i32(w.part_s, w.part_r, p.nwg, nq, p.kp, k, 0, w.win_s, w.win_i, w.inter_s, w.inter_i, st);
  if (e) return hip_fail((hipError_t)e, "merge launch");
  e = (slab_type == CRS_SLAB_I8)
          ? crs::refine_i8_launch(reinterpret_cast<const _Float16*>(q16_dev), nq, p.pdim, slab_dev, scales_dev, (int)n_rows, w.win_s,
                                  w.win_i, k, p.tile_rows, id_base, out_scores_dev, out_ids_dev, st)
          : crs::refine_launch(reinterpret_cast<const _Float16*>(q16_dev), nq, p.pdim, reinterpret_cast<const _Float16*>(slab_dev),
                               (int)n_rows, w.win_s, w.win_i, k, p.tile_rows, id_base, out_scores_dev, out_ids_dev, st);
  if (e == -1) return fail(CRS_EINVAL, "unsupported padded dimension");
  if (e) return hip_fail((hipError_t)e, "refine launch");
  return CRS_OK;
}

int crs_merge_topk(const float* scores_dev, const int64_t* ids_dev, int nlists, int nq, int k_in,
                   int k_out, float* out_scores_dev, int64_t* out_ids_dev, void* stream) {
  if (nlists <= 0 || nq <= 0 || k_in <= 0 || k_out <= 0 || k_out > CRS_MAX_K) return fail(CRS_EINVAL, "bad sizes (k_out <= CRS_MAX_K)");
  if (!scores_dev || !ids_dev || !out_scores_dev || !out_ids_dev) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::merge_launch_i64(scores_dev, ids_dev, nlists, nq, k_in, k_out, out_scores_dev,
                                      out_ids_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "merge launch") : CRS_OK;
}

// crs_merge_sorted / crs_merge_sorted_wire: one check of the sizes (merge_sorted.hip: a list fits the threads' registers and
// an LDS group up to CRS_MAX_K_CERT entries; the grid is nq x nlists workgroups)
static bool merge_sorted_sizes_ok(int nlists, int nq, int k_in, int k_out) {
  return nlists >= 1 && nlists <= 64 && nq >= 1 && nq <= 0x7fffffff / 64 && k_in >= 1 && k_in <= CRS_MAX_K_CERT && k_out >= 1 &&
         k_out <= CRS_MAX_K_CERT;
}

int crs_merge_sorted(const float* scores_dev, const int64_t* ids_dev, int nlists, int nq, int k_in,
                     int k_out, float* out_scores_dev, int64_t* out_ids_dev, void* stream) {
  if (!merge_sorted_sizes_ok(nlists, nq, k_in, k_out)) return fail(CRS_EINVAL, "bad sizes (k_in, k_out <= CRS_MAX_K_CERT, nlists <= 64)");
  if (!scores_dev || !ids_dev || !out_scores_dev || !out_ids_dev) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::merge_sorted_launch_i64(scores_dev, ids_dev, nlists, nq, k_in, k_out, out_scores_dev, out_ids_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "merge launch") : CRS_OK;
}

int crs_mmr_order(const float* vecs_dev, int64_t n_rows, int dim, const int64_t* rows_dev, const double* rel_dev,
                  const int32_t* counts_dev, int nq, int m_max, double lam, int32_t* order_dev, void* stream) {
  if (nq < 0 || dim <= 0 || n_rows < 0) return fail(CRS_EINVAL, "bad nq/dim/n_rows");
  if (m_max < 1 || m_max > CRS_MAX_K) return fail(CRS_EINVAL, "bad m_max (1 <= m_max <= CRS_MAX_K)");
  if (!(lam >= 0.0 && lam <= 1.0)) return fail(CRS_EINVAL, "lam must lie in [0, 1]");
  if (!vecs_dev || !rows_dev || !rel_dev || !counts_dev || !order_dev) return fail(CRS_EINVAL, "null pointer");
  if (nq == 0) return CRS_OK;
  const int e = crs::mmr_order_launch(vecs_dev, n_rows, dim, rows_dev, rel_dev, counts_dev, nq, m_max, lam, order_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "mmr_order launch") : CRS_OK;
}

int crs_token_match(const float* a_dev, const int32_t* len_a_dev, int seq_a, const float* b_dev, const int32_t* len_b_dev, int seq_b,
                    int n_pairs, int hidden, const float* w_a_dev, const float* w_b_dev, float* out_dev, void* stream) {
  if (seq_a < 1 || seq_a > 512) return fail(CRS_EINVAL, "seq_a must be in 1..512");
  if (seq_b < 1 || seq_b > 512) return fail(CRS_EINVAL, "seq_b must be in 1..512");
  if (hidden < 64 || hidden > 1024 || hidden % 64) return fail(CRS_EINVAL, "hidden must be a multiple of 64 in 64..1024");
  if (n_pairs < 0) return fail(CRS_EINVAL, "n_pairs must be >= 0");
  if (!a_dev) return fail(CRS_EINVAL, "a_dev is null");
  if (!len_a_dev) return fail(CRS_EINVAL, "len_a_dev is null");
  if (!b_dev) return fail(CRS_EINVAL, "b_dev is null");
  if (!len_b_dev) return fail(CRS_EINVAL, "len_b_dev is null");
  if (!out_dev) return fail(CRS_EINVAL, "out_dev is null");
  if (((uintptr_t)a_dev | (uintptr_t)b_dev) & 15) return fail(CRS_EINVAL, "a_dev / b_dev must be 16-byte aligned");
  if (n_pairs == 0) return CRS_OK;
  const int e = crs::token_match_launch(a_dev, len_a_dev, seq_a, b_dev, len_b_dev, seq_b, n_pairs, hidden, w_a_dev, w_b_dev, out_dev,
                                        (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "token_match launch") : CRS_OK;
}

int crs_rerank_lexical(const float* scores_dev, const int64_t* rows_dev, int nq, int m_max, const int64_t* doc_offsets_dev,
                       const int32_t* doc_tokens_dev, int64_t n_rows, int64_t n_doc_tokens, const int64_t* q_offsets_dev,
                       const int32_t* q_tokens_dev, int64_t n_q_tokens, const int32_t* q_norm_dev, int k, double threshold,
                       int32_t* order_dev, int32_t* count_dev, double* sim_dev, double* rr_dev, int32_t* reranked_dev, void* stream) {
  if (nq < 0 || n_rows < 0 || n_doc_tokens < 0 || n_q_tokens < 0) return fail(CRS_EINVAL, "bad nq/n_rows/n_doc_tokens/n_q_tokens");
  if (m_max < 1 || m_max > CRS_MAX_K) return fail(CRS_EINVAL, "bad m_max (1 <= m_max <= CRS_MAX_K)");
  if (k < 1) return fail(CRS_EINVAL, "bad k (k >= 1)");
  if (!scores_dev || !rows_dev || !doc_offsets_dev || !q_offsets_dev || !q_norm_dev || !order_dev || !count_dev || !sim_dev || !rr_dev ||
      !reranked_dev || (n_doc_tokens > 0 && !doc_tokens_dev) || (n_q_tokens > 0 && !q_tokens_dev))
    return fail(CRS_EINVAL, "null pointer");
  if (nq == 0) return CRS_OK;
  const int e = crs::rerank_lexical_launch(scores_dev, rows_dev, nq, m_max, doc_offsets_dev, doc_tokens_dev, n_rows, n_doc_tokens,
                                           q_offsets_dev, q_tokens_dev, n_q_tokens, q_norm_dev, k, threshold, order_dev, count_dev,
                                           sim_dev, rr_dev, reranked_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "rerank_lexical launch") : CRS_OK;
}

static const char* bm25_sizes_bad(int nq, int k, int64_t n_rows) {
  if (nq < 1 || nq > 64) return "bad nq (1 <= nq <= 64)";
  if (k < 1 || k > CRS_MAX_K) return "bad k (1 <= k <= CRS_MAX_K)";
  if (n_rows < 0 || n_rows >= 0x7fffffffll - 64) return "bad n_rows (0 <= n_rows < 2^31 - 64)";
  return nullptr;
}

int crs_bm25_workspace_bytes(int nq, int k, int64_t n_rows, size_t* bytes) {
  if (!bytes) return fail(CRS_EINVAL, "null pointer");
  if (const char* bad = bm25_sizes_bad(nq, k, n_rows)) return fail(CRS_EINVAL, "%s", bad);
  *bytes = crs::bm25_workspace_bytes(nq, k, n_rows);
  return CRS_OK;
}

int crs_bm25_topk(const int64_t* doc_offsets_dev, const int32_t* doc_tokens_dev, const int32_t* doc_tf_dev, const int32_t* doc_len_dev,
                  int64_t n_rows, int64_t n_doc_tokens, const int64_t* q_offsets_dev, const int32_t* q_tokens_dev,
                  const float* q_weights_dev, int nq, int64_t n_q_tokens, float c0, float c1, float k1p1, int k, void* workspace_dev,
                  size_t workspace_bytes, float* out_scores_dev, int64_t* out_rows_dev, void* stream) {
  if (const char* bad = bm25_sizes_bad(nq, k, n_rows)) return fail(CRS_EINVAL, "%s", bad);
  if (n_doc_tokens < 0) return fail(CRS_EINVAL, "bad n_doc_tokens");
  if (n_q_tokens < 0 || n_q_tokens > CRS_BM25_MAX_PAIRS) return fail(CRS_EINVAL, "bad n_q_tokens (0 <= n_q_tokens <= CRS_BM25_MAX_PAIRS)");
  if (!doc_offsets_dev || !q_offsets_dev || !out_scores_dev || !out_rows_dev || (n_rows > 0 && !doc_len_dev) ||
      (n_doc_tokens > 0 && (!doc_tokens_dev || !doc_tf_dev)) || (n_q_tokens > 0 && (!q_tokens_dev || !q_weights_dev)))
    return fail(CRS_EINVAL, "null pointer");
  if (!workspace_dev || ((uintptr_t)workspace_dev & 255)) return fail(CRS_EINVAL, "workspace must be a 256-byte aligned device pointer");
  if (workspace_bytes < crs::bm25_workspace_bytes(nq, k, n_rows)) return fail(CRS_ENOSPC, "workspace smaller than crs_bm25_workspace_bytes");
  const int e = crs::bm25_topk_launch(doc_offsets_dev, doc_tokens_dev, doc_tf_dev, doc_len_dev, n_rows, n_doc_tokens, q_offsets_dev,
                                      q_tokens_dev, q_weights_dev, nq, (int)n_q_tokens, c0, c1, k1p1, k, workspace_dev, out_scores_dev,
                                      out_rows_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "bm25_topk launch") : CRS_OK;
}

int crs_fuse_rrf(const int64_t* dense_rows_dev, int m_dense, const int64_t* lex_rows_dev, int m_lex, int nq, double c, double w_dense,
                 double w_lex, int k_out, int64_t* rows_dev, double* fused_dev, int32_t* dense_pos_dev, int32_t* lex_pos_dev,
                 int32_t* count_dev, void* stream) {
  if (nq < 0) return fail(CRS_EINVAL, "bad nq");
  if (m_dense < 1 || m_dense > CRS_MAX_K || m_lex < 1 || m_lex > CRS_MAX_K) return fail(CRS_EINVAL, "bad m_dense / m_lex (1 <= m <= CRS_MAX_K)");
  if (k_out < 1 || k_out > 2 * CRS_MAX_K) return fail(CRS_EINVAL, "bad k_out (1 <= k_out <= 2 CRS_MAX_K)");
  if (!(c >= 0.0) || !(c <= 1e300)) return fail(CRS_EINVAL, "c must be finite and >= 0");
  if (!(w_dense >= 0.0 && w_dense <= 1e300 && w_lex >= 0.0 && w_lex <= 1e300)) return fail(CRS_EINVAL, "weights must be finite and >= 0");
  if (!dense_rows_dev || !lex_rows_dev || !rows_dev || !fused_dev || !dense_pos_dev || !lex_pos_dev || !count_dev)
    return fail(CRS_EINVAL, "null pointer");
  if (nq == 0) return CRS_OK;
  const int e = crs::fuse_rrf_launch(dense_rows_dev, m_dense, lex_rows_dev, m_lex, nq, c, w_dense, w_lex, k_out, rows_dev, fused_dev,
                                     dense_pos_dev, lex_pos_dev, count_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "fuse_rrf launch") : CRS_OK;
}

int crs_wordpiece_encode(const uint8_t* text_dev, const int64_t* offsets_dev, int n_texts, int64_t n_bytes, const uint32_t* table_dev,
                         int64_t table_len, const uint32_t* rep_pool_dev, int64_t rep_pool_len, const int32_t* slots_dev, int64_t n_slots,
                         const uint32_t* vocab_pool_dev, int64_t vocab_pool_len, int max_probe, int lmax, int mode, int unk_id, int cls_id,
                         int sep_id, int pad_id, int hash_lo, int hash_span, int max_len, int32_t* ids_dev, int32_t* lens_dev,
                         int32_t* flags_dev, void* stream) {
  if (n_texts < 0 || n_bytes < 0) return fail(CRS_EINVAL, "bad n_texts / n_bytes");
  if (max_len < 2 || max_len > 65536) return fail(CRS_EINVAL, "bad max_len (2 <= max_len <= 65536)");
  if (mode != 0 && mode != 1) return fail(CRS_EINVAL, "bad mode (0 WordPiece, 1 hash)");
  if (table_len < 0 || rep_pool_len < 0 || vocab_pool_len < 0) return fail(CRS_EINVAL, "bad table sizes");
  if (n_slots < 1 || n_slots > (1ll << 30) || (n_slots & (n_slots - 1))) return fail(CRS_EINVAL, "n_slots must be a power of two");
  if (max_probe < 1 || max_probe > n_slots || lmax < 1 || lmax > 100) return fail(CRS_EINVAL, "bad max_probe / lmax (1 <= max_probe <= n_slots, 1 <= lmax <= 100)");
  if (mode == 1 && hash_span < 1) return fail(CRS_EINVAL, "hash_span must be >= 1");
  if (!offsets_dev || !slots_dev || !ids_dev || !lens_dev || !flags_dev || (n_bytes > 0 && !text_dev) || (table_len > 0 && !table_dev) ||
      (rep_pool_len > 0 && !rep_pool_dev) || (vocab_pool_len > 0 && !vocab_pool_dev))
    return fail(CRS_EINVAL, "null pointer");
  if ((uintptr_t)slots_dev & 15) return fail(CRS_EINVAL, "slots must be 16-byte aligned");
  if (n_texts == 0) return CRS_OK;
  const int e = crs::wordpiece_encode_launch(text_dev, offsets_dev, n_texts, n_bytes, table_dev, table_len, rep_pool_dev, rep_pool_len,
                                             slots_dev, n_slots, vocab_pool_dev, vocab_pool_len, max_probe, lmax, mode, unk_id, cls_id,
                                             sep_id, pad_id, hash_lo, hash_span, max_len, ids_dev, lens_dev, flags_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "wordpiece_encode launch") : CRS_OK;
}

int crs_rescore_f32(const float* q32_dev, int nq, int dim, const float* shadow_dev, int64_t n_rows,
                    int64_t id_base, int k, float* scores_dev, int64_t* ids_dev, void* stream) {
  if (nq <= 0 || dim <= 0 || k <= 0 || k > 64 || n_rows <= 0) return fail(CRS_EINVAL, "bad sizes (k <= 64)");
  if (!q32_dev || !shadow_dev || !scores_dev || !ids_dev) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::rescore_launch(q32_dev, nq, dim, shadow_dev, n_rows, id_base, k, scores_dev,
                                    ids_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "rescore launch") : CRS_OK;
}

int crs_score_rows_f32(const float* q32_dev, int nq, int dim, const float* shadow_dev, int64_t n_rows, int64_t id_base, int k,
                       const int64_t* ids_dev, float* scores_dev, void* stream) {
  if (nq <= 0 || dim <= 0 || k <= 0 || n_rows <= 0) return fail(CRS_EINVAL, "bad sizes");
  if (!q32_dev || !shadow_dev || !ids_dev || !scores_dev) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::score_rows_launch(q32_dev, nq, dim, shadow_dev, n_rows, id_base, k, ids_dev, scores_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "score_rows launch") : CRS_OK;
}

int crs_refine_f32(const float* q32_dev, int nq, int dim, const float* shadow_dev, int64_t n_rows,
                   int64_t id_base, const int64_t* cand_ids_dev, int k_in, int k_out,
                   float* out_scores_dev, int64_t* out_ids_dev, void* stream) {
  if (nq <= 0 || dim <= 0 || n_rows <= 0 || k_out <= 0 || k_in < k_out || k_in > CRS_MAX_K)
    return fail(CRS_EINVAL, "bad sizes (1 <= k_out <= k_in <= CRS_MAX_K)");
  if (!q32_dev || !shadow_dev || !cand_ids_dev || !out_scores_dev || !out_ids_dev) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::refine_f32_launch(q32_dev, nq, dim, shadow_dev, n_rows, id_base, cand_ids_dev, k_in, k_out,
                                       out_scores_dev, out_ids_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "refine_f32 launch") : CRS_OK;
}

// exactness workspace: [thresholds f32 [nq] | counters i32 [nq] | the escalation kernel's blocks-through counter (256 B) |
// row lists i64 [nq, cap]]; *bytes = its size
static crs::ExactWs exact_ws_at(void* base, int nq, int cap, size_t* bytes) {
  const size_t col = align_up((size_t)nq * 4, 256), lists = 2 * col + 256;
  const uintptr_t b = (uintptr_t)base;
  if (bytes) *bytes = lists + (size_t)nq * cap * 8;
  return {reinterpret_cast<float*>(b), reinterpret_cast<int*>(b + col), reinterpret_cast<int*>(b + 2 * col), reinterpret_cast<int64_t*>(b + lists)};
}
size_t crs_exact_workspace_bytes(int nq, int cap) {
  size_t bytes = 0;
  if (nq > 0 && cap > 0) exact_ws_at(nullptr, nq, cap, &bytes);
  return bytes;
}
float crs_exact_row_error_bound(int dim, int slab_type) { return crs::exact_err_rows_bound(dim, slab_type); }

// validates the arguments every certificate entry shares and carves the exactness workspace
static int exact_ws(int nq, int dim, int slab_type, int cap, size_t ws_bytes, void* ws, crs::ExactWs* out) {
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  if (nq <= 0 || dim <= 0 || dim > 1024) return fail(CRS_EINVAL, "bad nq/dim");
  if (cap < 64 || cap > CRS_EXACT_MAX_CAP) return fail(CRS_EINVAL, "cap must be in 64..CRS_EXACT_MAX_CAP");
  if (!ws || ((uintptr_t)ws & 15)) return fail(CRS_EINVAL, "exactness workspace must be a 16-byte aligned device pointer");
  size_t need = 0;
  *out = exact_ws_at(ws, nq, cap, &need);
  if (ws_bytes < need) return fail(CRS_ENOSPC, "exactness workspace too small");
  return CRS_OK;
}
// untracked (or NaN) row error: the analytic worst case
static float row_err_or_bound(float row_err_max, int dim, int slab_type) {
  return (row_err_max >= 0.f) ? row_err_max : crs::exact_err_rows_bound(dim, slab_type);
}
// the argument checks of the fp32 re-rank + certificate of k_in <= CRS_MAX_K candidates per query
static int cert_args_ok(int64_t n_rows, int k_in, int k_out, const void* q32_dev, const void* q16_dev, const void* shadow_dev,
                        const void* cand_ids_dev, const void* cand_scores_dev, const void* out_scores_dev, const void* out_ids_dev,
                        const void* status_dev) {
  if (n_rows <= 0 || k_out <= 0 || k_in < k_out || k_in > CRS_MAX_K) return fail(CRS_EINVAL, "bad sizes (1 <= k_out <= k_in <= CRS_MAX_K)");
  if (!q32_dev || !q16_dev || !shadow_dev || !cand_ids_dev || !cand_scores_dev || !out_scores_dev || !out_ids_dev || !status_dev)
    return fail(CRS_EINVAL, "null pointer");
  return CRS_OK;
}

int crs_refine_f32_cert(const float* q32_dev, const void* q16_dev, int nq, int dim, int slab_type, const float* shadow_dev,
                        int64_t n_rows, int64_t id_base, const int64_t* cand_ids_dev, const float* cand_scores_dev, int k_in,
                        int k_out, float row_err_max, float* out_scores_dev, int64_t* out_ids_dev, int32_t* status_dev,
                        void* exact_ws_dev, size_t exact_ws_bytes, int cap, void* stream) {
  crs::ExactWs ws;
  int rc = exact_ws(nq, dim, slab_type, cap, exact_ws_bytes, exact_ws_dev, &ws);
  if (rc) return rc;
  rc = cert_args_ok(n_rows, k_in, k_out, q32_dev, q16_dev, shadow_dev, cand_ids_dev, cand_scores_dev, out_scores_dev, out_ids_dev, status_dev);
  if (rc) return rc;
  const int e = crs::refine_cert_launch(q32_dev, reinterpret_cast<const _Float16*>(q16_dev), nq, dim, crs_row_elems(dim, slab_type),
                                        slab_type, shadow_dev, n_rows, id_base, cand_ids_dev, cand_scores_dev, k_in, k_out,
                                        row_err_or_bound(row_err_max, dim, slab_type), out_scores_dev, out_ids_dev, status_dev, ws,
                                        (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "refine_f32_cert launch") : CRS_OK;
}

int crs_escalate_exact(const float* q32_dev, const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                       const float* scales_dev, const float* shadow_dev, int64_t n_rows, int64_t id_base, int k_out,
                       float* out_scores_dev, int64_t* out_ids_dev, int32_t* status_dev, void* exact_ws_dev,
                       size_t exact_ws_bytes, int cap, void* stream) {
  crs::ExactWs ws;
  int rc = exact_ws(nq, dim, slab_type, cap, exact_ws_bytes, exact_ws_dev, &ws);
  if (rc) return rc;
  if (n_rows <= 0 || n_rows > 0x7fffffffLL - 64 || k_out <= 0 || k_out > CRS_MAX_K_CERT) return fail(CRS_EINVAL, "bad sizes");
  if (k_out > CRS_MAX_K && cap < k_out) return fail(CRS_EINVAL, "k_out above CRS_MAX_K needs cap >= k_out");
  if (!q32_dev || !q16_dev || !slab_dev || !shadow_dev || !out_scores_dev || !out_ids_dev || !status_dev) return fail(CRS_EINVAL, "null pointer");
  if (slab_type == CRS_SLAB_I8 && !scales_dev) return fail(CRS_EINVAL, "int8 slab needs scales");
  if (((uintptr_t)q16_dev | (uintptr_t)slab_dev) & 15) return fail(CRS_EINVAL, "q/slab must be 16-byte aligned");
  const int e = crs::escalate_launch(q32_dev, reinterpret_cast<const _Float16*>(q16_dev), nq, dim, crs_row_elems(dim, slab_type), slab_type,
                                     slab_dev, scales_dev, shadow_dev, n_rows, id_base, k_out, out_scores_dev, out_ids_dev, status_dev,
                                     ws, cap, device_cus(), (hipStream_t)stream);
  if (e == -1) return fail(CRS_EINVAL, "unsupported padded dimension");
  return e ? hip_fail((hipError_t)e, "escalate launch") : CRS_OK;
}

int crs_cosine_topk_cert(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev, const float* scales_dev,
                         int64_t n_rows, int k_in, int64_t id_base, void* workspace_dev, size_t workspace_bytes, float* cand_scores_dev,
                         int64_t* cand_ids_dev, const float* q32_dev, const float* shadow_dev, int k_out, float row_err_max,
                         float* out_scores_dev, int64_t* out_ids_dev, int32_t* status_dev, void* exact_ws_dev, size_t exact_ws_bytes,
                         int cap, void* stream) {
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  Plan p;
  int rc = make_plan(nq, dim, k_in, n_rows, slab_type, &p);
  if (rc) return rc;
  // one set of argument checks for both tails: the search's, then the certificate's
  rc = search_args_ok(p, q16_dev, nq, slab_type, slab_dev, scales_dev, k_in, workspace_dev, workspace_bytes, cand_scores_dev, cand_ids_dev);
  if (rc) return rc;
  crs::ExactWs ews;
  rc = exact_ws(nq, dim, slab_type, cap, exact_ws_bytes, exact_ws_dev, &ews);
  if (rc) return rc;
  rc = cert_args_ok(n_rows, k_in, k_out, q32_dev, q16_dev, shadow_dev, cand_ids_dev, cand_scores_dev, out_scores_dev, out_ids_dev, status_dev);
  if (rc) return rc;
  if (!(fused_tail_enabled() && fused_tail(p, slab_type, k_in))) {   // the chain: scan + merge (+ refine), then the certificate
    rc = crs_cosine_topk(q16_dev, nq, dim, slab_type, slab_dev, scales_dev, n_rows, k_in, id_base, workspace_dev, workspace_bytes,
                         cand_scores_dev, cand_ids_dev, stream);
    if (rc) return rc;
    return crs_refine_f32_cert(q32_dev, q16_dev, nq, dim, slab_type, shadow_dev, n_rows, id_base, cand_ids_dev, cand_scores_dev, k_in,
                               k_out, row_err_max, out_scores_dev, out_ids_dev, status_dev, exact_ws_dev, exact_ws_bytes, cap, stream);
  }
  hipStream_t st = (hipStream_t)stream;
  const ScanWs w = scan_ws(workspace_dev, p.part_elems, nq, k_in);
  int e = run_scan(p, q16_dev, nq, slab_type, slab_dev, scales_dev, n_rows, k_in, w, st);
  if (e == -1) return fail(CRS_EINVAL, "unsupported padded dimension");
  if (e) return hip_fail((hipError_t)e, "scan launch");
  e = crs::finish_cert_launch(w.part_s, w.part_r, p.nwg, p.kp, reinterpret_cast<const _Float16*>(q16_dev), nq, p.pdim,
                              reinterpret_cast<const _Float16*>(slab_dev), (int)n_rows, p.tile_rows, q32_dev, dim, shadow_dev, id_base, k_in,
                              k_out, row_err_or_bound(row_err_max, dim, slab_type), cand_scores_dev, cand_ids_dev, out_scores_dev,
                              out_ids_dev, status_dev, ews, st);
  if (e == -1) return fail(CRS_EINVAL, "unsupported plan for the fused tail");
  return e ? hip_fail((hipError_t)e, "finish launch") : CRS_OK;
}

// ---- certified top-k above CRS_MAX_K (csrc/large_k.hip) ----------------------------------------------------------------------
// workspace: [candidate scores f32 [parts, nq, 64] | candidate ids i64 [parts, nq, 64] | the chunk scans' workspace]
int crs_large_k_plan(int nq, int k_out, int64_t n_rows, int* parts, int64_t* chunk_rows, size_t* cand_bytes) {
  if (!parts || !chunk_rows || !cand_bytes) return fail(CRS_EINVAL, "null pointer");
  if (nq <= 0 || k_out <= 0 || k_out > CRS_MAX_K_CERT) return fail(CRS_EINVAL, "need nq > 0 and 1 <= k_out <= CRS_MAX_K_CERT");
  if (n_rows <= 0 || n_rows > 0x7fffffffLL - 64) return fail(CRS_EINVAL, "n_rows must be in 1..2^31-65");
  int64_t p0 = (k_out + 15) / 16;
  p0 = p0 < 2 ? 2 : p0 > crs::large_k_max_parts() ? crs::large_k_max_parts() : p0;
  const int64_t rows = ((n_rows + p0 - 1) / p0 + 15) / 16 * 16;
  *chunk_rows = rows;
  *parts = (int)((n_rows + rows - 1) / rows);
  const size_t slots = (size_t)*parts * nq * CRS_MAX_K;
  *cand_bytes = align_up(slots * 4, 256) + align_up(slots * 8, 256);
  return CRS_OK;
}

int crs_cosine_topk_large_cert_workspace_bytes(int nq, int dim, int k_out, int64_t n_rows, size_t* bytes) {
  if (!bytes) return fail(CRS_EINVAL, "null pointer");
  int parts;
  int64_t rows;
  size_t cand;
  int rc = crs_large_k_plan(nq, k_out, n_rows, &parts, &rows, &cand);
  if (rc) return rc;
  size_t scan = 0, last = 0;   // the chunks share one scan workspace: the larger of a full chunk's and the last chunk's
  rc = crs_scan_workspace_bytes(nq, dim, CRS_MAX_K, rows < n_rows ? rows : n_rows, &scan);
  if (rc) return rc;
  rc = crs_scan_workspace_bytes(nq, dim, CRS_MAX_K, n_rows - (int64_t)(parts - 1) * rows, &last);
  if (rc) return rc;
  *bytes = cand + (scan > last ? scan : last);
  return CRS_OK;
}

int crs_refine_large_cert(const float* q32_dev, const void* q16_dev, int nq, int dim, int slab_type, const float* shadow_dev,
                          int64_t n_rows, int64_t id_base, const int64_t* cand_ids_dev, const float* cand_scores_dev, int parts,
                          int64_t chunk_rows, int k_out, float row_err_max, float* out_scores_dev, int64_t* out_ids_dev,
                          int32_t* status_dev, void* exact_ws_dev, size_t exact_ws_bytes, int cap, void* stream) {
  crs::ExactWs ws;
  int rc = exact_ws(nq, dim, slab_type, cap, exact_ws_bytes, exact_ws_dev, &ws);
  if (rc) return rc;
  if (n_rows <= 0 || k_out <= 0 || k_out > CRS_MAX_K_CERT) return fail(CRS_EINVAL, "bad sizes (1 <= k_out <= CRS_MAX_K_CERT)");
  if (parts <= 0 || parts > crs::large_k_max_parts() || chunk_rows <= 0 || (int64_t)parts * chunk_rows < n_rows ||
      (int64_t)(parts - 1) * chunk_rows >= n_rows)
    return fail(CRS_EINVAL, "parts x chunk_rows must cover n_rows with 1..64 chunks, none of them empty");
  if (!q32_dev || !q16_dev || !shadow_dev || !cand_ids_dev || !cand_scores_dev || !out_scores_dev || !out_ids_dev || !status_dev)
    return fail(CRS_EINVAL, "null pointer");
  const int e = crs::large_cert_launch(q32_dev, reinterpret_cast<const _Float16*>(q16_dev), nq, dim, crs_row_elems(dim, slab_type), slab_type,
                                       shadow_dev, n_rows, id_base, cand_ids_dev, cand_scores_dev, parts, chunk_rows, k_out,
                                       row_err_or_bound(row_err_max, dim, slab_type), out_scores_dev, out_ids_dev, status_dev, ws,
                                       (hipStream_t)stream);
  if (e == -1) return fail(CRS_EINVAL, "bad parts");
  return e ? hip_fail((hipError_t)e, "large_cert launch") : CRS_OK;
}

int crs_cosine_topk_large_cert(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev, const float* scales_dev,
                               int64_t n_rows, int64_t id_base, void* workspace_dev, size_t workspace_bytes, const float* q32_dev,
                               const float* shadow_dev, int k_out, float row_err_max, float* out_scores_dev, int64_t* out_ids_dev,
                               int32_t* status_dev, void* exact_ws_dev, size_t exact_ws_bytes, int cap, void* stream) {
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  crs::ExactWs ews;
  int rc = exact_ws(nq, dim, slab_type, cap, exact_ws_bytes, exact_ws_dev, &ews);
  if (rc) return rc;
  size_t need = 0;
  rc = crs_cosine_topk_large_cert_workspace_bytes(nq, dim, k_out, n_rows, &need);
  if (rc) return rc;
  if (!q16_dev || !slab_dev || !workspace_dev || !q32_dev || !shadow_dev || !out_scores_dev || !out_ids_dev || !status_dev)
    return fail(CRS_EINVAL, "null pointer");
  if (slab_type == CRS_SLAB_I8 && !scales_dev) return fail(CRS_EINVAL, "int8 slab needs scales");
  if (((uintptr_t)q16_dev | (uintptr_t)slab_dev | (uintptr_t)workspace_dev) & 15) return fail(CRS_EINVAL, "q/slab/workspace must be 16-byte aligned");
  if (workspace_bytes < need) return fail(CRS_ENOSPC, "workspace too small");
  int parts;
  int64_t rows;
  size_t cand;
  rc = crs_large_k_plan(nq, k_out, n_rows, &parts, &rows, &cand);
  if (rc) return rc;
  const size_t slots = (size_t)parts * nq * CRS_MAX_K;
  float* cand_s = reinterpret_cast<float*>(workspace_dev);
  int64_t* cand_i = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(workspace_dev) + align_up(slots * 4, 256));
  char* scan_ws = reinterpret_cast<char*>(workspace_dev) + cand;
  const size_t row_bytes = (size_t)crs_row_elems(dim, slab_type) * (slab_type == CRS_SLAB_I8 ? 1 : 2);
  for (int p = 0; p < parts; ++p) {   // chunk p: rows [lo, lo + n) of the shard, its 64 best into block p of the candidates
    const int64_t lo = (int64_t)p * rows;
    const int64_t n = (n_rows - lo < rows) ? n_rows - lo : rows;
    rc = crs_cosine_topk(q16_dev, nq, dim, slab_type, reinterpret_cast<const char*>(slab_dev) + (size_t)lo * row_bytes,
                         scales_dev ? scales_dev + lo : nullptr, n, CRS_MAX_K, id_base + lo, scan_ws, workspace_bytes - cand,
                         cand_s + (size_t)p * nq * CRS_MAX_K, cand_i + (size_t)p * nq * CRS_MAX_K, stream);
    if (rc) return rc;
  }
  return crs_refine_large_cert(q32_dev, q16_dev, nq, dim, slab_type, shadow_dev, n_rows, id_base, cand_i, cand_s, parts, rows, k_out,
                               row_err_max, out_scores_dev, out_ids_dev, status_dev, exact_ws_dev, exact_ws_bytes, cap, stream);
}

size_t crs_wire_scores_offset(int nq, int k) { return (nq > 0 && k > 0) ? (size_t)nq * k * 8 : 0; }
size_t crs_wire_bytes(int nq, int k) {
  return (nq > 0 && k > 0) ? (size_t)nq * k * 8 + align_up((size_t)nq * k * 4, 8) : 0;
}
int crs_merge_topk_wire(const void* wire_dev, int nlists, int nq, int k_in, int k_out,
                        float* out_scores_dev, int64_t* out_ids_dev, void* stream) {
  if (nlists <= 0 || nq <= 0 || k_in <= 0 || k_out <= 0 || k_out > CRS_MAX_K) return fail(CRS_EINVAL, "bad sizes (k_out <= CRS_MAX_K)");
  if (!wire_dev || !out_scores_dev || !out_ids_dev) return fail(CRS_EINVAL, "null pointer");
  if ((uintptr_t)wire_dev & 7) return fail(CRS_EINVAL, "wire buffer must be 8-byte aligned");
  const int e = crs::merge_launch_wire(wire_dev, crs_wire_bytes(nq, k_in), crs_wire_scores_offset(nq, k_in), nlists, nq,
                                       k_in, k_out, out_scores_dev, out_ids_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "merge launch") : CRS_OK;
}

int crs_merge_sorted_wire(const void* wire_dev, int nlists, int nq, int k_in, int k_out,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream) {
  if (!merge_sorted_sizes_ok(nlists, nq, k_in, k_out)) return fail(CRS_EINVAL, "bad sizes (k_in, k_out <= CRS_MAX_K_CERT, nlists <= 64)");
  if (!wire_dev || !out_scores_dev || !out_ids_dev) return fail(CRS_EINVAL, "null pointer");
  if ((uintptr_t)wire_dev & 7) return fail(CRS_EINVAL, "wire buffer must be 8-byte aligned");
  const int e = crs::merge_sorted_launch_wire(wire_dev, crs_wire_bytes(nq, k_in), crs_wire_scores_offset(nq, k_in), nlists, nq,
                                              k_in, k_out, out_scores_dev, out_ids_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "merge launch") : CRS_OK;
}

int crs_scan_plan_describe(int nq, int dim, int k, int64_t n_rows, int slab_type, char* buf, size_t cap) {
  if (!buf || cap == 0) return fail(CRS_EINVAL, "null buffer");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  Plan p;
  const int rc = make_plan(nq, dim, k, n_rows, slab_type, &p);
  if (rc) return rc;
  char name[96];
  if (p.w1_qg) snprintf(name, sizeof name, "scan_w2_kernel<%d> (%d queries/workgroup, dump)", p.pdim, p.w1_qg);
  else if (p.wide_nw) snprintf(name, sizeof name, "scan_wide_kernel<%d,%d,%d>", p.pdim, p.wide_nw, crs::scan_wide_slots(k));
  else if (p.tb_nw) snprintf(name, sizeof name, "scan_tb_kernel<%d,%d,%d,%d>", p.pdim, p.tile_rows, p.tb_nw, p.tb_slots);
  else if (slab_type == CRS_SLAB_I8) snprintf(name, sizeof name, "scan_i8_kernel<%d,%d,%d,%d>", p.pdim, p.tile_rows, (p.i8_tb || k <= 16) ? 16 : 32, p.i8_tb ? p.tb_slots : -1);
  else snprintf(name, sizeof name, "scan_f16_kernel<%d,%d,%d>", p.pdim, p.tile_rows, k <= 16 ? 16 : 32);
  // the tail crs_cosine_topk_cert takes with this plan (crs_cosine_topk itself always runs merge [+ refine])
  snprintf(buf, cap, "%s streams=%d qblocks=%d kp=%d%s + merge%s; cert tail: %s", name, p.nwg, p.nqb, p.kp, p.nt ? " nt" : "",
           p.group_best ? " + refine" : "", fused_tail(p, slab_type, k) ? "fused" : "chain");
  return CRS_OK;
}

int crs_stream_create_cu_masked(int first_cu, int n_cus, void** stream_out) {
  if (!stream_out || n_cus <= 0 || first_cu < 0) return fail(CRS_EINVAL, "bad CU range / null output");
  const int cus = device_cus();
  if (cus <= 0) return fail(CRS_EHIP, "no HIP device available%s");
  if (first_cu + n_cus > cus) return fail(CRS_EINVAL, "CU range exceeds the device");
  const int words = (cus + 31) / 32;
  uint32_t mask[16] = {0};
  if (words > 16) return fail(CRS_EINVAL, "device has more than 512 CUs");
  for (int c = first_cu; c < first_cu + n_cus; ++c) mask[c >> 5] |= 1u << (c & 31);
  hipStream_t st = nullptr;
  const hipError_t e = hipExtStreamCreateWithCUMask(&st, (uint32_t)words, mask);
  if (e != hipSuccess) return hip_fail(e, "hipExtStreamCreateWithCUMask");
  *stream_out = (void*)st;
  return CRS_OK;
}

int crs_stream_destroy(void* stream) {
  if (!stream) return CRS_OK;
  const hipError_t e = hipStreamDestroy((hipStream_t)stream);
  return e == hipSuccess ? CRS_OK : hip_fail(e, "hipStreamDestroy");
}

int crs_time_cosine_topk(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                         const float* scales_dev, int64_t n_rows, int k, void* workspace_dev,
                         size_t workspace_bytes, float* out_scores_dev, int64_t* out_ids_dev,
                         void* stream, int iters, float* ms_total, float* ms_scan) {
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  Plan p;
  int rc = make_plan(nq, dim, k, n_rows, slab_type, &p);
  if (rc) return rc;
  if (iters <= 0 || !ms_total || !ms_scan) return fail(CRS_EINVAL, "bad iters / null outputs");
  if (workspace_bytes < ws_bytes(p.part_elems, nq, k)) return fail(CRS_ENOSPC, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t e0, e1;
  hipError_t he;
  if ((he = hipEventCreate(&e0)) != hipSuccess) return hip_fail(he, "hipEventCreate");
  if ((he = hipEventCreate(&e1)) != hipSuccess) return hip_fail(he, "hipEventCreate");
  const ScanWs w = scan_ws(workspace_dev, p.part_elems, nq, k);
  // scan kernel alone
  hipEventRecord(e0, st);
  for (int i = 0; i < iters; ++i) {
    const int e = run_scan(p, q16_dev, nq, slab_type, slab_dev, scales_dev, n_rows, k, w, st);
    if (e) { hipEventDestroy(e0); hipEventDestroy(e1); return e == -1 ? fail(CRS_EINVAL, "unsupported padded dimension") : hip_fail((hipError_t)e, "scan launch"); }
  }
  hipEventRecord(e1, st);
  if ((he = hipEventSynchronize(e1)) != hipSuccess) { hipEventDestroy(e0); hipEventDestroy(e1); return hip_fail(he, "scan timing"); }
  float ms = 0.f;
  hipEventElapsedTime(&ms, e0, e1);
  *ms_scan = ms / iters;
  // scan + merge (what one crs_cosine_topk call costs on the device)
  hipEventRecord(e0, st);
  for (int i = 0; i < iters; ++i) {
    rc = crs_cosine_topk(q16_dev, nq, dim, slab_type, slab_dev, scales_dev, n_rows, k, 0, workspace_dev,
                         workspace_bytes, out_scores_dev, out_ids_dev, stream);
    if (rc) { hipEventDestroy(e0); hipEventDestroy(e1); return rc; }
  }
  hipEventRecord(e1, st);
  if ((he = hipEventSynchronize(e1)) != hipSuccess) { hipEventDestroy(e0); hipEventDestroy(e1); return hip_fail(he, "total timing"); }
  hipEventElapsedTime(&ms, e0, e1);
  *ms_total = ms / iters;
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  return CRS_OK;
}

}  // extern "C"
