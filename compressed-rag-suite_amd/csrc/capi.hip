// capi.hip -- the extern "C" surface declared in include/crs_hip.h.
#include "../../include/crs_hip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>

#include "plan.h"
#include "scan.h"

namespace crs {
// CUs of the current device, queried once per device (0: no device); the one CU source of both planners (enc_capi.hip too)
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
}  // namespace crs

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

using crs::device_cus;
using crs::Plan;

// the plan of a search on the current device with the environment's knobs; sets the error text
int plan_for(int nq, int dim, int k, int64_t n_rows, int slab_type, Plan* p) {
  const char* why = "";
  const int rc = crs::make_plan(nq, dim, k, n_rows, slab_type, device_cus(), crs::knobs_from_env(), p, &why);
  return rc ? fail(rc, "%s", why) : CRS_OK;
}

// The search tail after the scan: finish.hip's one kernel (merge + tile re-score + fp32 re-rank + certificate) where the plan
// fits it, else the three-kernel chain.  CRS_FUSED_TAIL=0 forces the chain (tests compare the two).
bool fused_tail(const Plan& p, int k_in) {
  return p.slab_type == CRS_SLAB_F16 && p.group_best() && crs::finish_fits(p.nwg, p.kp, k_in, p.tile_rows, p.pdim);
}

// the scan workspace (plan.h: WsLayout) carved at base
struct ScanWs {
  unsigned* tau;
  float* part_s;
  int* part_r;
  float* win_s;
  int64_t* win_i;
  float* inter_s;
  int64_t* inter_i;
  size_t tau_bytes;
};
ScanWs scan_ws(void* base, const Plan& p) {
  const crs::WsLayout l = crs::ws_layout(p.part_elems, p.nq, p.k);
  char* b = static_cast<char*>(base);
  return {reinterpret_cast<unsigned*>(b + l.tau), reinterpret_cast<float*>(b + l.part_s), reinterpret_cast<int*>(b + l.part_r),
          reinterpret_cast<float*>(b + l.win_s), reinterpret_cast<int64_t*>(b + l.win_i), reinterpret_cast<float*>(b + l.inter_s),
          reinterpret_cast<int64_t*>(b + l.inter_i), l.tau_bytes};
}
size_t ws_bytes(const Plan& p) { return crs::ws_layout(p.part_elems, p.nq, p.k).bytes; }

}  // namespace

namespace crs {
int set_error(int code, const char* msg) {  // shared with enc_capi.hip
  snprintf(g_err, sizeof g_err, "%s", msg);
  return code;
}
int launch_status(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? CRS_OK : hip_fail(e, what);
}
}  // namespace crs

extern "C" {

const char* crs_last_error(void) { return g_err; }
int crs_abi_version(void) { return 3; }
int crs_row_elems(int dim, int slab_type) { return crs::row_elems(dim, slab_type); }
int crs_padded_dim(int dim) { return crs_row_elems(dim, CRS_SLAB_F16); }

int crs_scan_workspace_bytes(int nq, int dim, int k, int64_t n_rows, size_t* bytes) {
  if (!bytes) return fail(CRS_EINVAL, "null pointer");
  const char* why = "";
  const int rc = crs::plan_workspace_bytes(nq, dim, k, n_rows, device_cus(), crs::knobs_from_env(), bytes, &why);
  return rc ? fail(rc, "%s", why) : CRS_OK;
}

// fills the kernel arguments from the plan, zeroes what the plan says is read as zero, and calls the family's launcher
static int run_scan(const Plan& p, const void* q16, const void* slab, const float* scales, int64_t n_rows, const ScanWs& ws, hipStream_t st) {
  if (p.share_tau) {
    const hipError_t me = hipMemsetAsync(ws.tau, 0, ws.tau_bytes, st);
    if (me != hipSuccess) return (int)me;
  }
  crs::ScanArgs a;
  a.q = reinterpret_cast<const _Float16*>(q16);
  a.slab = slab;
  a.scales = scales;
  a.part_scores = ws.part_s;
  a.part_rows = ws.part_r;
  a.tau_shared = p.share_tau ? ws.tau : nullptr;
  a.stamps = nullptr;
  a.n_rows = (int)n_rows;
  a.n_tiles = p.n_tiles;
  a.nq = p.nq;
  a.k = p.k;
  a.sched = p.sched;
  a.boot = p.boot;
  a.kp = p.kp;
  a.nwg = p.nwg;
  a.nqb = p.nqb;
  a.ticket = p.ticket ? ws.tau : nullptr;   // the counter lives in the (then unused) shared-threshold words
  a.t_dyn = p.t_dyn;
  a.dyn_mask = p.dyn_mask;
  a.nt = p.nt;
  a.no_stagger = p.no_stagger;
  a.no_defer = p.no_defer;
  if (p.ticket) {
    const int ze = crs::scan_ticket_zero(a.ticket, st);
    if (ze) return ze;
  }
  switch (p.family) {
    case crs::Family::W1: return crs::scan_launch_w1(a, p.pdim, st);
    case crs::Family::Wide:
      return p.ring ? crs::scan_launch_wide_ring(a, p.pdim, p.waves, p.mfma, st) : crs::scan_launch_wide(a, p.pdim, p.waves, p.mfma, st);
    default: break;
  }
  if (p.slab_type == CRS_SLAB_I8) return crs::scan_launch_i8(a, p.pdim, p.slots, st);
  return p.family == crs::Family::TileBest ? crs::scan_launch_tb(a, p.pdim, p.waves, p.slots, st) : crs::scan_launch_f16(a, p.pdim, p.variant, st);
}

// the argument checks of a search (scan + tail into out_scores / out_ids) once its plan is made
static int search_args_ok(const Plan& p, const void* q16_dev, const void* slab_dev, const float* scales_dev,
                          const void* workspace_dev, size_t workspace_bytes, const void* out_scores_dev, const void* out_ids_dev) {
  if (!q16_dev || !slab_dev || !workspace_dev || !out_scores_dev || !out_ids_dev)
    return fail(CRS_EINVAL, "null pointer");
  if (p.slab_type == CRS_SLAB_I8 && !scales_dev) return fail(CRS_EINVAL, "int8 slab needs scales");
  if (((uintptr_t)q16_dev | (uintptr_t)slab_dev) & 15) return fail(CRS_EINVAL, "q/slab must be 16-byte aligned");
  if (workspace_bytes < ws_bytes(p)) return fail(CRS_ENOSPC, "workspace too small");
  return CRS_OK;
}

int crs_cosine_topk(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                    const float* scales_dev, int64_t n_rows, int k, int64_t id_base,
                    void* workspace_dev, size_t workspace_bytes, float* out_scores_dev,
                    int64_t* out_ids_dev, void* stream) {
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return fail(CRS_EINVAL, "bad slab_type");
  Plan p;
  int rc = plan_for(nq, dim, k, n_rows, slab_type, &p);
  if (rc) return rc;
  rc = search_args_ok(p, q16_dev, slab_dev, scales_dev, workspace_dev, workspace_bytes, out_scores_dev, out_ids_dev);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  ScanWs w = scan_ws(workspace_dev, p);
  int e = run_scan(p, q16_dev, slab_dev, scales_dev, n_rows, w, st);
  if (e == -1) return fail(CRS_EINVAL, "unsupported padded dimension");
  if (e) return hip_fail((hipError_t)e, "scan launch");
  if ((size_t)crs::merge_slices(p.nwg, p.kp) > crs::inter_lists(p.part_elems, nq)) w.inter_s = nullptr;   // (cannot happen: see inter_lists)
  if (!p.group_best()) {
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

int crs_token_project(const float* hidden_dev, const void* w16_dev, const float* bias_dev, const int64_t* dst_dev, void* out16_dev,
                      int64_t n_tok, int hidden, int dim, void* stream) {
  if (dim < 1 || dim > 128) return fail(CRS_EINVAL, "dim must be in 1..128");
  if (hidden < 32 || hidden > 1024 || hidden % 32) return fail(CRS_EINVAL, "hidden must be a multiple of 32 in 32..1024");
  if (n_tok < 0 || n_tok > ((int64_t)1 << 36)) return fail(CRS_EINVAL, "n_tok must be in 0..2^36");
  if (!hidden_dev) return fail(CRS_EINVAL, "hidden_dev is null");
  if (!w16_dev) return fail(CRS_EINVAL, "w16_dev is null");
  if (!dst_dev) return fail(CRS_EINVAL, "dst_dev is null");
  if (!out16_dev) return fail(CRS_EINVAL, "out16_dev is null");
  if (((uintptr_t)hidden_dev | (uintptr_t)w16_dev) & 15) return fail(CRS_EINVAL, "hidden_dev / w16_dev must be 16-byte aligned");
  if (n_tok == 0) return CRS_OK;
  const int e = crs::token_project_launch(hidden_dev, w16_dev, bias_dev, dst_dev, out16_dev, n_tok, hidden, dim, (hipStream_t)stream);
  if (e == -1) return fail(CRS_EINVAL, "unsupported dim");
  return e ? hip_fail((hipError_t)e, "token_project launch") : CRS_OK;
}

int crs_maxsim(const void* q16_dev, const int32_t* q_len_dev, int nq, int lq_max, const void* tok16_dev, const int64_t* offsets_dev,
               int64_t n_rows, int64_t n_tokens, const int64_t* rows_dev, int m_max, int dimp, float* out_dev, void* stream) {
  if (lq_max < 1 || lq_max > CRS_MAXSIM_MAX_QUERY) return fail(CRS_EINVAL, "lq_max must be in 1..CRS_MAXSIM_MAX_QUERY");
  if (dimp != 32 && dimp != 64 && dimp != 96 && dimp != 128) return fail(CRS_EINVAL, "dimp must be 32, 64, 96 or 128");
  if (nq < 0 || nq > 65535) return fail(CRS_EINVAL, "nq must be in 0..65535");
  if (m_max < 1) return fail(CRS_EINVAL, "bad m_max (m_max >= 1)");
  if (n_rows < 0 || n_tokens < 0) return fail(CRS_EINVAL, "bad n_rows/n_tokens");
  if (!q16_dev) return fail(CRS_EINVAL, "q16_dev is null");
  if (!q_len_dev) return fail(CRS_EINVAL, "q_len_dev is null");
  if (!offsets_dev) return fail(CRS_EINVAL, "offsets_dev is null");
  if (!rows_dev) return fail(CRS_EINVAL, "rows_dev is null");
  if (!out_dev) return fail(CRS_EINVAL, "out_dev is null");
  if (n_tokens > 0 && !tok16_dev) return fail(CRS_EINVAL, "tok16_dev is null");
  if (((uintptr_t)q16_dev | (uintptr_t)tok16_dev) & 15) return fail(CRS_EINVAL, "q16_dev / tok16_dev must be 16-byte aligned");
  if (nq == 0) return CRS_OK;
  const int e = crs::maxsim_launch(q16_dev, q_len_dev, nq, lq_max, tok16_dev, offsets_dev, n_rows, n_tokens, rows_dev, m_max, dimp,
                                   out_dev, (hipStream_t)stream);
  if (e == -1) return fail(CRS_EINVAL, "unsupported dimp");
  return e ? hip_fail((hipError_t)e, "maxsim launch") : CRS_OK;
}

int crs_pairs_above_f16(const void* slab_dev, int64_t n_rows, int dim, int64_t a_first, int64_t a_rows, int64_t b_first, int64_t b_rows,
                        float thr, int64_t* pairs_out_dev, float* scores_out_dev, int64_t cap, int64_t* count_dev, void* stream) {
  if (dim < 1 || dim > 1024) return fail(CRS_EINVAL, "bad dim (1 <= dim <= 1024)");
  if (n_rows < 0) return fail(CRS_EINVAL, "bad n_rows (n_rows >= 0)");
  if (a_first < 0 || a_rows < 0 || a_first > n_rows || a_rows > n_rows - a_first) return fail(CRS_EINVAL, "range a leaves [0, n_rows)");
  if (b_first < 0 || b_rows < 0 || b_first > n_rows || b_rows > n_rows - b_first) return fail(CRS_EINVAL, "range b leaves [0, n_rows)");
  if (!(thr == thr) || thr - thr != 0.0f) return fail(CRS_EINVAL, "thr must be finite");
  if (cap < 0) return fail(CRS_EINVAL, "bad cap (cap >= 0)");
  if (!slab_dev) return fail(CRS_EINVAL, "slab_dev is null");
  if (!count_dev) return fail(CRS_EINVAL, "count_dev is null");
  if (cap > 0 && (!pairs_out_dev || !scores_out_dev)) return fail(CRS_EINVAL, "pairs_out_dev / scores_out_dev is null");
  if (((uintptr_t)slab_dev | (uintptr_t)pairs_out_dev) & 15) return fail(CRS_EINVAL, "slab_dev / pairs_out_dev must be 16-byte aligned");
  if ((uintptr_t)count_dev & 7) return fail(CRS_EINVAL, "count_dev must be 8-byte aligned");
  const int64_t n_at = (a_rows + CRS_PAIRS_TILE - 1) / CRS_PAIRS_TILE, n_bt = (b_rows + CRS_PAIRS_TILE - 1) / CRS_PAIRS_TILE;
  if (n_at * ((n_bt + 7) / 8 * 8) > CRS_PAIRS_MAX_TILES) return fail(CRS_EINVAL, "too many tile pairs for one launch (CRS_PAIRS_MAX_TILES): stripe the ranges");
  if (a_rows == 0 || b_rows == 0) return CRS_OK;
  const int e = crs::pairs_above_launch(slab_dev, crs_padded_dim(dim), a_first, a_rows, b_first, b_rows, thr, pairs_out_dev, scores_out_dev,
                                        cap, count_dev, (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "pairs_above launch") : CRS_OK;
}

int crs_pairs_verify_f32(const int64_t* pairs_dev, int64_t m, const float* shadow_f32_dev, int64_t n_rows, int dim, float thr,
                         int64_t* rows_a_dev, int64_t* rows_b_dev, float* sims_dev, int64_t* count_dev, void* stream) {
  if (dim < 1 || dim > 1024) return fail(CRS_EINVAL, "bad dim (1 <= dim <= 1024)");
  if (n_rows < 0) return fail(CRS_EINVAL, "bad n_rows (n_rows >= 0)");
  if (m < 0 || m > (int64_t)1 << 31) return fail(CRS_EINVAL, "bad m (0 <= m <= 2^31)");
  if (!(thr == thr)) return fail(CRS_EINVAL, "thr must not be NaN");
  if (!count_dev) return fail(CRS_EINVAL, "count_dev is null");
  if (m > 0 && (!pairs_dev || !shadow_f32_dev || !rows_a_dev || !rows_b_dev || !sims_dev)) return fail(CRS_EINVAL, "null pointer");
  if ((uintptr_t)pairs_dev & 15) return fail(CRS_EINVAL, "pairs_dev must be 16-byte aligned");
  if ((uintptr_t)count_dev & 7) return fail(CRS_EINVAL, "count_dev must be 8-byte aligned");
  if (m == 0) return CRS_OK;
  const int e = crs::pairs_verify_launch(pairs_dev, m, shadow_f32_dev, n_rows, dim, thr, rows_a_dev, rows_b_dev, sims_dev, count_dev,
                                         (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "pairs_verify launch") : CRS_OK;
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

int crs_sparse_compact(const float* weights_dev, int batch, int vocab, int vp, int cap, const int32_t* skip_ids_dev, int n_skip,
                       int32_t* ids_dev, float* out_weights_dev, int32_t* counts_dev, void* stream) {
  if (batch < 1) return fail(CRS_EINVAL, "bad batch (batch >= 1)");
  if (vocab < 1 || vp < vocab) return fail(CRS_EINVAL, "bad vocab / vp (1 <= vocab <= vp)");
  if (cap < 1 || cap > CRS_SPARSE_MAX_TERMS) return fail(CRS_EINVAL, "bad cap (1 <= cap <= CRS_SPARSE_MAX_TERMS)");
  if (n_skip < 0 || n_skip > CRS_SPARSE_MAX_SKIP) return fail(CRS_EINVAL, "bad n_skip (0 <= n_skip <= CRS_SPARSE_MAX_SKIP)");
  if (!weights_dev || !ids_dev || !out_weights_dev || !counts_dev || (n_skip > 0 && !skip_ids_dev)) return fail(CRS_EINVAL, "null pointer");
  const int e = crs::sparse_compact_launch(weights_dev, batch, vocab, vp, cap, skip_ids_dev, n_skip, ids_dev, out_weights_dev, counts_dev,
                                           (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "sparse_compact launch") : CRS_OK;
}

int crs_sparse_workspace_bytes(int nq, int k, int64_t n_rows, size_t* bytes) {
  if (!bytes) return fail(CRS_EINVAL, "null pointer");
  if (const char* bad = bm25_sizes_bad(nq, k, n_rows)) return fail(CRS_EINVAL, "%s", bad);
  *bytes = crs::sparse_workspace_bytes(nq, k, n_rows);
  return CRS_OK;
}

int crs_sparse_topk(const int64_t* doc_offsets_dev, const int32_t* doc_tokens_dev, const float* doc_weights_dev, int64_t n_rows,
                    int64_t n_doc_tokens, const int64_t* q_offsets_dev, const int32_t* q_tokens_dev, const float* q_weights_dev, int nq,
                    int64_t n_q_tokens, int k, void* workspace_dev, size_t workspace_bytes, float* out_scores_dev,
                    int64_t* out_rows_dev, void* stream) {
  if (const char* bad = bm25_sizes_bad(nq, k, n_rows)) return fail(CRS_EINVAL, "%s", bad);
  if (n_doc_tokens < 0) return fail(CRS_EINVAL, "bad n_doc_tokens");
  if (n_q_tokens < 0 || n_q_tokens > CRS_BM25_MAX_PAIRS) return fail(CRS_EINVAL, "bad n_q_tokens (0 <= n_q_tokens <= CRS_BM25_MAX_PAIRS)");
  if (!doc_offsets_dev || !q_offsets_dev || !out_scores_dev || !out_rows_dev || (n_doc_tokens > 0 && (!doc_tokens_dev || !doc_weights_dev)) ||
      (n_q_tokens > 0 && (!q_tokens_dev || !q_weights_dev)))
    return fail(CRS_EINVAL, "null pointer");
  if (!workspace_dev || ((uintptr_t)workspace_dev & 255)) return fail(CRS_EINVAL, "workspace must be a 256-byte aligned device pointer");
  if (workspace_bytes < crs::sparse_workspace_bytes(nq, k, n_rows)) return fail(CRS_ENOSPC, "workspace smaller than crs_sparse_workspace_bytes");
  const int e = crs::sparse_topk_launch(doc_offsets_dev, doc_tokens_dev, doc_weights_dev, n_rows, n_doc_tokens, q_offsets_dev, q_tokens_dev,
                                        q_weights_dev, nq, (int)n_q_tokens, k, workspace_dev, out_scores_dev, out_rows_dev,
                                        (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "sparse_topk launch") : CRS_OK;
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

int crs_unigram_encode(const uint8_t* text_dev, const int64_t* offsets_dev, int n_texts, int64_t n_bytes, const uint32_t* table_dev,
                       int64_t table_len, const uint32_t* rep_pool_dev, int64_t rep_pool_len, const int32_t* slots_dev,
                       const double* slot_scores_dev, int64_t n_slots, const uint32_t* vocab_pool_dev, int64_t vocab_pool_len,
                       int max_probe, int lmax, double unk_score, int opts, int unk_id, int cls_id, int sep_id, int pad_id, int max_len,
                       int32_t* ids_dev, int32_t* lens_dev, int32_t* flags_dev, void* stream) {
  if (n_texts < 0 || n_bytes < 0) return fail(CRS_EINVAL, "bad n_texts / n_bytes");
  if (max_len < 2 || max_len > 65536) return fail(CRS_EINVAL, "bad max_len (2 <= max_len <= 65536)");
  if (opts < 0 || opts > 15) return fail(CRS_EINVAL, "bad opts (CRS_UNIGRAM_* bits)");
  if (table_len < 0 || rep_pool_len < 0 || vocab_pool_len < 0) return fail(CRS_EINVAL, "bad table sizes");
  if (n_slots < 1 || n_slots > (1ll << 30) || (n_slots & (n_slots - 1))) return fail(CRS_EINVAL, "n_slots must be a power of two");
  if (max_probe < 1 || max_probe > n_slots || lmax < 1 || lmax > CRS_UNIGRAM_MAX_WORD)
    return fail(CRS_EINVAL, "bad max_probe / lmax (1 <= max_probe <= n_slots, 1 <= lmax <= CRS_UNIGRAM_MAX_WORD)");
  if (!(unk_score == unk_score)) return fail(CRS_EINVAL, "unk_score is NaN");
  if (!offsets_dev || !slots_dev || !slot_scores_dev || !ids_dev || !lens_dev || !flags_dev || (n_bytes > 0 && !text_dev) ||
      (table_len > 0 && !table_dev) || (rep_pool_len > 0 && !rep_pool_dev) || (vocab_pool_len > 0 && !vocab_pool_dev))
    return fail(CRS_EINVAL, "null pointer");
  if (((uintptr_t)slots_dev & 15) || ((uintptr_t)slot_scores_dev & 7)) return fail(CRS_EINVAL, "slots must be 16-byte, slot_scores 8-byte aligned");
  if (n_texts == 0) return CRS_OK;
  const int e = crs::unigram_encode_launch(text_dev, offsets_dev, n_texts, n_bytes, table_dev, table_len, rep_pool_dev, rep_pool_len,
                                           slots_dev, slot_scores_dev, n_slots, vocab_pool_dev, vocab_pool_len, max_probe, lmax,
                                           unk_score, opts, unk_id, cls_id, sep_id, pad_id, max_len, ids_dev, lens_dev, flags_dev,
                                           (hipStream_t)stream);
  return e ? hip_fail((hipError_t)e, "unigram_encode launch") : CRS_OK;
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
  int rc = plan_for(nq, dim, k_in, n_rows, slab_type, &p);
  if (rc) return rc;
  // one set of argument checks for both tails: the search's, then the certificate's
  rc = search_args_ok(p, q16_dev, slab_dev, scales_dev, workspace_dev, workspace_bytes, cand_scores_dev, cand_ids_dev);
  if (rc) return rc;
  crs::ExactWs ews;
  rc = exact_ws(nq, dim, slab_type, cap, exact_ws_bytes, exact_ws_dev, &ews);
  if (rc) return rc;
  rc = cert_args_ok(n_rows, k_in, k_out, q32_dev, q16_dev, shadow_dev, cand_ids_dev, cand_scores_dev, out_scores_dev, out_ids_dev, status_dev);
  if (rc) return rc;
  if (!(crs::knobs_from_env().fused_tail && fused_tail(p, k_in))) {   // the chain: scan + merge (+ refine), then the certificate
    rc = crs_cosine_topk(q16_dev, nq, dim, slab_type, slab_dev, scales_dev, n_rows, k_in, id_base, workspace_dev, workspace_bytes,
                         cand_scores_dev, cand_ids_dev, stream);
    if (rc) return rc;
    return crs_refine_f32_cert(q32_dev, q16_dev, nq, dim, slab_type, shadow_dev, n_rows, id_base, cand_ids_dev, cand_scores_dev, k_in,
                               k_out, row_err_max, out_scores_dev, out_ids_dev, status_dev, exact_ws_dev, exact_ws_bytes, cap, stream);
  }
  hipStream_t st = (hipStream_t)stream;
  const ScanWs w = scan_ws(workspace_dev, p);
  int e = run_scan(p, q16_dev, slab_dev, scales_dev, n_rows, w, st);
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
  const int rc = plan_for(nq, dim, k, n_rows, slab_type, &p);
  if (rc) return rc;
  char text[192];
  crs::plan_describe(p, text, sizeof text);
  // the tail crs_cosine_topk_cert takes with this plan (crs_cosine_topk itself always runs merge [+ refine])
  snprintf(buf, cap, "%s; cert tail: %s", text, fused_tail(p, k) ? "fused" : "chain");
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
  int rc = plan_for(nq, dim, k, n_rows, slab_type, &p);
  if (rc) return rc;
  if (iters <= 0 || !ms_total || !ms_scan) return fail(CRS_EINVAL, "bad iters / null outputs");
  if (workspace_bytes < ws_bytes(p)) return fail(CRS_ENOSPC, "workspace too small");
  hipStream_t st = (hipStream_t)stream;
  hipEvent_t e0, e1;
  hipError_t he;
  if ((he = hipEventCreate(&e0)) != hipSuccess) return hip_fail(he, "hipEventCreate");
  if ((he = hipEventCreate(&e1)) != hipSuccess) return hip_fail(he, "hipEventCreate");
  const ScanWs w = scan_ws(workspace_dev, p);
  // scan kernel alone
  hipEventRecord(e0, st);
  for (int i = 0; i < iters; ++i) {
    const int e = run_scan(p, q16_dev, slab_dev, scales_dev, n_rows, w, st);
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
