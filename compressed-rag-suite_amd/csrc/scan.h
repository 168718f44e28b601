// Internal (C++) declarations shared by the HIP translation units of libcrs_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_forms.h"

namespace crs {

// capi.hip: the thread-local message of crs_last_error.  set_error returns `code`; launch_status turns hipGetLastError() after the
// launches of `what` into CRS_OK or CRS_EHIP ("what: <HIP's text>")
int set_error(int code, const char* msg);
int launch_status(const char* what);

struct ScanArgs {
  const _Float16* q;      // [nq, D] fp16, zero padded to D
  const void* slab;       // [n_rows, D] fp16 (or int8)
  const float* scales;    // int8 slabs: one fp32 per row, else nullptr
  float* part_scores;     // [nq, nwg, kp]
  int* part_rows;         // [nq, nwg, kp] local row index (tile-best kernels: first row of the tile), -1 = empty
  unsigned* tau_shared;   // [nq] order-preserving uint of the best published k-th score (0 = none); may be null
  unsigned long long* stamps;  // diagnostics only (tools/scan_probe); nullptr in the product path
  int n_rows;
  int n_tiles;
  int nq;
  int k;
  int sched;              // synchronous-compaction schedule: 0 none, 1 {3,4,6,8,12,...}, 2 {4,8,16,...}
  int boot;               // 1: bootstrap the threshold from the first 64 rows in registers (scan.hip)
  int kp;                 // slots per (query, workgroup) partial list (plan.h: k, tiles per stream, or chain slots)
  int nwg;                // tile streams (workgroups per query block)
  int nqb;                // query blocks (64, 128 or 256 queries each); the grid is nqb * nwg workgroups (scan_common.h: grid mapping)
  unsigned* ticket;       // scan_tb.hip chain mode: tiles >= t_dyn are handed out through this counter (zero at launch); else nullptr
  int t_dyn;              //   first dynamically scheduled tile (a multiple of nwg, >= 2 nwg, ring kernels >= 3 nwg); n_tiles when the schedule is static
  int dyn_mask;           //   a ticket stands for dyn_mask + 1 consecutive tiles (a power of two)
  int nt;                 // scan_tb.hip / scan_i8.hip: 1 = slab tiles streamed with the non-temporal policy (lds_dma16_nt)
  int no_stagger;         // scan_wide.hip, 24- / 32-slot forms: 1 = CRS_WIDE_STAGGER=0 (read by nothing else)
  int no_defer;           // scan_wide.hip, the forms of wide_defer<>: 1 = CRS_WIDE_DEFER=0, the chain runs on every tile (read by nothing else)
};

// the exactness workspace of a batch (capi.hip carves it): per-query escalation threshold and row counter, the escalation
// kernel's "blocks through" counter, and the per-query row lists [nq, cap]
struct ExactWs {
  float* thr;
  int* cnt;
  int* done;
  int64_t* lists;
};

// scan_refine.hip: re-open the k winning tiles (16, 32 or 64 rows each) per query, re-score, rank
int refine_launch(const _Float16* q16, int nq, int pdim, const _Float16* slab, int n_rows, const float* win_s,
                  const int64_t* win, int k, int tile_rows, int64_t id_base, float* out_s, int64_t* out_i, hipStream_t stream);

int refine_i8_launch(const _Float16* q16, int nq, int pdim, const void* slab, const float* scales, int n_rows, const float* win_s,
                     const int64_t* win, int k, int tile_rows, int64_t id_base, float* out_s, int64_t* out_i, hipStream_t stream);

// The scan launchers (scan.hip, scan_i8.hip, scan_tb.hip, scan_wide.hip, scan_w1.hip): the form comes from a Plan (plan.h), i.e. it
// satisfies its family's form_exists (scan_forms.h).  Each returns hipError_t as int, -1 for a form that does not exist.
int scan_launch_f16(const ScanArgs& a, int pdim, int variant, hipStream_t stream);   // variant: Knobs::scan_variant
// slots: -1 threshold kernel; 0 tile-best dump; else tile-best chain (finished by merge + refine_i8_launch)
int scan_launch_i8(const ScanArgs& a, int pdim, int slots, hipStream_t stream);
// tile-best 16x16x32 scan; nw = 4 (64 queries / workgroup) or 8 (128); slots = 0: dump mode (kp = tiles per stream), else chain
// mode (kp = slots); finished by merge + refine_launch
int scan_launch_tb(const ScanArgs& a, int pdim, int nw, int slots, hipStream_t stream);
int scan_ticket_zero(unsigned* ticket, hipStream_t stream);   // ScanArgs::ticket := 0, in stream order
// 65+ queries per launch, fp16 slabs; mfma: 16 or 32, the MFMA shape (Plan::mfma)
int scan_launch_wide(const ScanArgs& a, int pdim, int nw, int mfma, hipStream_t stream);
// the ring kernels of the same forms (scan_wide_ring.hip; Plan::ring, i.e. wide_ring_form holds)
int scan_launch_wide_ring(const ScanArgs& a, int pdim, int nw, int mfma, hipStream_t stream);
// 65+ queries per launch on 768-element fp16 rows: 256 queries per workgroup, dump selection
int scan_launch_w1(const ScanArgs& a, int pdim, hipStream_t stream);

// merge.hip
// inter_s / inter_i: [nq, merge_slices(nlists, k_in), k_out] scratch of the two-level form (> 8192 candidates per query);
// null = always one level
int merge_slices(int nlists, int k_in);
int merge_launch_i32(const float* scores, const int* rows, int nlists, int nq, int k_in, int k_out,
                     int64_t id_base, float* out_scores, int64_t* out_ids, float* inter_s, int64_t* inter_i, hipStream_t stream);
int merge_launch_i64(const float* scores, const int64_t* ids, int nlists, int nq, int k_in, int k_out,
                     float* out_scores, int64_t* out_ids, hipStream_t stream);

int merge_launch_wire(const void* wire, size_t block_bytes, size_t scores_off, int nlists, int nq, int k_in, int k_out,
                      float* out_scores, int64_t* out_ids, hipStream_t stream);

// merge_sorted.hip: lists that arrive sorted (score desc, id asc, empty slots last), k_in / k_out <= CRS_MAX_K_CERT, nlists <= 64
int merge_sorted_launch_i64(const float* scores, const int64_t* ids, int nlists, int nq, int k_in, int k_out, float* out_scores,
                            int64_t* out_ids, hipStream_t stream);
int merge_sorted_launch_wire(const void* wire, size_t block_bytes, size_t scores_off, int nlists, int nq, int k_in, int k_out,
                             float* out_scores, int64_t* out_ids, hipStream_t stream);

// mmr.hip: greedy MMR ordering of lists of <= CRS_MAX_K shadow rows, one workgroup per list
int mmr_order_launch(const float* vecs, int64_t n_rows, int dim, const int64_t* rows, const double* rel, const int* counts, int nq,
                     int m_max, double lam, int* order, hipStream_t stream);

// rerank.hip: score, threshold and lexical re-rank of lists of <= CRS_MAX_K candidates, one wave per list
int rerank_lexical_launch(const float* scores, const int64_t* rows, int nq, int m_max, const int64_t* doc_off, const int* doc_tok,
                          int64_t n_rows, int64_t n_doc_tok, const int64_t* q_off, const int* q_tok, int64_t n_q_tok, const int* q_norm,
                          int k, double threshold, int* order, int* out_count, double* sim, double* rr, int* reranked, hipStream_t stream);

// bm25.hip: exact BM25 top-k of <= 64 queries over the token CSR: pair table, scan (one wave per workgroup), merge
size_t bm25_workspace_bytes(int nq, int k, int64_t n_rows);
int bm25_topk_launch(const int64_t* doc_off, const int* doc_tok, const int* doc_tf, const int* doc_len, int64_t n_rows, int64_t n_doc_tok,
                     const int64_t* q_off, const int* q_tok, const float* q_w, int nq, int n_pairs, float c0, float c1, float k1p1, int k,
                     void* workspace, float* out_s, int64_t* out_i, hipStream_t stream);

// sparse_scan.hip: exact impact (dot product) top-k of <= 64 queries over a weighted token CSR: bm25.hip's scan with another term
size_t sparse_workspace_bytes(int nq, int k, int64_t n_rows);
int sparse_topk_launch(const int64_t* doc_off, const int* doc_tok, const float* doc_w, int64_t n_rows, int64_t n_doc_tok,
                       const int64_t* q_off, const int* q_tok, const float* q_w, int nq, int n_pairs, int k, void* workspace, float* out_s,
                       int64_t* out_i, hipStream_t stream);
// sparse_compact.hip: dense non-negative weight rows -> the <= cap largest (id, weight) per row in id order, one workgroup per row
int sparse_compact_launch(const float* weights, int batch, int V, int Vp, int cap, const int* skip_ids, int n_skip, int* out_ids,
                          float* out_w, int* counts, hipStream_t stream);

// fuse.hip: reciprocal rank fusion of a dense and a lexical list of <= CRS_MAX_K rows each, one wave per query
int fuse_rrf_launch(const int64_t* dense, int m_dense, const int64_t* lex, int m_lex, int nq, double c, double w_dense, double w_lex,
                    int k_out, int64_t* out_rows, double* out_fused, int* out_dpos, int* out_lpos, int* out_count, hipStream_t stream);

// wordpiece.hip: BERT basic tokenisation + WordPiece (or the hash rule) of UTF-8 texts, one workgroup per text
int wordpiece_encode_launch(const uint8_t* text, const int64_t* offsets, int n_texts, int64_t n_bytes, const uint32_t* table,
                            int64_t table_len, const uint32_t* rep, int64_t rep_len, const int32_t* slots, int64_t n_slots,
                            const uint32_t* pool, int64_t pool_len, int max_probe, int lmax, int mode, int unk, int cls, int sep, int pad,
                            int hash_lo, int hash_span, int max_len, int* ids, int* lens, int* flags, hipStream_t stream);
// unigram.hip: SentencePiece Unigram (normaliser table, Metaspace words, fp64 Viterbi) of UTF-8 texts, one workgroup per text
int unigram_encode_launch(const uint8_t* text, const int64_t* offsets, int n_texts, int64_t n_bytes, const uint32_t* table,
                          int64_t table_len, const uint32_t* rep, int64_t rep_len, const int32_t* slots, const double* slot_scores,
                          int64_t n_slots, const uint32_t* pool, int64_t pool_len, int max_probe, int lmax, double unk_score, int opts,
                          int unk, int cls, int sep, int pad, int max_len, int* ids, int* lens, int* flags, hipStream_t stream);

// token_match.hip: BERTScore's greedy matching of pairs of token-state matrices, one workgroup per pair
int token_match_launch(const float* a, const int* len_a, int seq_a, const float* b, const int* len_b, int seq_b, int n_pairs, int hidden,
                       const float* w_a, const float* w_b, float* out, hipStream_t stream);

// maxsim.hip: late-interaction scores of [nq, m_max] candidate rows over a token-vector CSR, one wave per pair; -1 = bad dimp
int maxsim_launch(const void* q16, const int* q_len, int nq, int lq_max, const void* tok16, const int64_t* offsets, int64_t n_rows,
                  int64_t n_tokens, const int64_t* rows, int m_max, int dimp, float* out, hipStream_t stream);
// token_project.hip: hidden states -> packed unit-length fp16 token vectors, one wave per 16 tokens; -1 = bad dim
int token_project_launch(const float* hidden, const void* w16, const float* bias, const int64_t* dst, void* out16, int64_t n_tok,
                         int H, int dim, hipStream_t stream);

// join.hip: thresholded self-join of an fp16 slab (pairs i < j with slab score >= thr, 256 x 256 tiles) and the fp32 check of its
// candidates against the shadow, a quarter wave per pair
int pairs_above_launch(const void* slab, int pdim, int64_t a_first, int64_t a_rows, int64_t b_first, int64_t b_rows, float thr,
                       int64_t* pairs_out, float* scores_out, int64_t cap, int64_t* counter, hipStream_t stream);
int pairs_verify_launch(const int64_t* pairs, int64_t m, const float* shadow, int64_t n_rows, int d, float thr, int64_t* rows_a,
                        int64_t* rows_b, float* sims, int64_t* counter, hipStream_t stream);

// convert.hip
int refine_f32_launch(const float* q32, int nq, int dim, const float* shadow, int64_t n_rows, int64_t id_base,
                      const int64_t* cand, int k_in, int k_out, float* out_s, int64_t* out_i, hipStream_t stream);
int score_rows_launch(const float* q32, int nq, int dim, const float* shadow, int64_t n_rows, int64_t id_base, int k, const int64_t* ids,
                      float* scores, hipStream_t stream);
int rescore_launch(const float* q32, int nq, int dim, const float* shadow, int64_t n_rows,
                   int64_t id_base, int k, float* scores, int64_t* ids, hipStream_t stream);

// finish.hip: the tail of a tile-best fp16 scan (merge + tile re-score + fp32 re-rank + certificate) in one kernel; -1 = the plan
// does not fit it (finish_fits)
bool finish_fits(int nlists, int kp, int kc, int tile_rows, int pdim);
int finish_cert_launch(const float* part_s, const int* part_r, int nlists, int kp, const _Float16* q16, int nq, int pdim,
                       const _Float16* slab, int n_rows, int tile_rows, const float* q32, int dim, const float* shadow, int64_t id_base,
                       int kc, int k_out, float err_rows, float* cand_s, int64_t* cand_i, float* out_s, int64_t* out_i, int* status,
                       const ExactWs& ws, hipStream_t stream);

// exact.hip: exactness certificate of the over-fetch re-rank + in-stream escalation of uncertified queries
float exact_err_arith(int dim, int pdim);
float exact_err_rows_bound(int dim, int slab_type);
int refine_cert_launch(const float* q32, const _Float16* q16, int nq, int dim, int pdim, int slab_type, const float* shadow,
                       int64_t n_rows, int64_t id_base, const int64_t* cand, const float* cand_s, int k_in, int k_out,
                       float err_rows, float* out_s, int64_t* out_i, int* status, const ExactWs& ws, hipStream_t stream);
int escalate_launch(const float* q32, const _Float16* q16, int nq, int dim, int pdim, int slab_type, const void* slab,
                    const float* scales, const float* shadow, int64_t n_rows, int64_t id_base, int k_out, float* out_s,
                    int64_t* out_i, int* status, const ExactWs& ws, int cap, int cus, hipStream_t stream);

// large_k.hip: fp32 re-rank + certificate of a partitioned over-fetch, cand / cand_s [parts, nq, 64] (k_out <= 4096 candidates);
// -1 = parts out of 1..large_k_max_parts()
int large_k_max_parts();
int large_cert_launch(const float* q32, const _Float16* q16, int nq, int dim, int pdim, int slab_type, const float* shadow, int64_t n_rows,
                      int64_t id_base, const int64_t* cand, const float* cand_s, int parts, int64_t chunk_rows, int k_out, float err_rows,
                      float* out_s, int64_t* out_i, int* status, const ExactWs& ws, hipStream_t stream);

}  // namespace crs
