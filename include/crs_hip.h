/* crs_hip.h -- C ABI of libcrs_hip.so: the MI355X (gfx950) embed -> index -> retrieve hot path.
 *
 * The reference (zahraamselim/compressed-rag-suite) is pure Python; the arithmetic of this path
 * lives in third-party wheels it calls (sentence-transformers / ChromaDB).  Each entry point
 * below names the reference call site it replaces.  All pointers marked "dev" are device (HBM)
 * addresses; no torch types cross this boundary.  `stream` is a hipStream_t passed as void*
 * (NULL = the default stream).  Every function returns 0 on success or a negative CRS_E* code;
 * crs_last_error() returns a thread-local message for the last failure.
 *
 * Nothing here ever falls back to the CPU: a missing GPU is an error.
 */
#ifndef CRS_HIP_H
#define CRS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRS_OK 0
#define CRS_EINVAL (-1)   /* bad argument (shape, alignment, k out of range) */
#define CRS_ENOSPC (-2)   /* workspace too small */
#define CRS_EHIP (-3)     /* HIP runtime error (message has hipGetErrorString) */

#define CRS_MAX_K 64      /* largest k one scan launch selects exactly */

/* Slab element types (the vector store's row format in HBM). */
#define CRS_SLAB_F16 0    /* fp16 unit rows                                   */
#define CRS_SLAB_I8 1     /* int8 rows + one fp32 scale per row (s = max|x|/127) */

const char* crs_last_error(void);
int crs_abi_version(void);

/* Slab rows are zero-padded: fp16 rows to a multiple of 128 elements, int8 rows to a multiple of
 * 256 (both = whole 256-byte groups for the LDS swizzle).  crs_row_elems returns the padded row
 * length for an embedding dimension (fp16: 384 -> 384, 100 -> 128; int8: 768 -> 768, 384 -> 512);
 * crs_padded_dim(dim) == crs_row_elems(dim, CRS_SLAB_F16).  Queries searched against a slab use
 * the slab's row length. */
int crs_row_elems(int dim, int slab_type);
int crs_padded_dim(int dim);

/* ---- index build (csrc/row_build.hip): replaces collection.add(embeddings=...) -- rag/indexing.py:114-119 ------
 * Converts `n` fp32 embedding rows (dev, row stride `dim`) into slab rows starting at row
 * `row0` of `slab` (dev, row stride crs_padded_dim(dim) elements).  Rows are L2-normalised in
 * fp32 first (x / max(||x||, 1e-12)): ChromaDB's cosine space does the same, and it is the
 * identity on already-normalised encoder output (rag/embedding.py:69).  For CRS_SLAB_I8,
 * `scales` (dev fp32, one per slab row) receives max|x|/127 of the normalised row.
 * `shadow_f32` (dev, stride `dim`, may be NULL) receives the normalised fp32 rows for exact
 * re-scoring.
 * `row_err_max` (dev, ONE fp32 that the caller zeroed when it created the slab; may be NULL) is raised to the
 * largest |stored row - normalised fp32 row|_2 seen so far (the stored row being fp16, or int8 * scale):
 * the measured row term of the exactness certificate below (ABI 3). */
int crs_slab_append_f32(const float* emb_dev, int64_t n, int dim, int slab_type, void* slab_dev,
                        float* scales_dev, float* shadow_f32_dev, int64_t row0, float* row_err_max_dev, void* stream);

/* ---- in-place mutation (additive to ABI 3; csrc/row_build.hip, csrc/mutate.hip) -- no reference call site: the reference's ChromaDB collection
 * offers delete / update / upsert, its own code never calls them --------------------------------------------------------------
 * crs_slab_write_rows_f32 is the scatter form of crs_slab_append_f32: row rows[i] (dev int64 [m], distinct, each < n_rows;
 * rows outside [0, n_rows) are skipped) of slab / scales / shadow is rewritten from emb[i] by the SAME kernel and per-row device
 * function as the append, so an updated row equals the same vector appended bit for bit; row_err_max is raised likewise.
 *
 * crs_slab_compact removes the `m` rows dead[0] < dead[1] < ... (dev int64, strictly ascending, all < n_rows) from the arrays
 * of one shard IN PLACE, keeping the order of the others: afterwards rows [0, n_rows - m) of slab, scales (may be NULL),
 * shadow (may be NULL; stride `dim`) and rows_global (dev int64, may be NULL) hold the survivors in their old order; what lies
 * past that is unspecified.  The survivor at destination d comes from source d + j, j = the number of dead rows below it.
 * Rows below dead[0] are not touched; `first_row` (0 <= first_row <= dead[0], 0 when the host does not know dead[0]) lets the
 * call skip the windows below it altogether.  The destination is walked in windows of W rows (W from bounce_bytes); per
 * window one launch gathers the window's source rows into `bounce`, the next copies `bounce` to the window.  Window i + 1
 * reads rows >= (i + 1) W and everything written before lies below that, so STREAM ORDER is the whole ordering argument: no
 * workgroup waits for another.  2 ceil((n_rows - m - first_row) / W) launches, no allocation, no host synchronisation.
 * crs_slab_compact_bounce_bytes is the smallest legal bounce size (a window of 1024 rows of every array); larger = fewer
 * windows.  bounce must be 256-byte aligned. */
int crs_slab_write_rows_f32(const float* emb_dev, const int64_t* rows_dev, int64_t m, int dim, int slab_type, void* slab_dev,
                            float* scales_dev, float* shadow_f32_dev, int64_t n_rows, float* row_err_max_dev, void* stream);
size_t crs_slab_compact_bounce_bytes(int dim, int slab_type, int has_shadow);
int crs_slab_compact(const int64_t* dead_dev, int64_t m, int64_t n_rows, int64_t first_row, int dim, int slab_type, void* slab_dev,
                     float* scales_dev, float* shadow_f32_dev, int64_t* rows_global_dev, void* bounce_dev, size_t bounce_bytes,
                     void* stream);
/* Host arithmetic of the above, for tests and callers that size buffers: rows per window for a bounce size (0 = too small). */
int64_t crs_slab_compact_window_rows(int dim, int slab_type, int has_shadow, size_t bounce_bytes);

/* Query side of the same conversion: fp32 [nq, dim] -> normalised fp16 [nq, crs_row_elems(dim, slab_type)] (the fp16 append
 * without shadow). */
int crs_queries_to_f16(const float* q_dev, int nq, int dim, int slab_type, void* q16_dev, void* stream);

/* ---- inner-product and squared-L2 spaces (additive to ABI 3; csrc/space.hip, row writers in csrc/row_build.hip) -- ChromaDB's hnsw:space 'ip' / 'l2',
 * which the reference's collection accepts (rag/indexing.py:83) --------------------------------------------------------------
 * The scan computes <fp16 query row, slab row>.  A store of one of these spaces keeps ONE scale R = 2^e >= the largest row norm
 * it has seen, as a device fp32 (`norm_scale_dev`, read by the kernels: growing it invalidates no captured graph), and stores
 *     ip:  u = x * (1/R)                                   d' = dim        query q / max(|q|, 1e-12)
 *     l2:  (v, t), v = x * (1/(2R)), t = fl(sum v_i^2)      d' = dim + 1    query (q / R, -1), normalised
 * so that the scan's descending score is the space's ascending distance, every stored row has norm <= 1 and the certificate and the
 * escalation of the cosine path hold as they are, over d' = crs_space_row_dim(dim, space) coordinates (slab rows:
 * crs_row_elems(d', slab_type) elements, shadow rows: d' floats).  Rows are NOT normalised.  `dim` is always the caller's
 * dimension: 1..1024 (ip), 1..1023 (l2).  Coordinates whose scaled value leaves the fp32 normal range are outside every "exact"
 * below.  The cosine space has no entry here: it is the functions above.
 *
 * crs_rows_norm_max raises *norm_max_dev (fp32 the caller zeroed) to the largest |x|_2 of n rows; a norm that is not finite leaves
 * +inf there and sets *flag_dev (int32, may be NULL) to 1.
 * crs_slab_append_space_f32 / crs_slab_write_rows_space_f32 are crs_slab_append_f32 / crs_slab_write_rows_f32 for these spaces:
 * the same arguments plus the scale, the same kernel and per-row device function behind all four (an updated row equals the same
 * vector appended, bit for bit), row_err_max raised over all d' coordinates.  The caller has made *norm_scale_dev a power of two >= every norm of the
 * batch before the call.
 * crs_slab_rescale_space follows a growth of the scale from R to R 2^shift: every shadow row [0, n_rows) is multiplied by
 * 2^-shift (t by 2^-2 shift), the slab row and int8 scale are rebuilt from it by that same per-row function, row_err_max is raised.
 * All of it is exact, so a rescaled row equals the same vector stored under the new scale bit for bit.  One launch.
 * crs_queries_to_space writes the unit fp32 queries q32 [nq, d'] and their scan block q16 [nq, crs_row_elems(d', slab_type)], zero
 * padded: what crs_cosine_topk_cert and its kin take as q32 / q16.
 * crs_space_distances turns a finished list into ChromaDB's distances: for ids [nq, k] (rows + id_base of the view the search ran
 * over; its shadow, n_rows and id_base are passed as to the certificate) and the caller's own queries q [nq, dim] it recovers
 * x = R u (ip) / 2R v (l2) exactly and computes 1 - <q, x> (ip) or sum (q_i - x_i)^2 (l2) in fp32, directly, not from the score;
 * out_dist / out_ids [nq, k] leave ordered by (distance asc, id asc), ids < 0 or outside the view as (+inf, -1) at the tail.
 * 1 <= k <= CRS_MAX_K_CERT; out_ids must not alias ids.  One workgroup per query, no workspace, no host synchronisation. */
#define CRS_SPACE_COSINE 0
#define CRS_SPACE_IP 1
#define CRS_SPACE_L2 2
int crs_space_row_dim(int dim, int space);      /* d' (0: bad arguments) */
int crs_rows_norm_max(const float* emb_dev, int64_t n, int dim, float* norm_max_dev, int32_t* flag_dev, void* stream);
int crs_slab_append_space_f32(const float* emb_dev, int64_t n, int dim, int space, int slab_type, const float* norm_scale_dev,
                              void* slab_dev, float* scales_dev, float* shadow_f32_dev, int64_t row0, float* row_err_max_dev,
                              void* stream);
int crs_slab_write_rows_space_f32(const float* emb_dev, const int64_t* rows_dev, int64_t m, int dim, int space, int slab_type,
                                  const float* norm_scale_dev, void* slab_dev, float* scales_dev, float* shadow_f32_dev, int64_t n_rows,
                                  float* row_err_max_dev, void* stream);
int crs_slab_rescale_space(int64_t n_rows, int dim, int space, int slab_type, int shift, void* slab_dev, float* scales_dev,
                           float* shadow_f32_dev, float* row_err_max_dev, void* stream);
int crs_queries_to_space(const float* q_dev, int nq, int dim, int space, int slab_type, const float* norm_scale_dev, float* q32_dev,
                         void* q16_dev, void* stream);
int crs_space_distances(const float* q_dev, int nq, int dim, int space, const float* shadow_f32_dev, int64_t n_rows, int64_t id_base,
                        const float* norm_scale_dev, const int64_t* ids_dev, int k, float* out_dist_dev, int64_t* out_ids_dev,
                        void* stream);

/* ---- search: replaces collection.query(query_embeddings, n_results) -- rag/indexing.py:171-176
 * Exact cosine top-k of `nq` fp16 queries against `n_rows` slab rows on the current device.
 *   q16_dev   fp16 [nq, pdim]  (pdim = crs_row_elems(dim, slab_type)), unit rows, zero padded
 *   slab_dev  fp16 or int8 [n_rows, pdim]; scales_dev fp32 [n_rows] for CRS_SLAB_I8 else NULL
 *             (int8: the kernel moves each query to 16-bit fixed point, see csrc/scan_i8.hip)
 *   k         1..CRS_MAX_K; if k > n_rows the tail slots are (-inf, -1)
 *   id_base   added to row indices (the shard's first global row)
 *   out_scores fp32 [nq, k] cosine, descending; out_ids int64 [nq, k]; ties -> lower id first
 * Workspace: crs_scan_workspace_bytes() bytes of device memory, contents don't-care. */
int crs_scan_workspace_bytes(int nq, int dim, int k, int64_t n_rows, size_t* bytes);
int crs_cosine_topk(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                    const float* scales_dev, int64_t n_rows, int k, int64_t id_base,
                    void* workspace_dev, size_t workspace_bytes, float* out_scores_dev,
                    int64_t* out_ids_dev, void* stream);

/* ---- multi-shard merge (new: the reference is single process) ------------------------------
 * Merges `nlists` partial results laid out [nlists, nq, k_in] (what an RCCL all-gather of the
 * per-shard crs_cosine_topk outputs delivers) into the global top-k_out per query; slots with
 * id < 0 are ignored.  Same ordering rule. */
int crs_merge_topk(const float* scores_dev, const int64_t* ids_dev, int nlists, int nq, int k_in,
                   int k_out, float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* The same merge for lists that arrive SORTED, for k above CRS_MAX_K (additive to ABI 3; csrc/merge_sorted.hip): what the shards
 * of a store return for top_k 65 .. CRS_MAX_K_CERT (crs_cosine_topk_large_cert + crs_escalate_exact).  Precondition: every list
 * [l, q, :] is already in the order of the results (score desc, id asc) with its empty slots (id < 0, any score) at the tail,
 * and ids >= 0 are distinct across the lists of a query.  The kernel does no arithmetic and no sort: an entry's output slot is
 * its position plus one binary-search count per other list, so out_scores / out_ids [nq, k_out] hold the input's own bits, in
 * the same order, with (-inf, -1) behind the last valid entry.  Lists that break the precondition give an unspecified order,
 * never an access outside the buffers.
 * Limits: 1 <= nlists <= 64, 1 <= k_in <= CRS_MAX_K_CERT, 1 <= k_out <= CRS_MAX_K_CERT; k_out may exceed k_in; nlists == 1 copies
 * or truncates. */
int crs_merge_sorted(const float* scores_dev, const int64_t* ids_dev, int nlists, int nq, int k_in,
                     int k_out, float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* Exact fp32 re-score of candidates: out[i, j] = <q32[i, :], shadow[ids[i, j], :]> for ids >= 0
 * (id_base subtracted first), then each row re-sorted by (score desc, id asc). Used when the
 * store keeps an fp32 shadow and over-fetches (recall vs an exact fp32 ranking). */
int crs_rescore_f32(const float* q32_dev, int nq, int dim, const float* shadow_dev, int64_t n_rows,
                    int64_t id_base, int k, float* scores_dev, int64_t* ids_dev, void* stream);

/* The scoring half alone, for candidate lists of ANY length k (VectorStore.search with top_k > CRS_MAX_K orders them with a
 * device sort): scores[i, j] = <q32[i, :], shadow[ids[i, j] - id_base, :]>; entries with ids < 0 get -inf, entries of other
 * shards are left as they are. */
int crs_score_rows_f32(const float* q32_dev, int nq, int dim, const float* shadow_dev, int64_t n_rows, int64_t id_base, int k,
                       const int64_t* ids_dev, float* scores_dev, void* stream);

/* Over-fetch + exact re-rank in one launch (Recall@10 = 1.0 against the fp32 ranking the
 * reference's ChromaDB collection keeps, rag/indexing.py:114-119).  cand_ids [nq, k_in] are the rows a
 * crs_cosine_topk call with k = k_in >= k_out found in the fp16 / int8 slab; each is re-scored as the fp32
 * dot product <q32[i], shadow[id - id_base]>, the k_in candidates are ranked (score desc, id asc; ids < 0
 * or outside this shard are empty) and the best k_out leave as out_scores fp32 [nq, k_out] / out_ids int64
 * [nq, k_out] (empty slots: -inf, -1).  One workgroup per query; k_out <= k_in <= CRS_MAX_K. */
int crs_refine_f32(const float* q32_dev, int nq, int dim, const float* shadow_dev, int64_t n_rows,
                   int64_t id_base, const int64_t* cand_ids_dev, int k_in, int k_out,
                   float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* ---- exactness certificate + escalation (ABI 3; csrc/exact.hip holds the derivation) ---------------------
 * The reference's store keeps and ranks fp32 rows (rag/indexing.py:114-119,171-176); north_star asks for
 * identical doc-id top-k sets.  crs_refine_f32_cert is crs_refine_f32 plus a per-query PROOF that the re-ranked
 * k_out are the fp32 top-k_out of all n_rows rows, not only of the k_in fetched ones:
 *     status[i] = 0   certified: k_out-th fp32 score > (k_in-th slab score) + eps_i, where eps_i bounds
 *                     |slab score - fp32 score| for query i over every row of the shard (from |q16_i - q32_i|_2,
 *                     measured here, and row_err_max = the value crs_slab_append_f32 tracked; pass a negative
 *                     number to use the analytic worst case crs_exact_row_error_bound instead)
 *     status[i] = 1   not certified (near-ties deeper than the over-fetch, e.g. near-duplicate chunks)
 * cand_scores [nq, k_in] are the slab scores crs_cosine_topk returned with cand_ids; q16 [nq, crs_row_elems] is
 * the query block that scan read, q32 [nq, dim] the unit fp32 queries.
 * crs_escalate_exact then makes every status-1 query exact on the same stream, with no host round trip: one more
 * sweep of the slab lists every row whose slab score is >= (k_out-th fp32 score so far) - eps_i (no row of the true
 * top-k can score lower), and the list is re-ranked in fp32; out_scores / out_ids of those queries are overwritten,
 * certified queries are left alone, and the one kernel's blocks all leave at once when nothing is to do (so the call can sit in a
 * captured graph; the lists are re-ranked by the last block through the sweep -- release fence + counter, no spinning).  A list longer than `cap` rows leaves status[i] = 2: call again with a larger cap
 * (<= CRS_EXACT_MAX_CAP).  Workspace: crs_exact_workspace_bytes(nq, cap) bytes, written by crs_refine_f32_cert and
 * consumed by crs_escalate_exact (same nq, cap).  crs_escalate_exact takes k_out <= CRS_MAX_K, or up to CRS_MAX_K_CERT when
 * cap >= k_out (after crs_cosine_topk_large_cert). */
#define CRS_EXACT_MAX_CAP 13312
size_t crs_exact_workspace_bytes(int nq, int cap);
float crs_exact_row_error_bound(int dim, int slab_type);
int crs_refine_f32_cert(const float* q32_dev, const void* q16_dev, int nq, int dim, int slab_type, const float* shadow_dev,
                        int64_t n_rows, int64_t id_base, const int64_t* cand_ids_dev, const float* cand_scores_dev, int k_in,
                        int k_out, float row_err_max, float* out_scores_dev, int64_t* out_ids_dev, int32_t* status_dev,
                        void* exact_ws_dev, size_t exact_ws_bytes, int cap, void* stream);
int crs_escalate_exact(const float* q32_dev, const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                       const float* scales_dev, const float* shadow_dev, int64_t n_rows, int64_t id_base, int k_out,
                       float* out_scores_dev, int64_t* out_ids_dev, int32_t* status_dev, void* exact_ws_dev,
                       size_t exact_ws_bytes, int cap, void* stream);

/* The scan and the certificate in one call (additive to ABI 3): crs_cosine_topk with k = k_in >= k_out into
 * cand_scores / cand_ids [nq, k_in], then crs_refine_f32_cert of those candidates into out_scores / out_ids [nq, k_out],
 * status and the exactness workspace -- the same outputs, bit for bit, as the two calls.  Where the scan plan ends in tile
 * representatives (tile-best kernels) of an fp16 slab with <= 16 384 candidates per query and rows of <= 640 elements, the
 * merge, the tile re-score, the fp32 re-rank and the certificate run as ONE kernel (csrc/finish.hip) instead of three;
 * other plans (int8 slabs, the threshold kernels, larger lists) take the two calls' kernels.  crs_scan_plan_describe names
 * the tail a plan takes ("cert tail: fused" / "chain").  crs_escalate_exact follows it as it follows crs_refine_f32_cert.
 * workspace: crs_scan_workspace_bytes(nq, dim, k_in, n_rows); exact_ws: crs_exact_workspace_bytes(nq, cap). */
int crs_cosine_topk_cert(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev, const float* scales_dev,
                         int64_t n_rows, int k_in, int64_t id_base, void* workspace_dev, size_t workspace_bytes, float* cand_scores_dev,
                         int64_t* cand_ids_dev, const float* q32_dev, const float* shadow_dev, int k_out, float row_err_max,
                         float* out_scores_dev, int64_t* out_ids_dev, int32_t* status_dev, void* exact_ws_dev, size_t exact_ws_bytes,
                         int cap, void* stream);

/* ---- certified top-k above one scan's 64 (additive to ABI 3; csrc/large_k.hip holds the derivation) -------------------------
 * One scan keeps at most CRS_MAX_K candidates per query.  crs_cosine_topk_large_cert over-fetches by partition instead: the
 * n_rows rows are cut into `parts` contiguous chunks of `chunk_rows` rows (the last one shorter; crs_large_k_plan), each chunk is
 * scanned with crs_cosine_topk at k = 64 on `stream` (no host sync), and one kernel re-scores the parts x 64 candidates in fp32
 * against the shadow, ranks them (score desc, id asc) into out_scores / out_ids [nq, k_out] (empty slots: -inf, -1) and certifies
 * each query as crs_refine_f32_cert does, against the largest (64th slab score + eps_i) of the chunks whose lists do not hold all
 * their rows: status 0 = the fp32 top-k_out of all n_rows rows, 1 = not proven.  It writes the exactness workspace like
 * crs_refine_f32_cert, so crs_escalate_exact (same k_out, cap >= k_out) follows it.  1 <= k_out <= CRS_MAX_K_CERT.
 *   crs_large_k_plan: parts = ceil(n_rows / chunk_rows) with chunk_rows = 16 * ceil(ceil(n_rows / P) / 16) and
 *     P = clamp(ceil(k_out / 16), 2, 64), so parts x 64 <= 4096; cand_bytes = the [parts, nq, 64] candidate block (scores fp32,
 *     ids int64, each 256-byte aligned).  Host arithmetic only.
 *   workspace: crs_cosine_topk_large_cert_workspace_bytes(nq, dim, k_out, n_rows) bytes = cand_bytes + the chunk scans' workspace.
 * crs_refine_large_cert is the kernel alone, for a candidate block the caller holds: cand_ids / cand_scores [parts, nq, 64] as
 * the chunk scans leave them (chunk p covers rows [p chunk_rows, min(n_rows, (p + 1) chunk_rows)) + id_base). */
#define CRS_MAX_K_CERT 1024
int crs_large_k_plan(int nq, int k_out, int64_t n_rows, int* parts, int64_t* chunk_rows, size_t* cand_bytes);
int crs_cosine_topk_large_cert_workspace_bytes(int nq, int dim, int k_out, int64_t n_rows, size_t* bytes);
int crs_cosine_topk_large_cert(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev, const float* scales_dev,
                               int64_t n_rows, int64_t id_base, void* workspace_dev, size_t workspace_bytes, const float* q32_dev,
                               const float* shadow_dev, int k_out, float row_err_max, float* out_scores_dev, int64_t* out_ids_dev,
                               int32_t* status_dev, void* exact_ws_dev, size_t exact_ws_bytes, int cap, void* stream);
int crs_refine_large_cert(const float* q32_dev, const void* q16_dev, int nq, int dim, int slab_type, const float* shadow_dev,
                          int64_t n_rows, int64_t id_base, const int64_t* cand_ids_dev, const float* cand_scores_dev, int parts,
                          int64_t chunk_rows, int k_out, float row_err_max, float* out_scores_dev, int64_t* out_ids_dev,
                          int32_t* status_dev, void* exact_ws_dev, size_t exact_ws_bytes, int cap, void* stream);

/* ---- diversity re-ordering: replaces the greedy MMR loop of ContextRetriever._apply_diversity -- rag/retrieval.py:219-277 ----
 * (additive to ABI 3; csrc/mmr.hip).  Orders `nq` lists of at most m_max <= CRS_MAX_K rows of one shard's fp32 rows in one launch,
 * one workgroup per list, reading the rows in place:
 *   vecs_dev    fp32 [n_rows, dim], the shard's shadow
 *   rows_dev    int64 [nq, m_max]   row of each list entry; an entry whose row is outside [0, n_rows) is never read and behaves
 *                                   as a zero vector
 *   rel_dev     fp64 [nq, m_max]    the relevance the host computed for each entry (the chunk's 'score'), in list order
 *   counts_dev  int32 [nq]          entries per list (clamped to [0, m_max])
 *   lam         1 - diversity_penalty, in [0, 1]
 *   order_dev   int32 [nq, m_max]   out: the first counts[i] slots are the list's positions in MMR order, the others -1
 * Position 0 is taken first.  Every candidate's `closest` starts at 0 and becomes max(closest, cos(candidate, newest pick)) after
 * each pick; cos = dot / (|a| |b|) in fp32 (fp32 products, fp32 accumulation; 0 when a norm is 0, never NaN);
 * value = lam * rel - (1 - lam) * closest in fp64; the largest value wins, equal values go to the lowest position -- the
 * reference's strict `>` over the pending candidates in ascending order.  No host synchronisation, no workspace. */
int crs_mmr_order(const float* vecs_dev, int64_t n_rows, int dim, const int64_t* rows_dev, const double* rel_dev,
                  const int32_t* counts_dev, int nq, int m_max, double lam, int32_t* order_dev, void* stream);

/* ---- lexical re-rank: replaces the scoring, threshold and _rerank loops of ContextRetriever.retrieve_batch -- rag/retrieval.py ----
 * (additive to ABI 3; csrc/rerank.hip).  Processes `nq` result lists of at most m_max <= CRS_MAX_K candidates in one launch, one
 * wave per list, with the host's fp64 arithmetic (every operation rounded on its own), so the outputs carry the host's bits:
 *   scores_dev       fp32 [nq, m_max]   the store's cosine scores, list order
 *   rows_dev         int64 [nq, m_max]  sidecar row of each candidate; a negative row is an empty slot; a row >= n_rows is never
 *                                       dereferenced and has no hits
 *   doc_offsets_dev  int64 [n_rows + 1] CSR over doc_tokens_dev: row r holds the ascending distinct token ids of its document
 *   doc_tokens_dev   int32 [n_doc_tokens]  (may be null when n_doc_tokens is 0); offsets are clamped into [0, n_doc_tokens]
 *   q_offsets_dev    int64 [nq + 1]     CSR over q_tokens_dev: the ascending distinct KNOWN token ids of each query
 *   q_tokens_dev     int32 [n_q_tokens] (may be null when n_q_tokens is 0); offsets are clamped into [0, n_q_tokens]
 *   q_norm_dev       int32 [nq]         max(distinct tokens of the query, 1), tokens no document holds included
 *   k, threshold     list length wanted (>= 1) and similarity_threshold
 * Per list: dist = (double)(1.0f - score); d = min(max(dist, 0), 2); sim = min(max(1 - d * d / 2, 0), 1) (NaN stays NaN); a
 * candidate is kept iff sim >= threshold.  More than k kept: rr = sim * 0.7 + (hits / q_norm) * 0.3 with hits = the number of query
 * ids among the row's ids, ordered by rr descending, equal rr by list position ascending, cut to k, reranked = 1.  Otherwise the
 * first min(kept, k) kept positions in list order, reranked = 0.
 *   order_dev        int32 [nq, m_max]  out: input positions, -1 past the count
 *   count_dev        int32 [nq]         out: entries of order
 *   sim_dev          fp64 [nq, m_max]   out, by input position (0 for an empty slot)
 *   rr_dev           fp64 [nq, m_max]   out, by input position: the re-rank score of the kept candidates of a reranked list, else 0
 *   reranked_dev     int32 [nq]         out
 * No host synchronisation, no workspace. */
int crs_rerank_lexical(const float* scores_dev, const int64_t* rows_dev, int nq, int m_max, const int64_t* doc_offsets_dev,
                       const int32_t* doc_tokens_dev, int64_t n_rows, int64_t n_doc_tokens, const int64_t* q_offsets_dev,
                       const int32_t* q_tokens_dev, int64_t n_q_tokens, const int32_t* q_norm_dev, int k, double threshold,
                       int32_t* order_dev, int32_t* count_dev, double* sim_dev, double* rr_dev, int32_t* reranked_dev, void* stream);

/* ---- hybrid retrieval, lexical half: exact BM25 top-k over the token CSR -- no reference call site (the reference retrieves by
 * cosine alone) (additive to ABI 3; csrc/bm25.hip).  A flat doc-at-a-time scan: every row of the CSR is streamed once for the
 * whole query batch, each query's top-k is selected in the kernel and the per-workgroup lists are joined as crs_merge_topk does.
 *   doc_offsets_dev  int64 [n_rows + 1]    CSR over doc_tokens_dev / doc_tf_dev; offsets are clamped into [0, n_doc_tokens]
 *   doc_tokens_dev   int32 [n_doc_tokens]  per row the ascending distinct token ids of its document (may be null when empty)
 *   doc_tf_dev       int32 [n_doc_tokens]  parallel: occurrences of that token in that row
 *   doc_len_dev      int32 [n_rows]        tokens of the row's document, repeats counted
 *   q_offsets_dev    int64 [nq + 1]        CSR over q_tokens_dev / q_weights_dev; offsets are clamped into [0, n_q_tokens]
 *   q_tokens_dev     int32 [n_q_tokens]    per query its ascending distinct KNOWN token ids (may be null when empty)
 *   q_weights_dev    fp32 [n_q_tokens]     parallel: w_t = ln(1 + (N - df_t + 0.5) / (df_t + 0.5)), computed in fp64, rounded once
 *   c0, c1, k1p1     k1 (1 - b), k1 b / avgdl and k1 + 1, computed in fp64, rounded once
 * score(q, d) over the tokens t both hold, in ascending token id, all fp32, every operation rounded on its own (no fused
 * multiply-add, correctly rounded division):
 *     dn = c0 + c1 * (float)len_d;   term_t = (w_t * ((float)tf * k1p1)) / ((float)tf + dn);   score = ((0 + term_1) + term_2) + ...
 * so the scores are a pure function of the inputs (tests/_bm25_ref.py restates them bit for bit in numpy).  A row that shares no
 * token with the query is not a hit, whatever its score would be, and never enters a list.
 *   out_scores_dev fp32 [nq, k] descending, out_rows_dev int64 [nq, k]; ties -> lower row first; empty slots (-inf, -1).
 * Limits (CRS_EINVAL otherwise): 1 <= nq <= 64; 1 <= k <= CRS_MAX_K; 0 <= n_q_tokens <= CRS_BM25_MAX_PAIRS (the (query, token)
 * pairs of one launch: cut a longer batch into several launches); 0 <= n_rows < 2^31 - 64.  A malformed CSR gives wrong scores,
 * never an access outside the buffers.  Workspace: crs_bm25_workspace_bytes() bytes, 256-byte aligned, contents don't-care.
 * No host synchronisation. */
#define CRS_BM25_MAX_PAIRS 4096
int crs_bm25_workspace_bytes(int nq, int k, int64_t n_rows, size_t* bytes);
int crs_bm25_topk(const int64_t* doc_offsets_dev, const int32_t* doc_tokens_dev, const int32_t* doc_tf_dev, const int32_t* doc_len_dev,
                  int64_t n_rows, int64_t n_doc_tokens, const int64_t* q_offsets_dev, const int32_t* q_tokens_dev,
                  const float* q_weights_dev, int nq, int64_t n_q_tokens, float c0, float c1, float k1p1, int k, void* workspace_dev,
                  size_t workspace_bytes, float* out_scores_dev, int64_t* out_rows_dev, void* stream);

/* ---- hybrid retrieval, fusion: weighted reciprocal rank fusion of a dense and a lexical list per query (additive to ABI 3;
 * csrc/fuse.hip).  One wave per query, `nq` queries per launch.
 *   dense_rows_dev   int64 [nq, m_dense]   rows in rank order, a negative row = empty slot; valid rows distinct within a list
 *   lex_rows_dev     int64 [nq, m_lex]     likewise; 1 <= m_dense, m_lex <= CRS_MAX_K
 * A row at 0-based position i of the dense list and j of the lexical list scores, in fp64 with every operation rounded on its own,
 *     fused = w_dense / ((c + i) + 1) + w_lex / ((c + j) + 1)      (dense term first; a row in one list only: that term alone)
 * Order: fused descending, ties by the smaller dense position (absent = infinite), then the smaller lexical position.
 *   rows_dev int64, fused_dev fp64, dense_pos_dev int32, lex_pos_dev int32 (-1 = absent), each [nq, k_out], 1 <= k_out <= 2 CRS_MAX_K;
 *   past the count: (-1, 0.0, -1, -1).  count_dev int32 [nq] = min(distinct rows, k_out).
 * c >= 0 and the weights finite and >= 0.  Rows are compared, never dereferenced.  No host synchronisation, no workspace. */
int crs_fuse_rrf(const int64_t* dense_rows_dev, int m_dense, const int64_t* lex_rows_dev, int m_lex, int nq, double c, double w_dense,
                 double w_lex, int k_out, int64_t* rows_dev, double* fused_dev, int32_t* dense_pos_dev, int32_t* lex_pos_dev,
                 int32_t* count_dev, void* stream);

/* ---- tokenisation: BERT basic tokenisation + WordPiece of a batch of UTF-8 texts -- the tokenizer inside SentenceTransformer.encode,
 * rag/embedding.py:65 (additive to ABI 3; csrc/wordpiece.hip).  One workgroup per text; the tables are built by rag/_wordpiece.py.
 *   text_dev       uint8 [n_bytes]          the texts' UTF-8 bytes, one after the other
 *   offsets_dev    int64 [n_texts + 1]      text i is bytes [offsets[i], offsets[i + 1]); clamped into [0, n_bytes]
 *   table_dev      uint32 [table_len]       one entry per code point: bits 0-2 class (0 drop, 1 white space, 2 a word of its own,
 *                                           3 keep, 4 fallback) | bits 3-4 n, the replacement's length (0-3) | bits 5-7 "is
 *                                           punctuation" of each replacement code point | bits 8-31 the replacement (n = 1) or
 *                                           its offset in rep_pool_dev (n >= 2).  A code point >= table_len counts as fallback
 *   rep_pool_dev   uint32 [rep_pool_len]    the replacements of two and three code points
 *   slots_dev      int32 [n_slots, 4]       the vocabulary, open addressing with linear probing, n_slots a power of two, 16-byte
 *                                           aligned: {offset in vocab_pool_dev, length | continuation << 31, id, hash}; length 0 =
 *                                           empty.  hash = FNV-1a (32 bit) over the code points from 2166136261 (a word's first
 *                                           piece) or 2166136261 ^ 0x9E3779B9 (a '##' piece); home slot (hash ^ hash >> 15) & (n_slots - 1)
 *   vocab_pool_dev uint32 [vocab_pool_len]  the pieces' code points, without the '##'
 *   max_probe      slots a lookup looks at before it gives up (the longest probe sequence of the built table); 1..n_slots
 *   lmax           code points of the longest piece; 1..100
 *   mode           0 WordPiece (a word of more than 100 code points, or with a position no piece matches, is unk_id);
 *                  1 one id per word, hash_lo + crc32(the word's UTF-8) % hash_span (zlib's CRC-32); the vocabulary is not read
 *   ids_dev   int32 [n_texts, max_len]  out: cls_id, the first max_len - 2 ids, sep_id, then pad_id
 *   lens_dev  int32 [n_texts]           out: ids before the padding (2..max_len)
 *   flags_dev int32 [n_texts]           out: 1 = the text holds a fallback code point in the part that was read; its row is to be
 *                                       ignored and the text tokenised on the host
 * A text is read only until max_len - 2 ids exist.  Malformed UTF-8 or tables give wrong ids, never an access outside the buffers.
 * Limits (CRS_EINVAL otherwise): n_texts >= 0 (0: no launch); 2 <= max_len <= 65536; hash_span >= 1 in mode 1.
 * Deterministic; no workspace, no host synchronisation. */
#define CRS_WORDPIECE_TILE_BYTES 1024   /* bytes of a text staged at a time (tests aim at the boundaries) */
int crs_wordpiece_encode(const uint8_t* text_dev, const int64_t* offsets_dev, int n_texts, int64_t n_bytes, const uint32_t* table_dev,
                         int64_t table_len, const uint32_t* rep_pool_dev, int64_t rep_pool_len, const int32_t* slots_dev, int64_t n_slots,
                         const uint32_t* vocab_pool_dev, int64_t vocab_pool_len, int max_probe, int lmax, int mode, int unk_id, int cls_id,
                         int sep_id, int pad_id, int hash_lo, int hash_span, int max_len, int32_t* ids_dev, int32_t* lens_dev,
                         int32_t* flags_dev, void* stream);

/* ---- tokenisation: SentencePiece Unigram of a batch of UTF-8 texts, as the `tokenizers` library runs XLM-RoBERTa's tokenizer.json
 * (normaliser, Replace(" {2,}"), WhitespaceSplit + Metaspace, Unigram, <s> $A </s>) -- the tokenizer inside SentenceTransformer.encode,
 * /root/reference/rag/embedding.py:65-71, when the model is a multilingual one (additive to ABI 3; csrc/unigram.hip).  One workgroup
 * per text; the tables are built by rag/_unigram.py.  text_dev, offsets_dev, ids_dev, lens_dev, flags_dev: as crs_wordpiece_encode.
 *   table_dev        uint32 [table_len]     one entry per code point: bits 0-2 class (0 drop, 3 keep, 4 fallback) | bits 3-4 n, the
 *                                           replacement's length (0-3) | bits 5-10 the kind of each replacement code point, two bits
 *                                           each (0 character, 1 U+0020, 2 other white space, 3 U+2581) | bits 11-31 the replacement
 *                                           (n = 1) or its offset in rep_pool_dev (n >= 2).  A code point >= table_len is fallback
 *   slots_dev        int32 [n_slots, 4]     the pieces, laid out as crs_wordpiece_encode's slots; no continuation bit, every hash
 *                                           starts from 2166136261
 *   slot_scores_dev  fp64 [n_slots]         the score of the piece in each slot (tokenizer.json's, unrounded)
 *   lmax             code points of the longest piece; 1..CRS_UNIGRAM_MAX_WORD
 *   unk_score        the score of an unknown character: the smallest piece score - 10
 *   opts             CRS_UNIGRAM_* bits
 * Per word (U+2581 + its characters): best[end] is replaced only by a strictly greater fp64 sum best[start] + score, starts
 * ascending; a start with no one-character piece gets a one-character candidate of unk_id at unk_score; unk_ids next to each other
 * in a word fuse into one.  flags_dev: 1 = a fallback code point, or a word of more than CRS_UNIGRAM_MAX_WORD code points (U+2581
 * included), in the part that was read: tokenise the text on the host.  Malformed UTF-8 or tables give wrong ids, never an access
 * outside the buffers.  Limits (CRS_EINVAL otherwise): n_texts >= 0; 2 <= max_len <= 65536; slot_scores_dev 8-byte aligned.
 * Deterministic; no workspace, no host synchronisation. */
#define CRS_UNIGRAM_TILE_BYTES 1024    /* bytes of a text staged at a time */
#define CRS_UNIGRAM_MAX_WORD 128       /* code points of the longest word the kernel walks, its U+2581 included */
#define CRS_UNIGRAM_COLLAPSE 1         /* a run of two or more U+0020 counts as one thing (a Replace(" {2,}") step exists) */
#define CRS_UNIGRAM_SINGLE_META 2      /* a lone U+0020 is a metaspace (no WhitespaceSplit); else it ends a word */
#define CRS_UNIGRAM_RUN_META 4         /* such a run is a metaspace; else it ends a word */
#define CRS_UNIGRAM_CRLF 8             /* CR in front of LF adds nothing: the normaliser turns the two into what LF alone gives */
int crs_unigram_encode(const uint8_t* text_dev, const int64_t* offsets_dev, int n_texts, int64_t n_bytes, const uint32_t* table_dev,
                       int64_t table_len, const uint32_t* rep_pool_dev, int64_t rep_pool_len, const int32_t* slots_dev,
                       const double* slot_scores_dev, int64_t n_slots, const uint32_t* vocab_pool_dev, int64_t vocab_pool_len,
                       int max_probe, int lmax, double unk_score, int opts, int unk_id, int cls_id, int sep_id, int pad_id, int max_len,
                       int32_t* ids_dev, int32_t* lens_dev, int32_t* flags_dev, void* stream);

/* ---- BERTScore token matching: the step behind the encoder in bert_score.score -- evaluation/retrieval/rag_metrics.py:179-207 ----
 * (additive to ABI 3; csrc/token_match.hip).  Scores `n_pairs` (candidate, reference) pairs of token states in one launch, one
 * workgroup per pair:
 *   a_dev      fp32 [n_pairs, seq_a, hidden]  candidate token states, 16-byte aligned; rows at or past len_a are never read
 *   len_a_dev  int32 [n_pairs]                real tokens of each candidate (clamped to [0, seq_a])
 *   b_dev      fp32 [n_pairs, seq_b, hidden]  reference token states, 16-byte aligned; rows at or past len_b are never read
 *   len_b_dev  int32 [n_pairs]                real tokens of each reference (clamped to [0, seq_b])
 *   w_a_dev    fp32 [n_pairs, seq_a] or null  token weights of the candidates (idf); null = 1 on every real token
 *   w_b_dev    fp32 [n_pairs, seq_b] or null  token weights of the references
 *   out_dev    fp32 [n_pairs, 3]              out: P, R, F
 * sim[i][j] = <a_i, b_j> / (|a_i| |b_j|) over i < len_a, j < len_b, fp32 products and fp32 accumulation (f32-input MFMA: an fmaf
 * chain over hidden), 0 when either norm is 0, never NaN from a zero row.  P = sum_i w_a[i] max_j sim[i][j] / sum_i w_a[i],
 * R = sum_j w_b[j] max_i sim[i][j] / sum_j w_b[j]; a side whose weight sum is not positive, and both sides of a pair with an empty
 * sentence, give 0.  F = 2PR / (P + R), 0 when P + R is 0 or not finite.  A pair's three numbers do not depend on n_pairs, on the
 * other pairs of the launch, on seq_a / seq_b or on anything stored in the padding rows.
 * Limits (CRS_EINVAL otherwise): 1 <= seq_a, seq_b <= 512; hidden a multiple of 64 in 64..1024; n_pairs >= 0 (0: no launch).
 * No host synchronisation, no workspace. */
int crs_token_match(const float* a_dev, const int32_t* len_a_dev, int seq_a, const float* b_dev, const int32_t* len_b_dev, int seq_b,
                    int n_pairs, int hidden, const float* w_a_dev, const float* w_b_dev, float* out_dev, void* stream);

/* ---- near-duplicate detection: thresholded self-join of the slab (additive to ABI 3; csrc/join.hip) -- no reference
 * call site: the reference's chunker produces the duplicates (chunk_overlap, repeated boiler-plate), nothing in it removes them ----
 * crs_pairs_above_f16 (stage 1) finds every pair (i, j) with i in [a_first, a_first + a_rows), j in [b_first, b_first + b_rows),
 * i < j and slab score <fp16 row i, fp16 row j> >= thr (fp32 accumulation over all crs_padded_dim(dim) elements, the padding being
 * the zeros the slab holds):
 *   slab_dev        fp16 [n_rows, crs_padded_dim(dim)], 16-byte aligned (CRS_SLAB_F16 only); both ranges lie inside [0, n_rows)
 *   pairs_out_dev   int64 [cap, 2], 16-byte aligned: (i, j) of each pair, once;  scores_out_dev fp32 [cap]: its slab score
 *   count_dev       ONE int64 the caller zeroed: the number of qualifying pairs is ADDED to it whether or not they fitted --
 *                   count > cap is the overflow signal, nothing is written at or past cap, and which pairs fitted is unspecified
 * Pair order is unspecified.  A = B = all rows is the whole self-join, A = all rows and B = the new tail the incremental one;
 * stripes of either bound the buffers and the grid: one launch takes at most CRS_PAIRS_MAX_TILES tile pairs,
 * ceil(a_rows / CRS_PAIRS_TILE) * (ceil(b_rows / CRS_PAIRS_TILE) rounded up to a multiple of 8) (CRS_EINVAL above that).  One
 * 512-thread workgroup per 256 x 256 tile pair (v_mfma_f32_16x16x32_f16; tile pairs without an i < j leave at once); a workgroup
 * with hits issues ONE returned atomic.  An empty range: no launch.  thr must be finite.
 *
 * crs_pairs_verify_f32 (stage 2) scores `m` candidate pairs (pairs_dev int64 [m, 2], 16-byte aligned) against the fp32 shadow
 * [n_rows, dim]: sim32 = one fmaf chain per lane of a quarter wave (lane l: coordinates l, l + 16, ...) and an xor butterfly -- a
 * fixed order, bitwise independent of m and of the other pairs.  Pairs with sim32 >= thr are compacted into rows_a_dev / rows_b_dev
 * (int64) / sims_dev (fp32), each [>= m], in unspecified order; their number is ADDED to count_dev (ONE int64 the caller zeroed).
 * A pair with a row outside [0, n_rows) is dropped, never dereferenced.  m = 0: no launch.
 *
 * With thr1 = t - eps for stage 1 and t for stage 2, eps = (2 E + E^2)(1 + 1e-4) + (1.5 pdim + 8) 2^-23 and E the slab's tracked
 * row error (row_err_max above), the result is exactly {i < j : sim32(i, j) >= t} (DESIGN 3.13 has the derivation).
 * No workspace, no host synchronisation. */
#define CRS_PAIRS_TILE 256               /* rows per tile edge of the join (tests aim at the boundaries) */
#define CRS_PAIRS_MAX_TILES (1 << 22)    /* tile pairs of one crs_pairs_above_f16 launch */
int crs_pairs_above_f16(const void* slab_dev, int64_t n_rows, int dim, int64_t a_first, int64_t a_rows, int64_t b_first, int64_t b_rows,
                        float thr, int64_t* pairs_out_dev, float* scores_out_dev, int64_t cap, int64_t* count_dev, void* stream);
int crs_pairs_verify_f32(const int64_t* pairs_dev, int64_t m, const float* shadow_f32_dev, int64_t n_rows, int dim, float thr,
                         int64_t* rows_a_dev, int64_t* rows_b_dev, float* sims_dev, int64_t* count_dev, void* stream);

/* ---- late interaction (ColBERT): per-token projection and MaxSim scoring of candidate lists -- no reference call site: the
 * reference re-ranks by token overlap alone (rag/retrieval.py:_rerank) (additive to ABI 3; csrc/token_project.hip, csrc/maxsim.hip,
 * DESIGN 3.15) ----
 * crs_token_project turns final hidden states into packed unit-length fp16 token vectors, dimp = dim rounded up to a multiple of 32:
 *   hidden_dev  fp32 [n_tok, hidden]   16-byte aligned; a row whose dst is negative is NEVER read (a padding position)
 *   w16_dev     fp16 [dim, hidden]     row-major (out, in), 16-byte aligned
 *   bias_dev    fp32 [dim] or null
 *   dst_dev     int64 [n_tok]          output slot of each token, < 0 = drop; the caller keeps the slots inside out16_dev
 *   out16_dev   fp16 [*, dimp]         out: row dst = y, zeros in [dim, dimp)
 * v = W h (+ b) with h rounded to fp16 on load and fp32 accumulation (v_mfma_f32_16x16x32_f16), y = v / |v| with the norm and the
 * scaling in fp32, rounded to fp16 once; y is all zeros when |v| is 0.  A token's output does not depend on what else is in the launch.
 * Limits (CRS_EINVAL otherwise, before any launch): 1 <= dim <= 128; hidden a multiple of 32 in 32..1024; 0 <= n_tok <= 2^36
 * (0: no launch).  No workspace, no host synchronisation.
 *
 * crs_maxsim scores nq lists of m_max candidate rows in one launch, one wave per (query, candidate):
 *   q16_dev      fp16 [nq, lq_max, dimp]  query token vectors, 16-byte aligned; rows at or past q_len are never read
 *   q_len_dev    int32 [nq]               query tokens (clamped to [0, lq_max])
 *   tok16_dev    fp16 [n_tokens, dimp]    the index's token vectors, 16-byte aligned (may be null when n_tokens is 0)
 *   offsets_dev  int64 [n_rows + 1]       CSR over tok16_dev: row r holds tokens [offsets[r], offsets[r + 1]); clamped into
 *                                         [0, n_tokens]
 *   rows_dev     int64 [nq, m_max]        candidate rows
 *   out_dev      fp32 [nq, m_max]         out[q][c] = sum_{i < q_len[q]} max_{j in doc} <q_i, d_j>, fp32 accumulation; the row
 *                                         maxima are added in a fixed order
 * A row < 0 or >= n_rows is never dereferenced and scores -inf; otherwise a document with no tokens, and q_len == 0, score 0.
 * A pair's score is bitwise independent of nq, m_max, lq_max and of what else shares the launch.
 * Limits (CRS_EINVAL otherwise, before any launch): 1 <= lq_max <= CRS_MAXSIM_MAX_QUERY; dimp in {32, 64, 96, 128}; 0 <= nq <= 65535
 * (0: no launch); m_max >= 1.  No workspace, no atomics, no host synchronisation. */
#define CRS_MAXSIM_MAX_QUERY 64          /* query tokens of crs_maxsim: four row blocks of 16 held in registers */
int crs_token_project(const float* hidden_dev, const void* w16_dev, const float* bias_dev, const int64_t* dst_dev, void* out16_dev,
                      int64_t n_tok, int hidden, int dim, void* stream);
int crs_maxsim(const void* q16_dev, const int32_t* q_len_dev, int nq, int lq_max, const void* tok16_dev, const int64_t* offsets_dev,
               int64_t n_rows, int64_t n_tokens, const int64_t* rows_dev, int m_max, int dimp, float* out_dev, void* stream);

/* ---- learned sparse retrieval (SPLADE): compaction of a dense weight row, impact top-k over a weighted token CSR -- no reference
 * call site (additive to ABI 3; csrc/sparse_compact.hip, csrc/sparse_scan.hip; the head that produces the dense rows
 * is crs_mlm_sparse_pool, crs_encoder.h) ----
 * crs_sparse_compact turns each row of weights_dev fp32 [batch, vp] (columns [0, vocab) count) into a bounded sparse row:
 *   the ids whose weight is > 0 (a NaN or -0 is not) and that are not in skip_ids_dev int32 [n_skip] (may be null when n_skip is 0);
 *   when more than `cap` remain, the cap largest weights, ties at the threshold by lower id; emitted in ascending id order as
 *   ids_dev int32 [batch, cap] / out_weights_dev fp32 [batch, cap], unused slots (-1, 0); counts_dev int32 [batch] = ids kept.
 * Exact and deterministic (no floating-point arithmetic: a positive float orders as its bit pattern).  One workgroup per text.
 * Limits (CRS_EINVAL otherwise, before any launch): batch >= 1; 1 <= vocab <= vp; 1 <= cap <= CRS_SPARSE_MAX_TERMS;
 * 0 <= n_skip <= CRS_SPARSE_MAX_SKIP.  No workspace, no host synchronisation.
 *
 * crs_sparse_topk is crs_bm25_topk with a weight per (row, token) in place of the term frequency and the row length:
 *   doc_weights_dev  fp32 [n_doc_tokens]  parallel to doc_tokens_dev
 * score(q, d) over the tokens t both hold, in ascending token id, all fp32, every operation rounded on its own (no fused
 * multiply-add):   score = ((0 + q_w1 * d_w1) + q_w2 * d_w2) + ...      (tests/_sparse_ref.py restates it bit for bit in numpy)
 * Everything else -- the other arguments, the limits (1 <= nq <= 64, 1 <= k <= CRS_MAX_K, 0 <= n_q_tokens <= CRS_BM25_MAX_PAIRS,
 * 0 <= n_rows < 2^31 - 64), "a row sharing no token is no hit", ties by lower row, empty slots (-inf, -1), offsets clamped before
 * they become addresses, the workspace rule (crs_sparse_workspace_bytes) and the merge -- is crs_bm25_topk's. */
#define CRS_SPARSE_MAX_TERMS 1024
#define CRS_SPARSE_MAX_SKIP 16
int crs_sparse_compact(const float* weights_dev, int batch, int vocab, int vp, int cap, const int32_t* skip_ids_dev, int n_skip,
                       int32_t* ids_dev, float* out_weights_dev, int32_t* counts_dev, void* stream);
int crs_sparse_workspace_bytes(int nq, int k, int64_t n_rows, size_t* bytes);
int crs_sparse_topk(const int64_t* doc_offsets_dev, const int32_t* doc_tokens_dev, const float* doc_weights_dev, int64_t n_rows,
                    int64_t n_doc_tokens, const int64_t* q_offsets_dev, const int32_t* q_tokens_dev, const float* q_weights_dev, int nq,
                    int64_t n_q_tokens, int k, void* workspace_dev, size_t workspace_bytes, float* out_scores_dev,
                    int64_t* out_rows_dev, void* stream);

/* ---- one-collective exchange (ONE all-gather per query batch) ------------------
 * A rank's per-shard result travels as one contiguous "wire block":
 *     [ ids int64 [nq, k] | scores fp32 [nq, k] | pad to 8 bytes ]        crs_wire_bytes(nq, k) bytes
 * crs_cosine_topk / crs_refine_f32 write it in place (out_ids = block, out_scores = block +
 * crs_wire_scores_offset(nq, k)); an all-gather of the blocks gives [nlists][crs_wire_bytes] and
 * crs_merge_topk_wire ranks it like crs_merge_topk. */
size_t crs_wire_bytes(int nq, int k);
size_t crs_wire_scores_offset(int nq, int k);
int crs_merge_topk_wire(const void* wire_dev, int nlists, int nq, int k_in, int k_out,
                        float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* crs_merge_sorted over the wire layout (same precondition and limits; wire_dev 8-byte aligned): the exchange of a sharded
 * search with top_k above CRS_MAX_K. */
int crs_merge_sorted_wire(const void* wire_dev, int nlists, int nq, int k_in, int k_out,
                          float* out_scores_dev, int64_t* out_ids_dev, void* stream);

/* Which scan kernel (and launch geometry) crs_cosine_topk would use for these sizes on the current
 * device, as text, e.g. "scan_tb_kernel<384,32,4,0> streams=768 qblocks=1 kp=5 + merge + refine".
 * For bench.py / profiles only; writes at most `cap` bytes including the terminator. */
int crs_scan_plan_describe(int nq, int dim, int k, int64_t n_rows, int slab_type, char* buf, size_t cap);

/* A HIP stream whose kernels run on CUs [first_cu, first_cu + n_cus) only (hipExtStreamCreateWithCUMask; on this part consecutive
 * mask bits go round the XCDs).  The throughput engine (rag/_engine.py) gives its query-encoder lanes such streams: the latency-bound
 * 38-launch encoder chain then shares a few CUs with the corpus sweep instead of touching all of them, and the sweep's dynamic tile
 * schedule routes around those CUs.  No reference counterpart (the reference runs one query at a time on one stream).
 * Destroy with crs_stream_destroy. */
int crs_stream_create_cu_masked(int first_cu, int n_cus, void** stream_out);
int crs_stream_destroy(void* stream);

/* Timing hook for bench.py: runs `iters` back-to-back crs_cosine_topk launches bracketed by
 * hipEvents on `stream` and returns the mean milliseconds of ONE launch pair (scan + merge)
 * in *ms_total and of the scan kernel alone in *ms_scan. */
int crs_time_cosine_topk(const void* q16_dev, int nq, int dim, int slab_type, const void* slab_dev,
                         const float* scales_dev, int64_t n_rows, int k, void* workspace_dev,
                         size_t workspace_bytes, float* out_scores_dev, int64_t* out_ids_dev,
                         void* stream, int iters, float* ms_total, float* ms_scan);

#ifdef __cplusplus
}
#endif
#endif /* CRS_HIP_H */
