// torch_ops.cpp -- PyTorch-ROCm custom ops over the C ABI of libcrs_hip.so (host-only C++, no device code).
//
// north_star / SURVEY section 8(b): "Python host code invokes hand-written HIP kernels via PyTorch-ROCm custom
// ops".  TORCH_LIBRARY(crs, ...) registers, for the HIP ("CUDA" dispatch key on torch-ROCm) backend:
//   crs::encoder_forward   replaces SentenceTransformer.encode's forward      (reference rag/embedding.py:65-71)
//   crs::slab_append       replaces collection.add(embeddings=...)            (reference rag/indexing.py:114-119)
//   crs::slab_write_rows / crs::slab_compact   in-place update and delete of rows (csrc/row_build.hip, csrc/mutate.hip; the
//                          reference's ChromaDB collection offers update / delete, its own code never calls them)
//   crs::queries_to_f16    query side of the same conversion                  (reference rag/indexing.py:156-168)
//   crs::rows_norm_max / slab_append_space / slab_write_rows_space / slab_rescale_space / queries_to_space / space_distances
//                          hnsw:space 'ip' and 'l2' on the same scan (csrc/row_build.hip, csrc/space.hip; ChromaDB's spaces, reference rag/indexing.py:83)
//   crs::cosine_topk       replaces collection.query(query_embeddings, n)     (reference rag/indexing.py:171-176)
//   crs::refine_f32        over-fetch re-rank against the fp32 shadow         
//   crs::refine_f32_cert / crs::escalate_exact   the same with a per-query exactness proof, and the in-stream
//                          escalation of unproven queries (identical ids to an fp32 store: rag/indexing.py:171-176)
//   crs::cosine_topk_cert  the scan and the certificate in one call (one fused tail kernel where the plan allows)
//   crs::cosine_topk_large_cert / crs::refine_large_cert   the same for 64 < k_out <= 1024: partitioned over-fetch, one
//                          fp32 re-rank + certificate kernel over every chunk's candidates
//   crs::merge_topk / crs::merge_topk_wire   cross-shard merge                (new vs the reference)
//   crs::merge_sorted / crs::merge_sorted_wire   the same for sorted lists, k 65 .. 1024
//   crs::mmr_order         replaces the greedy MMR loop of _apply_diversity  (reference rag/retrieval.py:219-277)
//   crs::token_match       the greedy matching behind bert_score.score  (reference evaluation/retrieval/rag_metrics.py:179-207)
//   crs::unigram_encode             SentencePiece Unigram tokenisation of UTF-8 texts on the device (XLM-RoBERTa's tokenizer.json)
//   crs::wordpiece_encode          BERT basic tokenisation + WordPiece of UTF-8 texts on the device (the tokenizer inside SentenceTransformer.encode)
//   crs::bm25_topk / crs::fuse_rrf   hybrid retrieval: exact BM25 scan over the token CSR, reciprocal rank fusion (new vs the reference)
//   crs::pairs_above / crs::pairs_verify   near-duplicate detection: thresholded self-join of the slab, fp32 check (new vs the reference)
//   crs::mlm_sparse_pool / crs::sparse_compact / crs::sparse_topk   learned sparse retrieval (SPLADE): MLM head with max-pool epilogue, compaction, impact scan (new vs the reference)
//   crs::token_project / crs::maxsim   late interaction (ColBERT): per-token projection and MaxSim scoring of candidate lists (new vs the reference)
//   crs::rerank_lexical    replaces the scoring, threshold and _rerank loops of retrieve_batch  (reference rag/retrieval.py:75-77, 196-217)
// Tensors are torch-owned; every op launches on the CURRENT HIP stream of the tensors' device, so the ops
// compose with torch streams and hipGraph capture.  Errors of the C ABI surface as RuntimeError (TORCH_CHECK)
// carrying crs_last_error(); the Python wrappers (rag/_native.py) translate where the reference's types differ.
// The C ABI (include/crs_hip.h, include/crs_encoder.h) stays the drop-in boundary for non-torch hosts
// (INTEGRATION.md section 2); this file only adapts it.
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>   // torch-ROCm tensors carry DeviceType "cuda": the masquerading guard/stream
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/library.h>

#include <tuple>
#include <vector>

#include "../../include/crs_encoder.h"
#include "../../include/crs_hip.h"

namespace {

using at::Tensor;

void* cur_stream(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

void ok(int rc, const char* what) { TORCH_CHECK(rc == 0, what, ": libcrs_hip error ", rc, ": ", crs_last_error()); }

void want(const Tensor& t, at::ScalarType ty, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a device (HIP) tensor");
  TORCH_CHECK(t.scalar_type() == ty, name, " has dtype ", t.scalar_type(), ", expected ", ty);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
const void* opt_ptr(const c10::optional<Tensor>& t) { return (t.has_value() && t->defined()) ? t->data_ptr() : nullptr; }
bool has(const c10::optional<Tensor>& t) { return t.has_value() && t->defined(); }

// every tensor of a call must live on the device whose stream and guard the op uses: with a one-process multi-device
// store a mismatched tensor would otherwise be a GPU memory fault (or a silent wrong-device read), not an exception
void same_device(const Tensor& ref, std::initializer_list<const Tensor*> ts, const char* op) {
  for (const Tensor* t : ts)
    if (t && t->defined()) TORCH_CHECK(t->device() == ref.device(), op, ": all tensors must be on ", ref.device(), ", got one on ", t->device());
}
const Tensor* opt_t(const c10::optional<Tensor>& t) { return has(t) ? &*t : nullptr; }

int slab_type_of(const Tensor& slab) {
  TORCH_CHECK(slab.scalar_type() == at::kHalf || slab.scalar_type() == at::kChar, "slab must be fp16 or int8");
  return slab.scalar_type() == at::kChar ? CRS_SLAB_I8 : CRS_SLAB_F16;
}

// ---- index build and row updates (csrc/row_build.hip) --------------------------------------------------------------
// the checks every row writer shares: row_err, and slab / scales / shadow shaped for `rows` rows of the space's stored dimension
int row_writer_checks(int64_t dim, int64_t space, const Tensor& slab, const c10::optional<Tensor>& scales, const c10::optional<Tensor>& shadow,
                      const c10::optional<Tensor>& row_err, int64_t rows) {
  if (has(row_err)) { want(*row_err, at::kFloat, "row_err"); TORCH_CHECK(row_err->numel() >= 1, "row_err must hold one fp32"); }
  TORCH_CHECK(slab.dim() == 2 && slab.is_cuda() && slab.is_contiguous(), "slab [cap, pdim]");
  const int st = slab_type_of(slab);
  TORCH_CHECK(dim > 0 && dim <= 1024, "bad dim");
  const int sdim = crs_space_row_dim((int)dim, (int)space);
  TORCH_CHECK(sdim > 0 && sdim <= 1024, "dim out of range for this space");
  TORCH_CHECK(slab.size(1) == crs_row_elems(sdim, st), "slab row length must be crs_row_elems(crs_space_row_dim(dim, space), slab_type)");
  TORCH_CHECK(rows >= 0 && rows <= slab.size(0), "rows exceed the slab");
  if (st == CRS_SLAB_I8) {
    TORCH_CHECK(has(scales), "int8 slab needs scales");
    want(*scales, at::kFloat, "scales");
    TORCH_CHECK(scales->numel() >= rows, "scales too short");
  }
  if (has(shadow)) {
    want(*shadow, at::kFloat, "shadow");
    TORCH_CHECK(shadow->dim() == 2 && shadow->size(1) == sdim && shadow->size(0) >= rows, "shadow must be fp32 [>= rows, crs_space_row_dim]");
  }
  return st;
}

void slab_append(const Tensor& emb, Tensor slab, c10::optional<Tensor> scales, c10::optional<Tensor> shadow, int64_t row0,
                 c10::optional<Tensor> row_err) {
  want(emb, at::kFloat, "emb");
  same_device(emb, {&slab, opt_t(scales), opt_t(shadow), opt_t(row_err)}, "crs::slab_append");
  TORCH_CHECK(emb.dim() == 2 && row0 >= 0, "emb [n, dim], row0 >= 0");
  const int64_t n = emb.size(0);
  const int dim = (int)emb.size(1);
  const int st = row_writer_checks(dim, CRS_SPACE_COSINE, slab, scales, shadow, row_err, row0 + n);
  c10::hip::HIPGuardMasqueradingAsCUDA g(emb.device());
  ok(crs_slab_append_f32(emb.data_ptr<float>(), n, dim, st, slab.data_ptr(), (float*)opt_ptr(scales), (float*)opt_ptr(shadow), row0,
                         (float*)opt_ptr(row_err), cur_stream(emb)), "crs::slab_append");
}

void slab_write_rows(const Tensor& emb, const Tensor& rows, Tensor slab, c10::optional<Tensor> scales, c10::optional<Tensor> shadow,
                     int64_t n_rows, c10::optional<Tensor> row_err) {
  want(emb, at::kFloat, "emb");
  want(rows, at::kLong, "rows");
  same_device(emb, {&rows, &slab, opt_t(scales), opt_t(shadow), opt_t(row_err)}, "crs::slab_write_rows");
  TORCH_CHECK(emb.dim() == 2 && rows.dim() == 1 && rows.size(0) == emb.size(0), "emb [m, dim], rows int64 [m]");
  const int dim = (int)emb.size(1);
  const int st = row_writer_checks(dim, CRS_SPACE_COSINE, slab, scales, shadow, row_err, n_rows);
  c10::hip::HIPGuardMasqueradingAsCUDA g(emb.device());
  ok(crs_slab_write_rows_f32(emb.data_ptr<float>(), rows.data_ptr<int64_t>(), emb.size(0), dim, st, slab.data_ptr(), (float*)opt_ptr(scales),
                             (float*)opt_ptr(shadow), n_rows, (float*)opt_ptr(row_err), cur_stream(emb)), "crs::slab_write_rows");
}

// ---- in-place mutation (csrc/mutate.hip) ------------------------------------------------------------------------
void slab_compact(const Tensor& dead, int64_t n_rows, Tensor slab, c10::optional<Tensor> scales, c10::optional<Tensor> shadow,
                  c10::optional<Tensor> rows_global, Tensor bounce, int64_t first_row) {
  want(dead, at::kLong, "dead");
  want(bounce, at::kByte, "bounce");
  same_device(dead, {&slab, opt_t(scales), opt_t(shadow), opt_t(rows_global), &bounce}, "crs::slab_compact");
  TORCH_CHECK(dead.dim() == 1 && slab.dim() == 2 && slab.is_cuda() && slab.is_contiguous(), "dead [m], slab [cap, pdim]");
  const int st = slab_type_of(slab);
  TORCH_CHECK(n_rows >= 0 && n_rows <= slab.size(0) && dead.size(0) <= n_rows, "n_rows exceeds the slab, or more dead rows than rows");
  int dim = (int)slab.size(1);        // without a shadow only the padded row length matters
  if (has(shadow)) {
    want(*shadow, at::kFloat, "shadow");
    TORCH_CHECK(shadow->dim() == 2 && shadow->size(0) >= n_rows, "shadow must be fp32 [>= n_rows, dim]");
    dim = (int)shadow->size(1);
  }
  TORCH_CHECK(slab.size(1) == crs_row_elems(dim, st), "slab row length must be crs_row_elems(dim, slab_type)");
  if (has(scales)) { want(*scales, at::kFloat, "scales"); TORCH_CHECK(scales->numel() >= n_rows, "scales too short"); }
  if (has(rows_global)) { want(*rows_global, at::kLong, "rows_global"); TORCH_CHECK(rows_global->numel() >= n_rows, "rows_global too short"); }
  c10::hip::HIPGuardMasqueradingAsCUDA g(dead.device());
  ok(crs_slab_compact(dead.data_ptr<int64_t>(), dead.size(0), n_rows, first_row, dim, st, slab.data_ptr(), (float*)opt_ptr(scales),
                      (float*)opt_ptr(shadow), (int64_t*)opt_ptr(rows_global), bounce.data_ptr(), (size_t)bounce.nbytes(), cur_stream(dead)),
     "crs::slab_compact");
}

void queries_to_f16(const Tensor& q32, Tensor out16, int64_t slab_type) {
  want(q32, at::kFloat, "q32");
  want(out16, at::kHalf, "out16");
  same_device(q32, {&out16}, "crs::queries_to_f16");
  TORCH_CHECK(q32.dim() == 2 && out16.dim() == 2 && out16.size(0) == q32.size(0) &&
                  out16.size(1) == crs_row_elems((int)q32.size(1), (int)slab_type), "out16 must be [nq, crs_row_elems(dim, slab_type)]");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_queries_to_f16(q32.data_ptr<float>(), (int)q32.size(0), (int)q32.size(1), (int)slab_type, out16.data_ptr(), cur_stream(q32)),
     "crs::queries_to_f16");
}

// ---- inner-product / squared-L2 spaces (csrc/row_build.hip, csrc/space.hip; include/crs_hip.h holds the contracts) --------------
void want_scale(const Tensor& norm_scale) {
  want(norm_scale, at::kFloat, "norm_scale");
  TORCH_CHECK(norm_scale.numel() >= 1, "norm_scale must hold one fp32");
}
void want_space(int64_t space) { TORCH_CHECK(space == CRS_SPACE_IP || space == CRS_SPACE_L2, "space must be CRS_SPACE_IP or CRS_SPACE_L2"); }

void rows_norm_max(const Tensor& emb, Tensor norm_max) {
  want(emb, at::kFloat, "emb");
  want(norm_max, at::kFloat, "norm_max");
  same_device(emb, {&norm_max}, "crs::rows_norm_max");
  TORCH_CHECK(emb.dim() == 2 && norm_max.numel() >= 1, "emb [n, dim], norm_max one fp32");
  c10::hip::HIPGuardMasqueradingAsCUDA g(emb.device());
  ok(crs_rows_norm_max(emb.data_ptr<float>(), emb.size(0), (int)emb.size(1), norm_max.data_ptr<float>(), nullptr, cur_stream(emb)),
     "crs::rows_norm_max");
}

void slab_append_space(const Tensor& emb, int64_t space, const Tensor& norm_scale, Tensor slab, c10::optional<Tensor> scales,
                       c10::optional<Tensor> shadow, int64_t row0, c10::optional<Tensor> row_err) {
  want(emb, at::kFloat, "emb");
  want_scale(norm_scale);
  same_device(emb, {&norm_scale, &slab, opt_t(scales), opt_t(shadow), opt_t(row_err)}, "crs::slab_append_space");
  want_space(space);
  TORCH_CHECK(emb.dim() == 2 && row0 >= 0, "emb [n, dim], row0 >= 0");
  const int dim = (int)emb.size(1);
  const int st = row_writer_checks(dim, space, slab, scales, shadow, row_err, row0 + emb.size(0));
  c10::hip::HIPGuardMasqueradingAsCUDA g(emb.device());
  ok(crs_slab_append_space_f32(emb.data_ptr<float>(), emb.size(0), dim, (int)space, st, norm_scale.data_ptr<float>(), slab.data_ptr(),
                               (float*)opt_ptr(scales), (float*)opt_ptr(shadow), row0, (float*)opt_ptr(row_err), cur_stream(emb)),
     "crs::slab_append_space");
}

void slab_write_rows_space(const Tensor& emb, const Tensor& rows, int64_t space, const Tensor& norm_scale, Tensor slab,
                           c10::optional<Tensor> scales, c10::optional<Tensor> shadow, int64_t n_rows, c10::optional<Tensor> row_err) {
  want(emb, at::kFloat, "emb");
  want(rows, at::kLong, "rows");
  want_scale(norm_scale);
  same_device(emb, {&rows, &norm_scale, &slab, opt_t(scales), opt_t(shadow), opt_t(row_err)}, "crs::slab_write_rows_space");
  want_space(space);
  TORCH_CHECK(emb.dim() == 2 && rows.dim() == 1 && rows.size(0) == emb.size(0), "emb [m, dim], rows int64 [m]");
  const int dim = (int)emb.size(1);
  const int st = row_writer_checks(dim, space, slab, scales, shadow, row_err, n_rows);
  c10::hip::HIPGuardMasqueradingAsCUDA g(emb.device());
  ok(crs_slab_write_rows_space_f32(emb.data_ptr<float>(), rows.data_ptr<int64_t>(), emb.size(0), dim, (int)space, st,
                                   norm_scale.data_ptr<float>(), slab.data_ptr(), (float*)opt_ptr(scales), (float*)opt_ptr(shadow), n_rows,
                                   (float*)opt_ptr(row_err), cur_stream(emb)), "crs::slab_write_rows_space");
}

void slab_rescale_space(int64_t n_rows, int64_t dim, int64_t space, int64_t shift, Tensor slab, c10::optional<Tensor> scales, Tensor shadow,
                        c10::optional<Tensor> row_err) {
  same_device(slab, {opt_t(scales), &shadow, opt_t(row_err)}, "crs::slab_rescale_space");
  want_space(space);
  const int st = row_writer_checks(dim, space, slab, scales, c10::optional<Tensor>(shadow), row_err, n_rows);
  c10::hip::HIPGuardMasqueradingAsCUDA g(slab.device());
  ok(crs_slab_rescale_space(n_rows, (int)dim, (int)space, st, (int)shift, slab.data_ptr(), (float*)opt_ptr(scales), shadow.data_ptr<float>(),
                            (float*)opt_ptr(row_err), cur_stream(slab)), "crs::slab_rescale_space");
}

void queries_to_space(const Tensor& q, int64_t space, int64_t slab_type, const Tensor& norm_scale, Tensor out32, Tensor out16) {
  want(q, at::kFloat, "q");
  want(out32, at::kFloat, "out32");
  want(out16, at::kHalf, "out16");
  want_scale(norm_scale);
  want_space(space);
  same_device(q, {&norm_scale, &out32, &out16}, "crs::queries_to_space");
  TORCH_CHECK(q.dim() == 2 && out32.dim() == 2 && out16.dim() == 2, "q [nq, dim], out32 [nq, d'], out16 [nq, pdim]");
  const int sdim = crs_space_row_dim((int)q.size(1), (int)space);
  TORCH_CHECK(sdim > 0 && sdim <= 1024, "dim out of range for this space");
  TORCH_CHECK(out32.size(0) == q.size(0) && out32.size(1) == sdim && out16.size(0) == q.size(0) &&
                  out16.size(1) == crs_row_elems(sdim, (int)slab_type), "out32 must be [nq, d'], out16 [nq, crs_row_elems(d', slab_type)]");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
  ok(crs_queries_to_space(q.data_ptr<float>(), (int)q.size(0), (int)q.size(1), (int)space, (int)slab_type, norm_scale.data_ptr<float>(),
                          out32.data_ptr<float>(), out16.data_ptr(), cur_stream(q)), "crs::queries_to_space");
}

void space_distances(const Tensor& q, int64_t space, const Tensor& shadow, int64_t n_rows, int64_t id_base, const Tensor& norm_scale,
                     const Tensor& ids, Tensor out_dist, Tensor out_ids) {
  want(q, at::kFloat, "q");
  want(shadow, at::kFloat, "shadow");
  want(ids, at::kLong, "ids");
  want(out_dist, at::kFloat, "out_dist");
  want(out_ids, at::kLong, "out_ids");
  want_scale(norm_scale);
  want_space(space);
  same_device(q, {&shadow, &norm_scale, &ids, &out_dist, &out_ids}, "crs::space_distances");
  TORCH_CHECK(q.dim() == 2 && shadow.dim() == 2 && ids.dim() == 2 && ids.size(0) == q.size(0), "q [nq, dim], shadow [rows, d'], ids [nq, k]");
  TORCH_CHECK(shadow.size(1) == crs_space_row_dim((int)q.size(1), (int)space) && n_rows >= 0 && n_rows <= shadow.size(0),
              "shadow must be fp32 [>= n_rows, crs_space_row_dim(dim, space)]");
  TORCH_CHECK(out_dist.sizes() == ids.sizes() && out_ids.sizes() == ids.sizes(), "out_dist / out_ids must be [nq, k]");
  if (ids.numel() == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(q.device());
  ok(crs_space_distances(q.data_ptr<float>(), (int)q.size(0), (int)q.size(1), (int)space, shadow.data_ptr<float>(), n_rows, id_base,
                         norm_scale.data_ptr<float>(), ids.data_ptr<int64_t>(), (int)ids.size(1), out_dist.data_ptr<float>(),
                         out_ids.data_ptr<int64_t>(), cur_stream(q)), "crs::space_distances");
}

// ---- search --------------------------------------------------------------------------------------------------
void cosine_topk_out(const Tensor& q16, const Tensor& slab, c10::optional<Tensor> scales, int64_t n_rows, int64_t dim, int64_t k,
                     int64_t id_base, Tensor workspace, Tensor out_scores, Tensor out_ids) {
  want(q16, at::kHalf, "q16");
  TORCH_CHECK(slab.is_cuda() && slab.is_contiguous() && slab.dim() == 2 && q16.dim() == 2, "q16 [nq, pdim], slab [rows, pdim]");
  const int st = slab_type_of(slab);
  const int pdim = crs_row_elems((int)dim, st);
  TORCH_CHECK(q16.size(1) == pdim && slab.size(1) == pdim, "q16 / slab row length must be crs_row_elems(dim, slab_type) = ", pdim);
  TORCH_CHECK(n_rows >= 1 && n_rows <= slab.size(0), "n_rows out of range");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  const int64_t nq = q16.size(0);
  TORCH_CHECK(out_scores.numel() == nq * k && out_ids.numel() == nq * k, "outputs must hold [nq, k]");
  TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous(), "workspace must be a contiguous device tensor");
  if (st == CRS_SLAB_I8) {
    TORCH_CHECK(has(scales), "int8 slab needs scales");
    want(*scales, at::kFloat, "scales");
    TORCH_CHECK(scales->numel() >= n_rows, "scales shorter than n_rows");
  }
  same_device(q16, {&slab, opt_t(scales), &workspace, &out_scores, &out_ids}, "crs::cosine_topk");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q16.device());
  ok(crs_cosine_topk(q16.data_ptr(), (int)nq, (int)dim, st, slab.data_ptr(), (const float*)opt_ptr(scales), n_rows, (int)k, id_base,
                     workspace.data_ptr(), (size_t)workspace.nbytes(), out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(),
                     cur_stream(q16)), "crs::cosine_topk");
}

std::tuple<Tensor, Tensor> cosine_topk(const Tensor& q16, const Tensor& slab, c10::optional<Tensor> scales, int64_t n_rows, int64_t dim,
                                       int64_t k, int64_t id_base) {
  TORCH_CHECK(q16.dim() == 2, "q16 must be [nq, pdim]");
  size_t need = 0;
  ok(crs_scan_workspace_bytes((int)q16.size(0), (int)dim, (int)k, n_rows, &need), "crs::cosine_topk (workspace)");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q16.device());
  Tensor ws = at::empty({(int64_t)need}, q16.options().dtype(at::kByte));
  Tensor s = at::empty({q16.size(0), k}, q16.options().dtype(at::kFloat));
  Tensor i = at::empty({q16.size(0), k}, q16.options().dtype(at::kLong));
  cosine_topk_out(q16, slab, scales, n_rows, dim, k, id_base, ws, s, i);
  return {s, i};
}

void refine_f32_out(const Tensor& q32, const Tensor& shadow, int64_t n_rows, int64_t id_base, const Tensor& cand_ids, int64_t k_out,
                    Tensor out_scores, Tensor out_ids) {
  want(q32, at::kFloat, "q32");
  want(shadow, at::kFloat, "shadow");
  want(cand_ids, at::kLong, "cand_ids");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  TORCH_CHECK(q32.dim() == 2 && shadow.dim() == 2 && cand_ids.dim() == 2 && shadow.size(1) == q32.size(1) &&
                  cand_ids.size(0) == q32.size(0) && n_rows <= shadow.size(0), "q32 [nq, dim], shadow [>= n_rows, dim], cand_ids [nq, k_in]");
  TORCH_CHECK(out_scores.numel() == q32.size(0) * k_out && out_ids.numel() == q32.size(0) * k_out, "outputs must hold [nq, k_out]");
  TORCH_CHECK(cand_ids.size(1) >= k_out, "cand_ids holds fewer than k_out candidates per query");
  same_device(q32, {&shadow, &cand_ids, &out_scores, &out_ids}, "crs::refine_f32");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_refine_f32(q32.data_ptr<float>(), (int)q32.size(0), (int)q32.size(1), shadow.data_ptr<float>(), n_rows, id_base,
                    cand_ids.data_ptr<int64_t>(), (int)cand_ids.size(1), (int)k_out, out_scores.data_ptr<float>(),
                    out_ids.data_ptr<int64_t>(), cur_stream(q32)), "crs::refine_f32");
}

void score_rows_f32_out(const Tensor& q32, const Tensor& shadow, int64_t n_rows, int64_t id_base, const Tensor& ids, Tensor scores) {
  want(q32, at::kFloat, "q32");
  want(shadow, at::kFloat, "shadow");
  want(ids, at::kLong, "ids");
  want(scores, at::kFloat, "scores");
  TORCH_CHECK(q32.dim() == 2 && shadow.dim() == 2 && ids.dim() == 2 && shadow.size(1) == q32.size(1) && ids.size(0) == q32.size(0) &&
                  scores.sizes() == ids.sizes() && n_rows <= shadow.size(0), "q32 [nq, dim], shadow [>= n_rows, dim], ids / scores [nq, k]");
  same_device(q32, {&shadow, &ids, &scores}, "crs::score_rows_f32");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_score_rows_f32(q32.data_ptr<float>(), (int)q32.size(0), (int)q32.size(1), shadow.data_ptr<float>(), n_rows, id_base, (int)ids.size(1),
                        ids.data_ptr<int64_t>(), scores.data_ptr<float>(), cur_stream(q32)), "crs::score_rows_f32");
}

// ---- exactness certificate + escalation (include/crs_hip.h, csrc/exact.hip) --------------------------------------------------
void refine_f32_cert_out(const Tensor& q32, const Tensor& q16, const Tensor& shadow, int64_t n_rows, int64_t id_base,
                         const Tensor& cand_ids, const Tensor& cand_scores, int64_t k_out, double row_err_max, int64_t slab_type,
                         Tensor out_scores, Tensor out_ids, Tensor status, Tensor exact_ws, int64_t cap) {
  want(q32, at::kFloat, "q32");
  want(q16, at::kHalf, "q16");
  want(shadow, at::kFloat, "shadow");
  want(cand_ids, at::kLong, "cand_ids");
  want(cand_scores, at::kFloat, "cand_scores");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  want(status, at::kInt, "status");
  TORCH_CHECK(exact_ws.is_cuda() && exact_ws.is_contiguous(), "exact_ws must be a contiguous device tensor");
  const int64_t nq = q32.size(0);
  TORCH_CHECK(q32.dim() == 2 && q16.dim() == 2 && shadow.dim() == 2 && cand_ids.dim() == 2 && shadow.size(1) == q32.size(1) &&
                  cand_ids.size(0) == nq && cand_scores.sizes() == cand_ids.sizes() && n_rows <= shadow.size(0) && q16.size(0) == nq &&
                  q16.size(1) == crs_row_elems((int)q32.size(1), (int)slab_type),
              "q32 [nq, dim], q16 [nq, crs_row_elems], shadow [>= n_rows, dim], cand_ids / cand_scores [nq, k_in]");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out && status.numel() == nq, "outputs must hold [nq, k_out], status [nq]");
  same_device(q32, {&q16, &shadow, &cand_ids, &cand_scores, &out_scores, &out_ids, &status, &exact_ws}, "crs::refine_f32_cert");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_refine_f32_cert(q32.data_ptr<float>(), q16.data_ptr(), (int)nq, (int)q32.size(1), (int)slab_type, shadow.data_ptr<float>(), n_rows,
                         id_base, cand_ids.data_ptr<int64_t>(), cand_scores.data_ptr<float>(), (int)cand_ids.size(1), (int)k_out,
                         (float)row_err_max, out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(), status.data_ptr<int32_t>(),
                         exact_ws.data_ptr(), (size_t)exact_ws.nbytes(), (int)cap, cur_stream(q32)), "crs::refine_f32_cert");
}

void cosine_topk_cert_out(const Tensor& q32, const Tensor& q16, const Tensor& slab, c10::optional<Tensor> scales, const Tensor& shadow,
                          int64_t n_rows, int64_t id_base, int64_t k_out, double row_err_max, Tensor workspace, Tensor cand_scores,
                          Tensor cand_ids, Tensor out_scores, Tensor out_ids, Tensor status, Tensor exact_ws, int64_t cap) {
  want(q32, at::kFloat, "q32");
  want(q16, at::kHalf, "q16");
  want(shadow, at::kFloat, "shadow");
  want(cand_scores, at::kFloat, "cand_scores");
  want(cand_ids, at::kLong, "cand_ids");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  want(status, at::kInt, "status");
  TORCH_CHECK(slab.is_cuda() && slab.is_contiguous() && slab.dim() == 2, "slab [rows, pdim]");
  TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous(), "workspace must be a contiguous device tensor");
  TORCH_CHECK(exact_ws.is_cuda() && exact_ws.is_contiguous(), "exact_ws must be a contiguous device tensor");
  const int st = slab_type_of(slab);
  const int64_t nq = q32.size(0);
  const int dim = (int)q32.size(1);
  const int pdim = crs_row_elems(dim, st);
  TORCH_CHECK(q32.dim() == 2 && q16.dim() == 2 && q16.size(0) == nq && q16.size(1) == pdim && slab.size(1) == pdim && shadow.dim() == 2 &&
                  shadow.size(1) == dim && n_rows >= 1 && n_rows <= slab.size(0) && n_rows <= shadow.size(0) && cand_ids.dim() == 2 &&
                  cand_ids.size(0) == nq && cand_scores.sizes() == cand_ids.sizes(),
              "q32 [nq, dim], q16 [nq, pdim], slab [>= n_rows, pdim], shadow [>= n_rows, dim], cand_scores / cand_ids [nq, k_in]");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out && status.numel() == nq, "outputs must hold [nq, k_out], status [nq]");
  if (st == CRS_SLAB_I8) {
    TORCH_CHECK(has(scales), "int8 slab needs scales");
    want(*scales, at::kFloat, "scales");
    TORCH_CHECK(scales->numel() >= n_rows, "scales shorter than n_rows");
  }
  same_device(q32, {&q16, &slab, opt_t(scales), &shadow, &workspace, &cand_scores, &cand_ids, &out_scores, &out_ids, &status, &exact_ws},
              "crs::cosine_topk_cert");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_cosine_topk_cert(q16.data_ptr(), (int)nq, dim, st, slab.data_ptr(), (const float*)opt_ptr(scales), n_rows, (int)cand_ids.size(1),
                          id_base, workspace.data_ptr(), (size_t)workspace.nbytes(), cand_scores.data_ptr<float>(), cand_ids.data_ptr<int64_t>(),
                          q32.data_ptr<float>(), shadow.data_ptr<float>(), (int)k_out, (float)row_err_max, out_scores.data_ptr<float>(),
                          out_ids.data_ptr<int64_t>(), status.data_ptr<int32_t>(), exact_ws.data_ptr(), (size_t)exact_ws.nbytes(), (int)cap,
                          cur_stream(q32)), "crs::cosine_topk_cert");
}

// ---- certified top-k above CRS_MAX_K (include/crs_hip.h, csrc/large_k.hip) ------------------------------------------------------
void cosine_topk_large_cert_out(const Tensor& q32, const Tensor& q16, const Tensor& slab, c10::optional<Tensor> scales, const Tensor& shadow,
                                int64_t n_rows, int64_t id_base, int64_t k_out, double row_err_max, Tensor workspace, Tensor out_scores,
                                Tensor out_ids, Tensor status, Tensor exact_ws, int64_t cap) {
  want(q32, at::kFloat, "q32");
  want(q16, at::kHalf, "q16");
  want(shadow, at::kFloat, "shadow");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  want(status, at::kInt, "status");
  TORCH_CHECK(slab.is_cuda() && slab.is_contiguous() && slab.dim() == 2, "slab [rows, pdim]");
  TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous(), "workspace must be a contiguous device tensor");
  TORCH_CHECK(exact_ws.is_cuda() && exact_ws.is_contiguous(), "exact_ws must be a contiguous device tensor");
  const int st = slab_type_of(slab);
  const int64_t nq = q32.size(0);
  const int dim = (int)q32.size(1);
  const int pdim = crs_row_elems(dim, st);
  TORCH_CHECK(q32.dim() == 2 && q16.dim() == 2 && q16.size(0) == nq && q16.size(1) == pdim && slab.size(1) == pdim && shadow.dim() == 2 &&
                  shadow.size(1) == dim && n_rows >= 1 && n_rows <= slab.size(0) && n_rows <= shadow.size(0),
              "q32 [nq, dim], q16 [nq, pdim], slab [>= n_rows, pdim], shadow [>= n_rows, dim]");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out && status.numel() == nq, "outputs must hold [nq, k_out], status [nq]");
  if (st == CRS_SLAB_I8) {
    TORCH_CHECK(has(scales), "int8 slab needs scales");
    want(*scales, at::kFloat, "scales");
    TORCH_CHECK(scales->numel() >= n_rows, "scales shorter than n_rows");
  }
  same_device(q32, {&q16, &slab, opt_t(scales), &shadow, &workspace, &out_scores, &out_ids, &status, &exact_ws}, "crs::cosine_topk_large_cert");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_cosine_topk_large_cert(q16.data_ptr(), (int)nq, dim, st, slab.data_ptr(), (const float*)opt_ptr(scales), n_rows, id_base,
                                workspace.data_ptr(), (size_t)workspace.nbytes(), q32.data_ptr<float>(), shadow.data_ptr<float>(), (int)k_out,
                                (float)row_err_max, out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(), status.data_ptr<int32_t>(),
                                exact_ws.data_ptr(), (size_t)exact_ws.nbytes(), (int)cap, cur_stream(q32)),
     "crs::cosine_topk_large_cert");
}

void refine_large_cert_out(const Tensor& q32, const Tensor& q16, const Tensor& shadow, int64_t n_rows, int64_t id_base, const Tensor& cand_ids,
                           const Tensor& cand_scores, int64_t chunk_rows, int64_t k_out, double row_err_max, int64_t slab_type,
                           Tensor out_scores, Tensor out_ids, Tensor status, Tensor exact_ws, int64_t cap) {
  want(q32, at::kFloat, "q32");
  want(q16, at::kHalf, "q16");
  want(shadow, at::kFloat, "shadow");
  want(cand_ids, at::kLong, "cand_ids");
  want(cand_scores, at::kFloat, "cand_scores");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  want(status, at::kInt, "status");
  TORCH_CHECK(exact_ws.is_cuda() && exact_ws.is_contiguous(), "exact_ws must be a contiguous device tensor");
  const int64_t nq = q32.size(0);
  TORCH_CHECK(q32.dim() == 2 && q16.dim() == 2 && shadow.dim() == 2 && cand_ids.dim() == 3 && shadow.size(1) == q32.size(1) &&
                  cand_ids.size(1) == nq && cand_ids.size(2) == CRS_MAX_K && cand_scores.sizes() == cand_ids.sizes() &&
                  n_rows <= shadow.size(0) && q16.size(0) == nq && q16.size(1) == crs_row_elems((int)q32.size(1), (int)slab_type),
              "q32 [nq, dim], q16 [nq, crs_row_elems], shadow [>= n_rows, dim], cand_ids / cand_scores [parts, nq, 64]");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out && status.numel() == nq, "outputs must hold [nq, k_out], status [nq]");
  same_device(q32, {&q16, &shadow, &cand_ids, &cand_scores, &out_scores, &out_ids, &status, &exact_ws}, "crs::refine_large_cert");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_refine_large_cert(q32.data_ptr<float>(), q16.data_ptr(), (int)nq, (int)q32.size(1), (int)slab_type, shadow.data_ptr<float>(), n_rows,
                           id_base, cand_ids.data_ptr<int64_t>(), cand_scores.data_ptr<float>(), (int)cand_ids.size(0), chunk_rows, (int)k_out,
                           (float)row_err_max, out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(), status.data_ptr<int32_t>(),
                           exact_ws.data_ptr(), (size_t)exact_ws.nbytes(), (int)cap, cur_stream(q32)),
     "crs::refine_large_cert");
}

void escalate_exact(const Tensor& q32, const Tensor& q16, const Tensor& slab, c10::optional<Tensor> scales, const Tensor& shadow,
                    int64_t n_rows, int64_t id_base, int64_t k_out, Tensor out_scores, Tensor out_ids, Tensor status, Tensor exact_ws,
                    int64_t cap) {
  want(q32, at::kFloat, "q32");
  want(q16, at::kHalf, "q16");
  want(shadow, at::kFloat, "shadow");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  want(status, at::kInt, "status");
  TORCH_CHECK(slab.is_cuda() && slab.is_contiguous() && slab.dim() == 2, "slab [rows, pdim]");
  TORCH_CHECK(exact_ws.is_cuda() && exact_ws.is_contiguous(), "exact_ws must be a contiguous device tensor");
  const int st = slab_type_of(slab);
  const int64_t nq = q32.size(0);
  const int pdim = crs_row_elems((int)q32.size(1), st);
  TORCH_CHECK(q32.dim() == 2 && q16.dim() == 2 && q16.size(0) == nq && q16.size(1) == pdim && slab.size(1) == pdim && shadow.dim() == 2 &&
                  shadow.size(1) == q32.size(1) && n_rows >= 1 && n_rows <= slab.size(0) && n_rows <= shadow.size(0),
              "q32 [nq, dim], q16 [nq, pdim], slab [>= n_rows, pdim], shadow [>= n_rows, dim]");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out && status.numel() == nq, "outputs must hold [nq, k_out], status [nq]");
  if (st == CRS_SLAB_I8) {
    TORCH_CHECK(has(scales), "int8 slab needs scales");
    want(*scales, at::kFloat, "scales");
    TORCH_CHECK(scales->numel() >= n_rows, "scales shorter than n_rows");
  }
  same_device(q32, {&q16, &slab, opt_t(scales), &shadow, &out_scores, &out_ids, &status, &exact_ws}, "crs::escalate_exact");
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  ok(crs_escalate_exact(q32.data_ptr<float>(), q16.data_ptr(), (int)nq, (int)q32.size(1), st, slab.data_ptr(), (const float*)opt_ptr(scales),
                        shadow.data_ptr<float>(), n_rows, id_base, (int)k_out, out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(),
                        status.data_ptr<int32_t>(), exact_ws.data_ptr(), (size_t)exact_ws.nbytes(), (int)cap, cur_stream(q32)),
     "crs::escalate_exact");
}

std::tuple<Tensor, Tensor> refine_f32(const Tensor& q32, const Tensor& shadow, int64_t n_rows, int64_t id_base, const Tensor& cand_ids,
                                      int64_t k_out) {
  c10::hip::HIPGuardMasqueradingAsCUDA g(q32.device());
  Tensor s = at::empty({q32.size(0), k_out}, q32.options().dtype(at::kFloat));
  Tensor i = at::empty({q32.size(0), k_out}, q32.options().dtype(at::kLong));
  refine_f32_out(q32, shadow, n_rows, id_base, cand_ids, k_out, s, i);
  return {s, i};
}

void merge_topk_out(const Tensor& scores, const Tensor& ids, int64_t k_out, Tensor out_scores, Tensor out_ids) {
  want(scores, at::kFloat, "scores");
  want(ids, at::kLong, "ids");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  TORCH_CHECK(scores.dim() == 3 && ids.sizes() == scores.sizes(), "scores / ids must be [nlists, nq, k_in]");
  TORCH_CHECK(out_scores.numel() == scores.size(1) * k_out && out_ids.numel() == scores.size(1) * k_out, "outputs must hold [nq, k_out]");
  same_device(scores, {&ids, &out_scores, &out_ids}, "crs::merge_topk");
  c10::hip::HIPGuardMasqueradingAsCUDA g(scores.device());
  ok(crs_merge_topk(scores.data_ptr<float>(), ids.data_ptr<int64_t>(), (int)scores.size(0), (int)scores.size(1), (int)scores.size(2),
                    (int)k_out, out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(), cur_stream(scores)), "crs::merge_topk");
}

std::tuple<Tensor, Tensor> merge_topk(const Tensor& scores, const Tensor& ids, int64_t k_out) {
  TORCH_CHECK(scores.dim() == 3, "scores must be [nlists, nq, k_in]");
  c10::hip::HIPGuardMasqueradingAsCUDA g(scores.device());
  Tensor s = at::empty({scores.size(1), k_out}, scores.options().dtype(at::kFloat));
  Tensor i = at::empty({scores.size(1), k_out}, scores.options().dtype(at::kLong));
  merge_topk_out(scores, ids, k_out, s, i);
  return {s, i};
}

void merge_topk_wire_out(const Tensor& wire, int64_t nlists, int64_t nq, int64_t k_in, int64_t k_out, Tensor out_scores, Tensor out_ids) {
  TORCH_CHECK(wire.is_cuda() && wire.is_contiguous() && wire.scalar_type() == at::kByte, "wire must be a contiguous uint8 device tensor");
  TORCH_CHECK((size_t)wire.numel() >= (size_t)nlists * crs_wire_bytes((int)nq, (int)k_in), "wire buffer shorter than nlists * crs_wire_bytes(nq, k_in)");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out, "outputs must hold [nq, k_out]");
  same_device(wire, {&out_scores, &out_ids}, "crs::merge_topk_wire");
  c10::hip::HIPGuardMasqueradingAsCUDA g(wire.device());
  ok(crs_merge_topk_wire(wire.data_ptr(), (int)nlists, (int)nq, (int)k_in, (int)k_out, out_scores.data_ptr<float>(),
                         out_ids.data_ptr<int64_t>(), cur_stream(wire)), "crs::merge_topk_wire");
}

// sorted lists, k up to CRS_MAX_K_CERT (csrc/merge_sorted.hip)
void merge_sorted_out(const Tensor& scores, const Tensor& ids, int64_t k_out, Tensor out_scores, Tensor out_ids) {
  want(scores, at::kFloat, "scores");
  want(ids, at::kLong, "ids");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  TORCH_CHECK(scores.dim() == 3 && ids.sizes() == scores.sizes(), "scores / ids must be [nlists, nq, k_in]");
  TORCH_CHECK(out_scores.numel() == scores.size(1) * k_out && out_ids.numel() == scores.size(1) * k_out, "outputs must hold [nq, k_out]");
  same_device(scores, {&ids, &out_scores, &out_ids}, "crs::merge_sorted");
  c10::hip::HIPGuardMasqueradingAsCUDA g(scores.device());
  ok(crs_merge_sorted(scores.data_ptr<float>(), ids.data_ptr<int64_t>(), (int)scores.size(0), (int)scores.size(1), (int)scores.size(2),
                      (int)k_out, out_scores.data_ptr<float>(), out_ids.data_ptr<int64_t>(), cur_stream(scores)), "crs::merge_sorted");
}

void merge_sorted_wire_out(const Tensor& wire, int64_t nlists, int64_t nq, int64_t k_in, int64_t k_out, Tensor out_scores, Tensor out_ids) {
  TORCH_CHECK(wire.is_cuda() && wire.is_contiguous() && wire.scalar_type() == at::kByte, "wire must be a contiguous uint8 device tensor");
  TORCH_CHECK(nlists >= 0 && (size_t)wire.numel() >= (size_t)nlists * crs_wire_bytes((int)nq, (int)k_in), "wire buffer shorter than nlists * crs_wire_bytes(nq, k_in)");
  want(out_scores, at::kFloat, "out_scores");
  want(out_ids, at::kLong, "out_ids");
  TORCH_CHECK(out_scores.numel() == nq * k_out && out_ids.numel() == nq * k_out, "outputs must hold [nq, k_out]");
  same_device(wire, {&out_scores, &out_ids}, "crs::merge_sorted_wire");
  c10::hip::HIPGuardMasqueradingAsCUDA g(wire.device());
  ok(crs_merge_sorted_wire(wire.data_ptr(), (int)nlists, (int)nq, (int)k_in, (int)k_out, out_scores.data_ptr<float>(),
                           out_ids.data_ptr<int64_t>(), cur_stream(wire)), "crs::merge_sorted_wire");
}

// ---- diversity re-ordering (csrc/mmr.hip) -------------------------------------------------------------------------
// vecs fp32 [>= n_rows, dim]; rows int64 / rel fp64 / order int32 [nq, m_max]; counts int32 [nq]
void mmr_order_out(const Tensor& vecs, int64_t n_rows, const Tensor& rows, const Tensor& rel, const Tensor& counts, double lam, Tensor order) {
  want(vecs, at::kFloat, "vecs");
  want(rows, at::kLong, "rows");
  want(rel, at::kDouble, "rel");
  want(counts, at::kInt, "counts");
  want(order, at::kInt, "order");
  same_device(vecs, {&rows, &rel, &counts, &order}, "crs::mmr_order");
  TORCH_CHECK(vecs.dim() == 2 && n_rows >= 0 && n_rows <= vecs.size(0), "vecs must be fp32 [>= n_rows, dim]");
  TORCH_CHECK(rows.dim() == 2 && rel.sizes() == rows.sizes() && order.sizes() == rows.sizes(), "rows / rel / order must be [nq, m_max]");
  TORCH_CHECK(counts.dim() == 1 && counts.size(0) == rows.size(0), "counts must be int32 [nq]");
  TORCH_CHECK(rows.size(0) <= 0x7fffffff, "too many lists");
  if (rows.size(0) == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(vecs.device());
  ok(crs_mmr_order(vecs.data_ptr<float>(), n_rows, (int)vecs.size(1), rows.data_ptr<int64_t>(), rel.data_ptr<double>(),
                   counts.data_ptr<int32_t>(), (int)rows.size(0), (int)rows.size(1), lam, order.data_ptr<int32_t>(), cur_stream(vecs)),
     "crs::mmr_order");
}

// ---- BERTScore token matching (csrc/token_match.hip) ---------------------------------------------------------------
// a fp32 [n, seq_a, hidden], b fp32 [n, seq_b, hidden]; len_a / len_b int32 [n]; w_a fp32 [n, seq_a] / w_b fp32 [n, seq_b] (optional);
// out fp32 [n, 3]
void token_match_out(const Tensor& a, const Tensor& len_a, const Tensor& b, const Tensor& len_b, c10::optional<Tensor> w_a,
                     c10::optional<Tensor> w_b, Tensor out) {
  want(a, at::kFloat, "a");
  want(len_a, at::kInt, "len_a");
  want(b, at::kFloat, "b");
  want(len_b, at::kInt, "len_b");
  want(out, at::kFloat, "out");
  if (has(w_a)) want(*w_a, at::kFloat, "w_a");
  if (has(w_b)) want(*w_b, at::kFloat, "w_b");
  same_device(a, {&len_a, &b, &len_b, opt_t(w_a), opt_t(w_b), &out}, "crs::token_match");
  TORCH_CHECK(a.dim() == 3 && b.dim() == 3 && a.size(0) == b.size(0) && a.size(2) == b.size(2),
              "a must be fp32 [n, seq_a, hidden] and b fp32 [n, seq_b, hidden]");
  const int64_t n = a.size(0);
  TORCH_CHECK(n <= 0x7fffffff, "too many pairs");
  TORCH_CHECK(len_a.dim() == 1 && len_a.size(0) == n && len_b.dim() == 1 && len_b.size(0) == n, "len_a / len_b must be int32 [n]");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == n && out.size(1) == 3, "out must be fp32 [n, 3]");
  if (has(w_a)) TORCH_CHECK(w_a->dim() == 2 && w_a->size(0) == n && w_a->size(1) == a.size(1), "w_a must be fp32 [n, seq_a]");
  if (has(w_b)) TORCH_CHECK(w_b->dim() == 2 && w_b->size(0) == n && w_b->size(1) == b.size(1), "w_b must be fp32 [n, seq_b]");
  TORCH_CHECK(a.size(1) <= 0x7fffffff && b.size(1) <= 0x7fffffff && a.size(2) <= 0x7fffffff, "sizes out of range");
  if (n == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(a.device());
  ok(crs_token_match(a.data_ptr<float>(), len_a.data_ptr<int32_t>(), (int)a.size(1), b.data_ptr<float>(), len_b.data_ptr<int32_t>(),
                     (int)b.size(1), (int)n, (int)a.size(2), (const float*)opt_ptr(w_a), (const float*)opt_ptr(w_b),
                     out.data_ptr<float>(), cur_stream(a)), "crs::token_match");
}

// ---- lexical re-rank (csrc/rerank.hip) ----------------------------------------------------------------------------
// scores fp32 / rows int64 / order int32 / sim, rr fp64 [nq, m_max]; doc_offsets int64 [>= n_rows + 1], doc_tokens int32 (the rows'
// token CSR); q_offsets int64 [nq + 1], q_tokens int32 (the queries' known tokens); q_norm / count / reranked int32 [nq]
void rerank_lexical(const Tensor& scores, const Tensor& rows, const Tensor& doc_offsets, const Tensor& doc_tokens, int64_t n_rows,
                    const Tensor& q_offsets, const Tensor& q_tokens, const Tensor& q_norm, int64_t k, double threshold, Tensor order,
                    Tensor count, Tensor sim, Tensor rr, Tensor reranked) {
  want(scores, at::kFloat, "scores");
  want(rows, at::kLong, "rows");
  want(doc_offsets, at::kLong, "doc_offsets");
  want(doc_tokens, at::kInt, "doc_tokens");
  want(q_offsets, at::kLong, "q_offsets");
  want(q_tokens, at::kInt, "q_tokens");
  want(q_norm, at::kInt, "q_norm");
  want(order, at::kInt, "order");
  want(count, at::kInt, "count");
  want(sim, at::kDouble, "sim");
  want(rr, at::kDouble, "rr");
  want(reranked, at::kInt, "reranked");
  same_device(scores, {&rows, &doc_offsets, &doc_tokens, &q_offsets, &q_tokens, &q_norm, &order, &count, &sim, &rr, &reranked},
              "crs::rerank_lexical");
  TORCH_CHECK(rows.dim() == 2 && scores.sizes() == rows.sizes() && order.sizes() == rows.sizes() && sim.sizes() == rows.sizes() &&
              rr.sizes() == rows.sizes(), "scores / rows / order / sim / rr must be [nq, m_max]");
  const int64_t nq = rows.size(0);
  TORCH_CHECK(nq <= 0x7fffffff, "too many lists");
  TORCH_CHECK(n_rows >= 0 && doc_offsets.dim() == 1 && doc_offsets.numel() >= n_rows + 1, "doc_offsets must be int64 [>= n_rows + 1]");
  TORCH_CHECK(q_offsets.dim() == 1 && q_offsets.numel() == nq + 1, "q_offsets must be int64 [nq + 1]");
  TORCH_CHECK(q_norm.numel() == nq && count.numel() == nq && reranked.numel() == nq, "q_norm / count / reranked must be int32 [nq]");
  TORCH_CHECK(k >= 1 && k <= 0x7fffffff, "k must be at least 1");
  if (nq == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(scores.device());
  ok(crs_rerank_lexical(scores.data_ptr<float>(), rows.data_ptr<int64_t>(), (int)nq, (int)rows.size(1), doc_offsets.data_ptr<int64_t>(),
                        doc_tokens.numel() ? doc_tokens.data_ptr<int32_t>() : nullptr, n_rows, doc_tokens.numel(),
                        q_offsets.data_ptr<int64_t>(), q_tokens.numel() ? q_tokens.data_ptr<int32_t>() : nullptr, q_tokens.numel(),
                        q_norm.data_ptr<int32_t>(), (int)k, threshold, order.data_ptr<int32_t>(), count.data_ptr<int32_t>(),
                        sim.data_ptr<double>(), rr.data_ptr<double>(), reranked.data_ptr<int32_t>(), cur_stream(scores)),
     "crs::rerank_lexical");
}

// ---- late interaction (csrc/token_project.hip, csrc/maxsim.hip) ------------------------------------------------------
// hidden fp32 [n_tok, H]; w16 fp16 [dim, H]; bias fp32 [dim] (optional); dst int64 [n_tok], < 0 = drop, else a row of out16 (the
// caller builds it on the host and keeps it below out16's rows); out16 fp16 [rows, dim rounded up to 32]
void token_project(const Tensor& hidden, const Tensor& w16, c10::optional<Tensor> bias, const Tensor& dst, Tensor out16) {
  want(hidden, at::kFloat, "hidden");
  want(w16, at::kHalf, "w16");
  want(dst, at::kLong, "dst");
  want(out16, at::kHalf, "out16");
  if (has(bias)) want(*bias, at::kFloat, "bias");
  same_device(hidden, {&w16, opt_t(bias), &dst, &out16}, "crs::token_project");
  TORCH_CHECK(hidden.dim() == 2 && w16.dim() == 2 && w16.size(1) == hidden.size(1), "hidden must be fp32 [n_tok, H] and w16 fp16 [dim, H]");
  const int64_t n_tok = hidden.size(0), H = hidden.size(1), dim = w16.size(0);
  TORCH_CHECK(dim >= 1 && dim <= 128 && H <= 1024, "dim must be in 1..128 and H at most 1024");
  TORCH_CHECK(dst.dim() == 1 && dst.size(0) == n_tok, "dst must be int64 [n_tok]");
  TORCH_CHECK(out16.dim() == 2 && out16.size(1) == (dim + 31) / 32 * 32, "out16 must be fp16 [rows, dim rounded up to 32]");
  if (has(bias)) TORCH_CHECK(bias->numel() == dim, "bias must be fp32 [dim]");
  if (n_tok == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(hidden.device());
  ok(crs_token_project(hidden.data_ptr<float>(), w16.data_ptr(), (const float*)opt_ptr(bias), dst.data_ptr<int64_t>(), out16.data_ptr(),
                       n_tok, (int)H, (int)dim, cur_stream(hidden)), "crs::token_project");
}

// q16 fp16 [nq, lq_max, dimp]; q_len int32 [nq]; tok16 fp16 [>= n_tokens, dimp]; offsets int64 [>= n_rows + 1]; rows int64 /
// out fp32 [nq, m_max]
void maxsim(const Tensor& q16, const Tensor& q_len, const Tensor& tok16, int64_t n_tokens, const Tensor& offsets, int64_t n_rows,
            const Tensor& rows, Tensor out) {
  want(q16, at::kHalf, "q16");
  want(q_len, at::kInt, "q_len");
  want(tok16, at::kHalf, "tok16");
  want(offsets, at::kLong, "offsets");
  want(rows, at::kLong, "rows");
  want(out, at::kFloat, "out");
  same_device(q16, {&q_len, &tok16, &offsets, &rows, &out}, "crs::maxsim");
  TORCH_CHECK(q16.dim() == 3 && q16.size(1) >= 1 && q16.size(1) <= CRS_MAXSIM_MAX_QUERY, "q16 must be fp16 [nq, lq_max <= 64, dimp]");
  const int64_t nq = q16.size(0), dimp = q16.size(2);
  TORCH_CHECK(nq <= 65535, "too many queries");
  TORCH_CHECK(dimp == 32 || dimp == 64 || dimp == 96 || dimp == 128, "dimp must be 32, 64, 96 or 128");
  TORCH_CHECK(q_len.dim() == 1 && q_len.size(0) == nq, "q_len must be int32 [nq]");
  TORCH_CHECK(tok16.dim() == 2 && tok16.size(1) == dimp && n_tokens >= 0 && n_tokens <= tok16.size(0), "tok16 must be fp16 [>= n_tokens, dimp]");
  TORCH_CHECK(n_rows >= 0 && offsets.dim() == 1 && offsets.numel() >= n_rows + 1, "offsets must be int64 [>= n_rows + 1]");
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) == nq && rows.size(1) >= 1 && rows.size(1) <= 0x7fffffff && out.sizes() == rows.sizes(),
              "rows / out must be [nq, m_max >= 1]");
  if (nq == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(q16.device());
  ok(crs_maxsim(q16.data_ptr(), q_len.data_ptr<int32_t>(), (int)nq, (int)q16.size(1), n_tokens ? tok16.data_ptr() : nullptr,
                offsets.data_ptr<int64_t>(), n_rows, n_tokens, rows.data_ptr<int64_t>(), (int)rows.size(1), (int)dimp,
                out.data_ptr<float>(), cur_stream(q16)), "crs::maxsim");
}

// ---- near-duplicate join (csrc/join.hip) ---------------------------------------------------------------------------
// slab fp16 [>= n_rows, pdim]; pairs int64 [cap, 2], scores fp32 [cap]; count int64 [1], zeroed by the caller, receives the number
// of qualifying pairs (count > cap: overflow)
void pairs_above_out(const Tensor& slab, int64_t n_rows, int64_t dim, int64_t a_first, int64_t a_rows, int64_t b_first, int64_t b_rows,
                     double thr, Tensor pairs, Tensor scores, Tensor count) {
  want(slab, at::kHalf, "slab");
  want(pairs, at::kLong, "pairs");
  want(scores, at::kFloat, "scores");
  want(count, at::kLong, "count");
  same_device(slab, {&pairs, &scores, &count}, "crs::pairs_above");
  TORCH_CHECK(dim >= 1 && dim <= 1024, "dim must be in 1..1024");
  TORCH_CHECK(slab.dim() == 2 && slab.size(1) == crs_padded_dim((int)dim), "slab must be fp16 [rows, crs_padded_dim(dim)]");
  TORCH_CHECK(n_rows >= 0 && n_rows <= slab.size(0), "n_rows exceeds the slab");
  TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2 && scores.dim() == 1 && scores.size(0) == pairs.size(0),
              "pairs must be int64 [cap, 2] and scores fp32 [cap]");
  TORCH_CHECK(count.numel() == 1, "count must hold one int64");
  const int64_t cap = pairs.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA g(slab.device());
  ok(crs_pairs_above_f16(slab.data_ptr(), n_rows, (int)dim, a_first, a_rows, b_first, b_rows, (float)thr,
                         cap ? pairs.data_ptr<int64_t>() : nullptr, cap ? scores.data_ptr<float>() : nullptr, cap, count.data_ptr<int64_t>(),
                         cur_stream(slab)), "crs::pairs_above");
}

// pairs int64 [m, 2]; shadow fp32 [>= n_rows, dim]; rows_a / rows_b int64 [>= m], sims fp32 [>= m]; count int64 [1], zeroed by the caller
void pairs_verify_out(const Tensor& pairs, const Tensor& shadow, int64_t n_rows, double thr, Tensor rows_a, Tensor rows_b, Tensor sims,
                      Tensor count) {
  want(pairs, at::kLong, "pairs");
  want(shadow, at::kFloat, "shadow");
  want(rows_a, at::kLong, "rows_a");
  want(rows_b, at::kLong, "rows_b");
  want(sims, at::kFloat, "sims");
  want(count, at::kLong, "count");
  same_device(pairs, {&shadow, &rows_a, &rows_b, &sims, &count}, "crs::pairs_verify");
  TORCH_CHECK(pairs.dim() == 2 && pairs.size(1) == 2, "pairs must be int64 [m, 2]");
  TORCH_CHECK(shadow.dim() == 2 && shadow.size(1) >= 1 && shadow.size(1) <= 1024 && n_rows >= 0 && n_rows <= shadow.size(0),
              "shadow must be fp32 [>= n_rows, dim], dim in 1..1024");
  const int64_t m = pairs.size(0);
  TORCH_CHECK(rows_a.numel() >= m && rows_b.numel() >= m && sims.numel() >= m, "rows_a / rows_b / sims must hold m entries");
  TORCH_CHECK(count.numel() == 1, "count must hold one int64");
  if (m == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(pairs.device());
  ok(crs_pairs_verify_f32(pairs.data_ptr<int64_t>(), m, shadow.data_ptr<float>(), n_rows, (int)shadow.size(1), (float)thr,
                          rows_a.data_ptr<int64_t>(), rows_b.data_ptr<int64_t>(), sims.data_ptr<float>(), count.data_ptr<int64_t>(),
                          cur_stream(pairs)), "crs::pairs_verify");
}

// ---- hybrid retrieval: BM25 scan (csrc/bm25.hip) and rank fusion (csrc/fuse.hip) ------------------------------------------------------
// doc_offsets int64 [>= n_rows + 1], doc_tokens / doc_tf int32 (same length), doc_len int32 [>= n_rows]; q_offsets int64 [nq + 1],
// q_tokens int32 / q_weights fp32 (same length); workspace uint8 (crs_bm25_workspace_bytes); out_scores fp32 / out_rows int64 [nq, k]
void bm25_topk(const Tensor& doc_offsets, const Tensor& doc_tokens, const Tensor& doc_tf, const Tensor& doc_len, int64_t n_rows,
               const Tensor& q_offsets, const Tensor& q_tokens, const Tensor& q_weights, double c0, double c1, double k1p1, int64_t k,
               Tensor workspace, Tensor out_scores, Tensor out_rows) {
  want(doc_offsets, at::kLong, "doc_offsets");
  want(doc_tokens, at::kInt, "doc_tokens");
  want(doc_tf, at::kInt, "doc_tf");
  want(doc_len, at::kInt, "doc_len");
  want(q_offsets, at::kLong, "q_offsets");
  want(q_tokens, at::kInt, "q_tokens");
  want(q_weights, at::kFloat, "q_weights");
  want(workspace, at::kByte, "workspace");
  want(out_scores, at::kFloat, "out_scores");
  want(out_rows, at::kLong, "out_rows");
  same_device(doc_offsets, {&doc_tokens, &doc_tf, &doc_len, &q_offsets, &q_tokens, &q_weights, &workspace, &out_scores, &out_rows},
              "crs::bm25_topk");
  TORCH_CHECK(n_rows >= 0 && doc_offsets.dim() == 1 && doc_offsets.numel() >= n_rows + 1, "doc_offsets must be int64 [>= n_rows + 1]");
  TORCH_CHECK(doc_len.dim() == 1 && doc_len.numel() >= n_rows, "doc_len must be int32 [>= n_rows]");
  TORCH_CHECK(doc_tokens.dim() == 1 && doc_tf.dim() == 1 && doc_tf.numel() == doc_tokens.numel(), "doc_tokens / doc_tf must be int32 of one length");
  TORCH_CHECK(q_offsets.dim() == 1 && q_offsets.numel() >= 2, "q_offsets must be int64 [nq + 1]");
  const int64_t nq = q_offsets.numel() - 1;
  TORCH_CHECK(q_tokens.dim() == 1 && q_weights.dim() == 1 && q_weights.numel() == q_tokens.numel(), "q_tokens / q_weights must be of one length");
  TORCH_CHECK(nq <= 64 && k >= 1 && k <= CRS_MAX_K, "at most 64 queries per launch, 1 <= k <= 64");
  TORCH_CHECK(out_scores.numel() == nq * k && out_rows.numel() == nq * k, "outputs must hold [nq, k]");
  c10::hip::HIPGuardMasqueradingAsCUDA g(doc_offsets.device());
  ok(crs_bm25_topk(doc_offsets.data_ptr<int64_t>(), doc_tokens.numel() ? doc_tokens.data_ptr<int32_t>() : nullptr,
                   doc_tf.numel() ? doc_tf.data_ptr<int32_t>() : nullptr, doc_len.numel() ? doc_len.data_ptr<int32_t>() : nullptr, n_rows,
                   doc_tokens.numel(), q_offsets.data_ptr<int64_t>(), q_tokens.numel() ? q_tokens.data_ptr<int32_t>() : nullptr,
                   q_weights.numel() ? q_weights.data_ptr<float>() : nullptr, (int)nq, q_tokens.numel(), (float)c0, (float)c1, (float)k1p1,
                   (int)k, workspace.data_ptr(), (size_t)workspace.numel(), out_scores.data_ptr<float>(), out_rows.data_ptr<int64_t>(),
                   cur_stream(doc_offsets)), "crs::bm25_topk");
}

// ---- learned sparse retrieval (csrc/mlm_pool.hip, csrc/sparse_compact.hip, csrc/sparse_scan.hip) ------------------------------------
// hidden fp32 [batch, seq, H] (final hidden states; padding positions are never read); lens int32 [batch]; transform_w16 fp16 [H, H],
// transform_bias / ln_gamma / ln_beta fp32 [H]; decoder_w16 fp16 [V, H]; decoder_bias fp32 [V]; workspace uint8
// (crs_mlm_workspace_bytes; afterwards it begins with t as fp16 [tokens_padded, H]); out fp32 [batch, Vp >= V], columns [0, V) written
void mlm_sparse_pool(const Tensor& hidden, const Tensor& lens, const Tensor& transform_w16, const Tensor& transform_bias,
                     const Tensor& ln_gamma, const Tensor& ln_beta, double ln_eps, const Tensor& decoder_w16, const Tensor& decoder_bias,
                     int64_t max_pos, Tensor workspace, Tensor out) {
  want(hidden, at::kFloat, "hidden");
  want(lens, at::kInt, "lens");
  want(transform_w16, at::kHalf, "transform_w16");
  want(transform_bias, at::kFloat, "transform_bias");
  want(ln_gamma, at::kFloat, "ln_gamma");
  want(ln_beta, at::kFloat, "ln_beta");
  want(decoder_w16, at::kHalf, "decoder_w16");
  want(decoder_bias, at::kFloat, "decoder_bias");
  want(workspace, at::kByte, "workspace");
  want(out, at::kFloat, "out");
  same_device(hidden, {&lens, &transform_w16, &transform_bias, &ln_gamma, &ln_beta, &decoder_w16, &decoder_bias, &workspace, &out},
              "crs::mlm_sparse_pool");
  TORCH_CHECK(hidden.dim() == 3 && hidden.size(0) >= 1 && hidden.size(1) >= 1, "hidden must be fp32 [batch >= 1, seq >= 1, H]");
  const int64_t batch = hidden.size(0), seq = hidden.size(1), H = hidden.size(2);
  TORCH_CHECK(batch * seq <= (1 << 22), "too many tokens (batch * seq <= 2^22)");
  TORCH_CHECK(lens.dim() == 1 && lens.size(0) == batch, "lens must be int32 [batch]");
  TORCH_CHECK(transform_w16.dim() == 2 && transform_w16.size(0) == H && transform_w16.size(1) == H, "transform_w16 must be fp16 [H, H]");
  TORCH_CHECK(transform_bias.numel() == H && ln_gamma.numel() == H && ln_beta.numel() == H, "transform_bias / ln_gamma / ln_beta must be fp32 [H]");
  TORCH_CHECK(decoder_w16.dim() == 2 && decoder_w16.size(1) == H && decoder_w16.size(0) >= 1 && decoder_w16.size(0) <= (1 << 20),
              "decoder_w16 must be fp16 [V, H]");
  const int64_t V = decoder_w16.size(0);
  TORCH_CHECK(decoder_bias.numel() == V, "decoder_bias must be fp32 [V]");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == batch && out.size(1) >= V && out.size(1) <= 0x7fffffff, "out must be fp32 [batch, Vp >= V]");
  crs_mlm_head head;
  head.hidden = (int32_t)H;
  head.vocab = (int32_t)V;
  head.max_pos = (int32_t)max_pos;
  head.ln_eps = (float)ln_eps;
  head.transform_w16 = transform_w16.data_ptr();
  head.transform_bias = transform_bias.data_ptr<float>();
  head.ln_gamma = ln_gamma.data_ptr<float>();
  head.ln_beta = ln_beta.data_ptr<float>();
  head.decoder_w16 = decoder_w16.data_ptr();
  head.decoder_bias = decoder_bias.data_ptr<float>();
  c10::hip::HIPGuardMasqueradingAsCUDA g(hidden.device());
  ok(crs_mlm_sparse_pool(hidden.data_ptr<float>(), lens.data_ptr<int32_t>(), (int)batch, (int)seq, &head, workspace.data_ptr(),
                         (size_t)workspace.numel(), out.data_ptr<float>(), (int)out.size(1), cur_stream(hidden)), "crs::mlm_sparse_pool");
}

// weights fp32 [batch, Vp >= vocab]; skip_ids int32 [<= CRS_SPARSE_MAX_SKIP] (optional); ids int32 / out_weights fp32 [batch, cap];
// counts int32 [batch]
void sparse_compact(const Tensor& weights, int64_t vocab, c10::optional<Tensor> skip_ids, Tensor ids, Tensor out_weights, Tensor counts) {
  want(weights, at::kFloat, "weights");
  want(ids, at::kInt, "ids");
  want(out_weights, at::kFloat, "out_weights");
  want(counts, at::kInt, "counts");
  if (has(skip_ids)) want(*skip_ids, at::kInt, "skip_ids");
  same_device(weights, {opt_t(skip_ids), &ids, &out_weights, &counts}, "crs::sparse_compact");
  TORCH_CHECK(weights.dim() == 2 && weights.size(0) >= 1 && weights.size(1) <= 0x7fffffff && weights.size(0) <= 0x7fffffff,
              "weights must be fp32 [batch >= 1, Vp]");
  const int64_t batch = weights.size(0);
  TORCH_CHECK(vocab >= 1 && vocab <= weights.size(1), "vocab must be in 1..Vp");
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == batch && ids.size(1) >= 1 && ids.size(1) <= CRS_SPARSE_MAX_TERMS && out_weights.sizes() == ids.sizes(),
              "ids / out_weights must be [batch, 1 <= cap <= CRS_SPARSE_MAX_TERMS]");
  TORCH_CHECK(counts.dim() == 1 && counts.size(0) == batch, "counts must be int32 [batch]");
  const int64_t n_skip = has(skip_ids) ? skip_ids->numel() : 0;
  TORCH_CHECK(n_skip <= CRS_SPARSE_MAX_SKIP, "at most CRS_SPARSE_MAX_SKIP skip ids");
  c10::hip::HIPGuardMasqueradingAsCUDA g(weights.device());
  ok(crs_sparse_compact(weights.data_ptr<float>(), (int)batch, (int)vocab, (int)weights.size(1), (int)ids.size(1),
                        n_skip ? skip_ids->data_ptr<int32_t>() : nullptr, (int)n_skip, ids.data_ptr<int32_t>(), out_weights.data_ptr<float>(),
                        counts.data_ptr<int32_t>(), cur_stream(weights)), "crs::sparse_compact");
}

// doc_offsets int64 [>= n_rows + 1], doc_tokens int32 / doc_weights fp32 (same length); q_offsets int64 [nq + 1], q_tokens int32 /
// q_weights fp32 (same length); workspace uint8 (crs_sparse_workspace_bytes); out_scores fp32 / out_rows int64 [nq, k]
void sparse_topk(const Tensor& doc_offsets, const Tensor& doc_tokens, const Tensor& doc_weights, int64_t n_rows, const Tensor& q_offsets,
                 const Tensor& q_tokens, const Tensor& q_weights, int64_t k, Tensor workspace, Tensor out_scores, Tensor out_rows) {
  want(doc_offsets, at::kLong, "doc_offsets");
  want(doc_tokens, at::kInt, "doc_tokens");
  want(doc_weights, at::kFloat, "doc_weights");
  want(q_offsets, at::kLong, "q_offsets");
  want(q_tokens, at::kInt, "q_tokens");
  want(q_weights, at::kFloat, "q_weights");
  want(workspace, at::kByte, "workspace");
  want(out_scores, at::kFloat, "out_scores");
  want(out_rows, at::kLong, "out_rows");
  same_device(doc_offsets, {&doc_tokens, &doc_weights, &q_offsets, &q_tokens, &q_weights, &workspace, &out_scores, &out_rows}, "crs::sparse_topk");
  TORCH_CHECK(n_rows >= 0 && doc_offsets.dim() == 1 && doc_offsets.numel() >= n_rows + 1, "doc_offsets must be int64 [>= n_rows + 1]");
  TORCH_CHECK(doc_tokens.dim() == 1 && doc_weights.dim() == 1 && doc_weights.numel() == doc_tokens.numel(),
              "doc_tokens / doc_weights must be of one length");
  TORCH_CHECK(q_offsets.dim() == 1 && q_offsets.numel() >= 2, "q_offsets must be int64 [nq + 1]");
  const int64_t nq = q_offsets.numel() - 1;
  TORCH_CHECK(q_tokens.dim() == 1 && q_weights.dim() == 1 && q_weights.numel() == q_tokens.numel(), "q_tokens / q_weights must be of one length");
  TORCH_CHECK(nq <= 64 && k >= 1 && k <= CRS_MAX_K, "at most 64 queries per launch, 1 <= k <= 64");
  TORCH_CHECK(out_scores.numel() == nq * k && out_rows.numel() == nq * k, "outputs must hold [nq, k]");
  c10::hip::HIPGuardMasqueradingAsCUDA g(doc_offsets.device());
  ok(crs_sparse_topk(doc_offsets.data_ptr<int64_t>(), doc_tokens.numel() ? doc_tokens.data_ptr<int32_t>() : nullptr,
                     doc_weights.numel() ? doc_weights.data_ptr<float>() : nullptr, n_rows, doc_tokens.numel(), q_offsets.data_ptr<int64_t>(),
                     q_tokens.numel() ? q_tokens.data_ptr<int32_t>() : nullptr, q_weights.numel() ? q_weights.data_ptr<float>() : nullptr,
                     (int)nq, q_tokens.numel(), (int)k, workspace.data_ptr(), (size_t)workspace.numel(), out_scores.data_ptr<float>(),
                     out_rows.data_ptr<int64_t>(), cur_stream(doc_offsets)), "crs::sparse_topk");
}

// dense_rows int64 [nq, m_dense], lex_rows int64 [nq, m_lex]; rows int64 / fused fp64 / dense_pos, lex_pos int32 [nq, k_out]; count int32 [nq]
void fuse_rrf(const Tensor& dense_rows, const Tensor& lex_rows, double c, double w_dense, double w_lex, Tensor rows, Tensor fused,
              Tensor dense_pos, Tensor lex_pos, Tensor count) {
  want(dense_rows, at::kLong, "dense_rows");
  want(lex_rows, at::kLong, "lex_rows");
  want(rows, at::kLong, "rows");
  want(fused, at::kDouble, "fused");
  want(dense_pos, at::kInt, "dense_pos");
  want(lex_pos, at::kInt, "lex_pos");
  want(count, at::kInt, "count");
  same_device(dense_rows, {&lex_rows, &rows, &fused, &dense_pos, &lex_pos, &count}, "crs::fuse_rrf");
  TORCH_CHECK(dense_rows.dim() == 2 && lex_rows.dim() == 2 && lex_rows.size(0) == dense_rows.size(0), "dense_rows [nq, m_dense], lex_rows [nq, m_lex]");
  const int64_t nq = dense_rows.size(0);
  TORCH_CHECK(nq <= 0x7fffffff, "too many lists");
  TORCH_CHECK(rows.dim() == 2 && rows.size(0) == nq && fused.sizes() == rows.sizes() && dense_pos.sizes() == rows.sizes() &&
              lex_pos.sizes() == rows.sizes(), "rows / fused / dense_pos / lex_pos must be [nq, k_out]");
  TORCH_CHECK(count.numel() == nq, "count must be int32 [nq]");
  TORCH_CHECK(dense_rows.size(1) <= 0x7fffffff && lex_rows.size(1) <= 0x7fffffff && rows.size(1) <= 0x7fffffff, "sizes out of range");
  if (nq == 0) return;
  c10::hip::HIPGuardMasqueradingAsCUDA g(dense_rows.device());
  ok(crs_fuse_rrf(dense_rows.data_ptr<int64_t>(), (int)dense_rows.size(1), lex_rows.data_ptr<int64_t>(), (int)lex_rows.size(1), (int)nq, c,
                  w_dense, w_lex, (int)rows.size(1), rows.data_ptr<int64_t>(), fused.data_ptr<double>(), dense_pos.data_ptr<int32_t>(),
                  lex_pos.data_ptr<int32_t>(), count.data_ptr<int32_t>(), cur_stream(dense_rows)), "crs::fuse_rrf");
}

// ---- tokenisation (csrc/wordpiece.hip) ------------------------------------------------------------------------------------------------
// text uint8 [n_bytes], offsets int64 [n + 1]; table / rep_pool / vocab_pool int32 holding the uint32 bit patterns; slots int32 [n_slots, 4];
// ids int32 [n, max_len], lens / flags int32 [n]
void wordpiece_encode(const Tensor& text, const Tensor& offsets, int64_t n_bytes, const Tensor& table, const Tensor& rep_pool,
                      const Tensor& slots, const Tensor& vocab_pool, int64_t max_probe, int64_t lmax, int64_t mode, int64_t unk_id,
                      int64_t cls_id, int64_t sep_id, int64_t pad_id, int64_t hash_lo, int64_t hash_span, Tensor ids, Tensor lens,
                      Tensor flags) {
  want(text, at::kByte, "text");
  want(offsets, at::kLong, "offsets");
  want(table, at::kInt, "table");
  want(rep_pool, at::kInt, "rep_pool");
  want(slots, at::kInt, "slots");
  want(vocab_pool, at::kInt, "vocab_pool");
  want(ids, at::kInt, "ids");
  want(lens, at::kInt, "lens");
  want(flags, at::kInt, "flags");
  same_device(text, {&offsets, &table, &rep_pool, &slots, &vocab_pool, &ids, &lens, &flags}, "crs::wordpiece_encode");
  TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 1, "offsets must be int64 [n + 1]");
  const int64_t n = offsets.numel() - 1;
  TORCH_CHECK(n <= 0x7fffffff, "too many texts");
  TORCH_CHECK(n_bytes >= 0 && n_bytes <= text.numel(), "n_bytes exceeds text");
  TORCH_CHECK(slots.dim() == 2 && slots.size(1) == 4, "slots must be int32 [n_slots, 4]");
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == n && lens.numel() == n && flags.numel() == n, "ids [n, max_len], lens [n], flags [n]");
  TORCH_CHECK(ids.size(1) <= 0x7fffffff, "max_len out of range");
  c10::hip::HIPGuardMasqueradingAsCUDA g(text.device());
  ok(crs_wordpiece_encode(text.data_ptr<uint8_t>(), offsets.data_ptr<int64_t>(), (int)n, n_bytes, (const uint32_t*)table.data_ptr<int32_t>(),
                          table.numel(), (const uint32_t*)rep_pool.data_ptr<int32_t>(), rep_pool.numel(), slots.data_ptr<int32_t>(),
                          slots.size(0), (const uint32_t*)vocab_pool.data_ptr<int32_t>(), vocab_pool.numel(), (int)max_probe, (int)lmax,
                          (int)mode, (int)unk_id, (int)cls_id, (int)sep_id, (int)pad_id, (int)hash_lo, (int)hash_span, (int)ids.size(1),
                          ids.data_ptr<int32_t>(), lens.data_ptr<int32_t>(), flags.data_ptr<int32_t>(), cur_stream(text)),
     "crs::wordpiece_encode");
}

// csrc/unigram.hip: the same tensors; slot_scores fp64 [n_slots]; opts = CRS_UNIGRAM_* bits
void unigram_encode(const Tensor& text, const Tensor& offsets, int64_t n_bytes, const Tensor& table, const Tensor& rep_pool,
                    const Tensor& slots, const Tensor& slot_scores, const Tensor& vocab_pool, int64_t max_probe, int64_t lmax,
                    double unk_score, int64_t opts, int64_t unk_id, int64_t cls_id, int64_t sep_id, int64_t pad_id, Tensor ids, Tensor lens,
                    Tensor flags) {
  want(text, at::kByte, "text");
  want(offsets, at::kLong, "offsets");
  want(table, at::kInt, "table");
  want(rep_pool, at::kInt, "rep_pool");
  want(slots, at::kInt, "slots");
  want(slot_scores, at::kDouble, "slot_scores");
  want(vocab_pool, at::kInt, "vocab_pool");
  want(ids, at::kInt, "ids");
  want(lens, at::kInt, "lens");
  want(flags, at::kInt, "flags");
  same_device(text, {&offsets, &table, &rep_pool, &slots, &slot_scores, &vocab_pool, &ids, &lens, &flags}, "crs::unigram_encode");
  TORCH_CHECK(offsets.dim() == 1 && offsets.numel() >= 1, "offsets must be int64 [n + 1]");
  const int64_t n = offsets.numel() - 1;
  TORCH_CHECK(n <= 0x7fffffff, "too many texts");
  TORCH_CHECK(n_bytes >= 0 && n_bytes <= text.numel(), "n_bytes exceeds text");
  TORCH_CHECK(slots.dim() == 2 && slots.size(1) == 4, "slots must be int32 [n_slots, 4]");
  TORCH_CHECK(slot_scores.numel() == slots.size(0), "slot_scores must be fp64 [n_slots]");
  TORCH_CHECK(ids.dim() == 2 && ids.size(0) == n && lens.numel() == n && flags.numel() == n, "ids [n, max_len], lens [n], flags [n]");
  TORCH_CHECK(ids.size(1) <= 0x7fffffff, "max_len out of range");
  c10::hip::HIPGuardMasqueradingAsCUDA g(text.device());
  ok(crs_unigram_encode(text.data_ptr<uint8_t>(), offsets.data_ptr<int64_t>(), (int)n, n_bytes, (const uint32_t*)table.data_ptr<int32_t>(),
                        table.numel(), (const uint32_t*)rep_pool.data_ptr<int32_t>(), rep_pool.numel(), slots.data_ptr<int32_t>(),
                        slot_scores.data_ptr<double>(), slots.size(0), (const uint32_t*)vocab_pool.data_ptr<int32_t>(), vocab_pool.numel(),
                        (int)max_probe, (int)lmax, unk_score, (int)opts, (int)unk_id, (int)cls_id, (int)sep_id, (int)pad_id,
                        (int)ids.size(1), ids.data_ptr<int32_t>(), lens.data_ptr<int32_t>(), flags.data_ptr<int32_t>(), cur_stream(text)),
     "crs::unigram_encode");
}

// ---- encoder -------------------------------------------------------------------------------------------------
// desc = [vocab_size, hidden, layers, heads, ffn, max_pos, pooling, flags (CRS_ENC_*, optional)]; weights = [word_emb, pos_emb, type_emb, emb_ln_g, emb_ln_b]
// followed by 12 tensors per layer in crs_encoder_layer order (w_qkv b_qkv w_o b_o ln1_g ln1_b w_up b_up w_down b_down ln2_g ln2_b).
// encoder_forward_ex adds rel_bias (optional): fp32 [heads, 2 * span - 1], the additive relative-position bias of crs_encoder_ext.
// encoder_forward_rope adds rope_table (optional): fp32 [positions, head_dim], crs_encoder_rope's table (descriptors with CRS_ENC_ROTARY);
// an EMPTY pos_emb tensor (weights[1]) is passed as NULL: no position row is added at the embedding step.
// desc + weights of a call as the C structs (the layer array lives in `layers`)
struct EncArgs {
  crs_encoder_desc d;
  std::vector<crs_encoder_layer> layers;
  crs_encoder_weights cw;
};

void enc_args(const Tensor& ids, at::TensorList weights, at::IntArrayRef desc, double ln_eps, EncArgs& a) {
  TORCH_CHECK(desc.size() == 7 || desc.size() == 8, "desc = [vocab_size, hidden, layers, heads, ffn, max_pos, pooling(, flags)]");
  a.d = crs_encoder_desc{(int32_t)desc[0], (int32_t)desc[1], (int32_t)desc[2], (int32_t)desc[3], (int32_t)desc[4], (int32_t)desc[5],
                         (float)ln_eps, (int32_t)desc[6], desc.size() == 8 ? (int32_t)desc[7] : 0};
  TORCH_CHECK((int64_t)weights.size() == 5 + 12 * (int64_t)a.d.layers, "weights must hold 5 + 12 * layers tensors");
  for (const Tensor& t : weights) TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.device() == ids.device(), "weights must be contiguous tensors on the device of ids");
  a.layers.resize((size_t)a.d.layers);
  for (int l = 0; l < a.d.layers; ++l) {
    const Tensor* w = &weights[5 + 12 * l];
    // an EMPTY vector is NULL for the library: b_up (CRS_ENC_GATED_SILU without bias); under CRS_ENC_PRENORM every bias and layer 0's ln1_g
    const auto vec = [](const Tensor& t) { return t.numel() ? (const float*)t.data_ptr() : nullptr; };
    a.layers[l] = crs_encoder_layer{w[0].data_ptr(), vec(w[1]), w[2].data_ptr(), vec(w[3]), vec(w[4]), vec(w[5]), w[6].data_ptr(), vec(w[7]),
                                    w[8].data_ptr(), vec(w[9]), vec(w[10]), vec(w[11])};
  }
  a.cw = crs_encoder_weights{(const float*)weights[0].data_ptr(), weights[1].numel() ? (const float*)weights[1].data_ptr() : nullptr,
                             (const float*)weights[2].data_ptr(),
                             (const float*)weights[3].data_ptr(), (const float*)weights[4].data_ptr(), a.layers.data()};
}

void encoder_forward_rope(const Tensor& ids, const Tensor& lens, at::TensorList weights, at::IntArrayRef desc, double ln_eps, Tensor workspace,
                          Tensor out, c10::optional<Tensor> q16_out, int64_t slab_type, bool normalize, c10::optional<Tensor> hidden_out,
                          c10::optional<Tensor> rel_bias, c10::optional<Tensor> rope_table) {
  want(ids, at::kInt, "ids");
  want(lens, at::kInt, "lens");
  want(out, at::kFloat, "out");
  EncArgs ea;
  enc_args(ids, weights, desc, ln_eps, ea);
  const crs_encoder_desc& d = ea.d;
  const crs_encoder_weights& cw = ea.cw;
  TORCH_CHECK(ids.dim() == 2 && lens.numel() == ids.size(0) && out.numel() == ids.size(0) * d.hidden, "ids [B, S], lens [B], out [B, H]");
  same_device(ids, {&lens, &workspace, &out, opt_t(q16_out), opt_t(hidden_out)}, "crs::encoder_forward");
  const int b = (int)ids.size(0), s = (int)ids.size(1);
  crs_encoder_ext ext{nullptr, 0};
  if (rel_bias.has_value() && rel_bias->defined()) {
    want(*rel_bias, at::kFloat, "rel_bias");
    same_device(ids, {opt_t(rel_bias)}, "crs::encoder_forward_ex");
    TORCH_CHECK(rel_bias->dim() == 2 && rel_bias->size(0) == d.heads && (rel_bias->size(1) & 1) == 1, "rel_bias must be [heads, 2 * span - 1]");
    ext.rel_bias_dev = rel_bias->data_ptr<float>();
    ext.rel_span = (int32_t)((rel_bias->size(1) + 1) / 2);
  }
  crs_encoder_rope rope{nullptr, 0};
  if (rope_table.has_value() && rope_table->defined()) {
    want(*rope_table, at::kFloat, "rope_table");
    same_device(ids, {opt_t(rope_table)}, "crs::encoder_forward_rope");
    TORCH_CHECK(rope_table->dim() == 2 && rope_table->size(1) * d.heads == d.hidden, "rope_table must be [positions, head_dim]");
    rope.table_dev = rope_table->data_ptr<float>();
    rope.positions = (int32_t)rope_table->size(0);
  }
  c10::hip::HIPGuardMasqueradingAsCUDA g(ids.device());
  if (q16_out.has_value() && q16_out->defined()) {
    want(*q16_out, at::kHalf, "q16_out");
    TORCH_CHECK(normalize && !(hidden_out.has_value() && hidden_out->defined()), "q16_out needs normalize=True and no hidden_out");
    TORCH_CHECK(q16_out->numel() == (int64_t)b * crs_row_elems(d.hidden, (int)slab_type), "q16_out must be [B, crs_row_elems(H, slab_type)]");
    ok(crs_encoder_forward_queries_rope(&d, &cw, ids.data_ptr<int32_t>(), lens.data_ptr<int32_t>(), b, s, workspace.data_ptr(),
                                        (size_t)workspace.nbytes(), out.data_ptr<float>(), q16_out->data_ptr(), (int)slab_type, cur_stream(ids), &ext,
                                        &rope),
       "crs::encoder_forward");
    return;
  }
  float* hid = nullptr;
  if (hidden_out.has_value() && hidden_out->defined()) {
    want(*hidden_out, at::kFloat, "hidden_out");
    TORCH_CHECK(hidden_out->numel() == (int64_t)b * s * d.hidden, "hidden_out must be [B, S, H]");
    hid = hidden_out->data_ptr<float>();
  }
  ok(crs_encoder_forward_rope(&d, &cw, ids.data_ptr<int32_t>(), lens.data_ptr<int32_t>(), b, s, workspace.data_ptr(), (size_t)workspace.nbytes(),
                              out.data_ptr<float>(), normalize ? 1 : 0, hid, cur_stream(ids), &ext, &rope), "crs::encoder_forward");
}

// encoder_forward_prenorm: descriptors with CRS_ENC_PRENORM (crs_encoder_prenorm): the two rope tables fp32 [positions, head_dim], the
// window, the full-attention period, the final norm's gain and (optional) bias
void encoder_forward_prenorm(const Tensor& ids, const Tensor& lens, at::TensorList weights, at::IntArrayRef desc, double ln_eps, Tensor workspace,
                             Tensor out, c10::optional<Tensor> q16_out, int64_t slab_type, bool normalize, c10::optional<Tensor> hidden_out,
                             const Tensor& rope_global, const Tensor& rope_local, int64_t window, int64_t global_every, const Tensor& final_ln_g,
                             c10::optional<Tensor> final_ln_b) {
  want(ids, at::kInt, "ids");
  want(lens, at::kInt, "lens");
  want(out, at::kFloat, "out");
  want(rope_global, at::kFloat, "rope_global");
  want(rope_local, at::kFloat, "rope_local");
  want(final_ln_g, at::kFloat, "final_ln_g");
  EncArgs ea;
  enc_args(ids, weights, desc, ln_eps, ea);
  const crs_encoder_desc& d = ea.d;
  TORCH_CHECK(ids.dim() == 2 && lens.numel() == ids.size(0) && out.numel() == ids.size(0) * d.hidden, "ids [B, S], lens [B], out [B, H]");
  same_device(ids, {&lens, &workspace, &out, opt_t(q16_out), opt_t(hidden_out), &rope_global, &rope_local, &final_ln_g, opt_t(final_ln_b)},
              "crs::encoder_forward_prenorm");
  TORCH_CHECK(rope_global.dim() == 2 && rope_global.size(1) * d.heads == d.hidden && rope_local.sizes() == rope_global.sizes(),
              "rope_global and rope_local must both be [positions, head_dim]");
  TORCH_CHECK(final_ln_g.numel() == d.hidden, "final_ln_g must be [H]");
  TORCH_CHECK(window >= INT32_MIN && window <= INT32_MAX && global_every >= INT32_MIN && global_every <= INT32_MAX, "window / global_every out of range");
  crs_encoder_prenorm pre{rope_global.data_ptr<float>(), rope_local.data_ptr<float>(), (int32_t)rope_global.size(0), (int32_t)window,
                          (int32_t)global_every, final_ln_g.data_ptr<float>(), nullptr};
  if (final_ln_b.has_value() && final_ln_b->defined() && final_ln_b->numel()) {
    want(*final_ln_b, at::kFloat, "final_ln_b");
    TORCH_CHECK(final_ln_b->numel() == d.hidden, "final_ln_b must be [H]");
    pre.final_ln_b = final_ln_b->data_ptr<float>();
  }
  const int b = (int)ids.size(0), s = (int)ids.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA g(ids.device());
  if (q16_out.has_value() && q16_out->defined()) {
    want(*q16_out, at::kHalf, "q16_out");
    TORCH_CHECK(normalize && !(hidden_out.has_value() && hidden_out->defined()), "q16_out needs normalize=True and no hidden_out");
    TORCH_CHECK(q16_out->numel() == (int64_t)b * crs_row_elems(d.hidden, (int)slab_type), "q16_out must be [B, crs_row_elems(H, slab_type)]");
    ok(crs_encoder_forward_queries_prenorm(&d, &ea.cw, ids.data_ptr<int32_t>(), lens.data_ptr<int32_t>(), b, s, workspace.data_ptr(),
                                           (size_t)workspace.nbytes(), out.data_ptr<float>(), q16_out->data_ptr(), (int)slab_type, cur_stream(ids), &pre),
       "crs::encoder_forward_prenorm");
    return;
  }
  float* hid = nullptr;
  if (hidden_out.has_value() && hidden_out->defined()) {
    want(*hidden_out, at::kFloat, "hidden_out");
    TORCH_CHECK(hidden_out->numel() == (int64_t)b * s * d.hidden, "hidden_out must be [B, S, H]");
    hid = hidden_out->data_ptr<float>();
  }
  ok(crs_encoder_forward_prenorm(&d, &ea.cw, ids.data_ptr<int32_t>(), lens.data_ptr<int32_t>(), b, s, workspace.data_ptr(), (size_t)workspace.nbytes(),
                                 out.data_ptr<float>(), normalize ? 1 : 0, hid, cur_stream(ids), &pre), "crs::encoder_forward_prenorm");
}

void encoder_forward_ex(const Tensor& ids, const Tensor& lens, at::TensorList weights, at::IntArrayRef desc, double ln_eps, Tensor workspace,
                        Tensor out, c10::optional<Tensor> q16_out, int64_t slab_type, bool normalize, c10::optional<Tensor> hidden_out,
                        c10::optional<Tensor> rel_bias) {
  encoder_forward_rope(ids, lens, weights, desc, ln_eps, workspace, out, q16_out, slab_type, normalize, hidden_out, rel_bias, c10::nullopt);
}

void encoder_forward(const Tensor& ids, const Tensor& lens, at::TensorList weights, at::IntArrayRef desc, double ln_eps, Tensor workspace,
                     Tensor out, c10::optional<Tensor> q16_out, int64_t slab_type, bool normalize, c10::optional<Tensor> hidden_out) {
  encoder_forward_ex(ids, lens, weights, desc, ln_eps, workspace, out, q16_out, slab_type, normalize, hidden_out, c10::nullopt);
}

// Sentence-pair scores (crs_encoder_score_pairs): weights / desc as encoder_forward; head = [w_pool [H, H], b_pool [H], w_cls [H] (or
// [1, H]), b_cls [1]], all fp32; type_ids (optional) int32 [B, S]; activation 0 logit, 1 sigmoid.  type_rows is weights[2]'s row count.
void encoder_score_pairs(const Tensor& ids, c10::optional<Tensor> type_ids, const Tensor& lens, at::TensorList weights, at::TensorList head,
                         at::IntArrayRef desc, double ln_eps, int64_t activation, Tensor workspace, Tensor scores,
                         c10::optional<Tensor> pooled_out, c10::optional<Tensor> hidden_out) {
  want(ids, at::kInt, "ids");
  want(lens, at::kInt, "lens");
  want(scores, at::kFloat, "scores");
  EncArgs ea;
  enc_args(ids, weights, desc, ln_eps, ea);
  const int64_t H = ea.d.hidden;
  TORCH_CHECK(ids.dim() == 2 && lens.numel() == ids.size(0) && scores.numel() == ids.size(0), "ids [B, S], lens [B], scores [B]");
  same_device(ids, {&lens, &workspace, &scores, opt_t(type_ids), opt_t(pooled_out), opt_t(hidden_out)}, "crs::encoder_score_pairs");
  TORCH_CHECK(head.size() == 4, "head = [w_pool, b_pool, w_cls, b_cls]");
  for (const Tensor& t : head) {
    want(t, at::kFloat, "head tensor");
    same_device(ids, {&t}, "crs::encoder_score_pairs");
  }
  TORCH_CHECK(head[0].numel() == H * H && head[1].numel() == H && head[2].numel() == H && head[3].numel() == 1,
              "head must be w_pool [H, H], b_pool [H], w_cls [H], b_cls [1] (one label)");
  TORCH_CHECK(weights[2].dim() == 2 && weights[2].size(1) == H, "weights[2] (token types) must be [rows, H]");
  const int b = (int)ids.size(0), s = (int)ids.size(1);
  const int32_t* types = nullptr;
  if (has(type_ids)) {
    want(*type_ids, at::kInt, "type_ids");
    TORCH_CHECK(type_ids->numel() == ids.numel(), "type_ids must be [B, S]");
    types = type_ids->data_ptr<int32_t>();
  }
  float *pooled = nullptr, *hid = nullptr;
  if (has(pooled_out)) {
    want(*pooled_out, at::kFloat, "pooled_out");
    TORCH_CHECK(pooled_out->numel() == (int64_t)b * H, "pooled_out must be [B, H]");
    pooled = pooled_out->data_ptr<float>();
  }
  if (has(hidden_out)) {
    want(*hidden_out, at::kFloat, "hidden_out");
    TORCH_CHECK(hidden_out->numel() == (int64_t)b * s * H, "hidden_out must be [B, S, H]");
    hid = hidden_out->data_ptr<float>();
  }
  const crs_encoder_head hd{head[0].data_ptr<float>(), head[1].data_ptr<float>(), head[2].data_ptr<float>(), head[3].data_ptr<float>(),
                            (int32_t)weights[2].size(0), (int32_t)activation};
  c10::hip::HIPGuardMasqueradingAsCUDA g(ids.device());
  ok(crs_encoder_score_pairs(&ea.d, &ea.cw, &hd, ids.data_ptr<int32_t>(), types, lens.data_ptr<int32_t>(), b, s, workspace.data_ptr(),
                             (size_t)workspace.nbytes(), scores.data_ptr<float>(), pooled, hid, cur_stream(ids)), "crs::encoder_score_pairs");
}

}  // namespace

TORCH_LIBRARY(crs, m) {
  m.def("slab_append(Tensor emb, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, int row0, Tensor(d!)? row_err=None) -> ()");
  m.def("slab_write_rows(Tensor emb, Tensor rows, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, int n_rows, Tensor(d!)? row_err=None) -> ()");
  m.def("slab_compact(Tensor dead, int n_rows, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, Tensor(d!)? rows_global, "
        "Tensor(e!) bounce, int first_row=0) -> ()");
  m.def("queries_to_f16(Tensor q32, Tensor(a!) out16, int slab_type) -> ()");
  m.def("rows_norm_max(Tensor emb, Tensor(a!) norm_max) -> ()");
  m.def("slab_append_space(Tensor emb, int space, Tensor norm_scale, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, int row0, "
        "Tensor(d!)? row_err=None) -> ()");
  m.def("slab_write_rows_space(Tensor emb, Tensor rows, int space, Tensor norm_scale, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!)? shadow, "
        "int n_rows, Tensor(d!)? row_err=None) -> ()");
  m.def("slab_rescale_space(int n_rows, int dim, int space, int shift, Tensor(a!) slab, Tensor(b!)? scales, Tensor(c!) shadow, "
        "Tensor(d!)? row_err=None) -> ()");
  m.def("queries_to_space(Tensor q, int space, int slab_type, Tensor norm_scale, Tensor(a!) out32, Tensor(b!) out16) -> ()");
  m.def("space_distances(Tensor q, int space, Tensor shadow, int n_rows, int id_base, Tensor norm_scale, Tensor ids, Tensor(a!) out_dist, "
        "Tensor(b!) out_ids) -> ()");
  m.def("cosine_topk(Tensor q16, Tensor slab, Tensor? scales, int n_rows, int dim, int k, int id_base) -> (Tensor, Tensor)");
  m.def("cosine_topk_out(Tensor q16, Tensor slab, Tensor? scales, int n_rows, int dim, int k, int id_base, Tensor(a!) workspace, "
        "Tensor(b!) out_scores, Tensor(c!) out_ids) -> ()");
  m.def("refine_f32(Tensor q32, Tensor shadow, int n_rows, int id_base, Tensor cand_ids, int k_out) -> (Tensor, Tensor)");
  m.def("refine_f32_out(Tensor q32, Tensor shadow, int n_rows, int id_base, Tensor cand_ids, int k_out, Tensor(a!) out_scores, "
        "Tensor(b!) out_ids) -> ()");
  m.def("score_rows_f32_out(Tensor q32, Tensor shadow, int n_rows, int id_base, Tensor ids, Tensor(a!) scores) -> ()");
  m.def("refine_f32_cert_out(Tensor q32, Tensor q16, Tensor shadow, int n_rows, int id_base, Tensor cand_ids, Tensor cand_scores, int k_out, "
        "float row_err_max, int slab_type, Tensor(a!) out_scores, Tensor(b!) out_ids, Tensor(c!) status, Tensor(d!) exact_ws, int cap) -> ()");
  m.def("cosine_topk_cert_out(Tensor q32, Tensor q16, Tensor slab, Tensor? scales, Tensor shadow, int n_rows, int id_base, int k_out, "
        "float row_err_max, Tensor(a!) workspace, Tensor(b!) cand_scores, Tensor(c!) cand_ids, Tensor(d!) out_scores, Tensor(e!) out_ids, "
        "Tensor(f!) status, Tensor(g!) exact_ws, int cap) -> ()");
  m.def("escalate_exact(Tensor q32, Tensor q16, Tensor slab, Tensor? scales, Tensor shadow, int n_rows, int id_base, int k_out, "
        "Tensor(a!) out_scores, Tensor(b!) out_ids, Tensor(c!) status, Tensor(d!) exact_ws, int cap) -> ()");
  m.def("cosine_topk_large_cert_out(Tensor q32, Tensor q16, Tensor slab, Tensor? scales, Tensor shadow, int n_rows, int id_base, "
        "int k_out, float row_err_max, Tensor(a!) workspace, Tensor(b!) out_scores, Tensor(c!) out_ids, Tensor(d!) status, "
        "Tensor(e!) exact_ws, int cap) -> ()");
  m.def("refine_large_cert_out(Tensor q32, Tensor q16, Tensor shadow, int n_rows, int id_base, Tensor cand_ids, Tensor cand_scores, "
        "int chunk_rows, int k_out, float row_err_max, int slab_type, Tensor(a!) out_scores, Tensor(b!) out_ids, Tensor(c!) status, "
        "Tensor(d!) exact_ws, int cap) -> ()");
  m.def("merge_topk(Tensor scores, Tensor ids, int k_out) -> (Tensor, Tensor)");
  m.def("merge_topk_out(Tensor scores, Tensor ids, int k_out, Tensor(a!) out_scores, Tensor(b!) out_ids) -> ()");
  m.def("merge_topk_wire_out(Tensor wire, int nlists, int nq, int k_in, int k_out, Tensor(a!) out_scores, Tensor(b!) out_ids) -> ()");
  m.def("merge_sorted_out(Tensor scores, Tensor ids, int k_out, Tensor(a!) out_scores, Tensor(b!) out_ids) -> ()");
  m.def("merge_sorted_wire_out(Tensor wire, int nlists, int nq, int k_in, int k_out, Tensor(a!) out_scores, Tensor(b!) out_ids) -> ()");
  m.def("mmr_order_out(Tensor vecs, int n_rows, Tensor rows, Tensor rel, Tensor counts, float lam, Tensor(a!) order) -> ()");
  m.def("token_match_out(Tensor a, Tensor len_a, Tensor b, Tensor len_b, Tensor? w_a, Tensor? w_b, Tensor(a!) out) -> ()");
  m.def("rerank_lexical(Tensor scores, Tensor rows, Tensor doc_offsets, Tensor doc_tokens, int n_rows, Tensor q_offsets, Tensor q_tokens, "
        "Tensor q_norm, int k, float threshold, Tensor(a!) order, Tensor(b!) count, Tensor(c!) sim, Tensor(d!) rr, Tensor(e!) reranked) -> ()");
  m.def("token_project(Tensor hidden, Tensor w16, Tensor? bias, Tensor dst, Tensor(a!) out16) -> ()");
  m.def("maxsim(Tensor q16, Tensor q_len, Tensor tok16, int n_tokens, Tensor offsets, int n_rows, Tensor rows, Tensor(a!) out) -> ()");
  m.def("pairs_above_out(Tensor slab, int n_rows, int dim, int a_first, int a_rows, int b_first, int b_rows, float thr, "
        "Tensor(a!) pairs, Tensor(b!) scores, Tensor(c!) count) -> ()");
  m.def("pairs_verify_out(Tensor pairs, Tensor shadow, int n_rows, float thr, Tensor(a!) rows_a, Tensor(b!) rows_b, Tensor(c!) sims, "
        "Tensor(d!) count) -> ()");
  m.def("bm25_topk(Tensor doc_offsets, Tensor doc_tokens, Tensor doc_tf, Tensor doc_len, int n_rows, Tensor q_offsets, Tensor q_tokens, "
        "Tensor q_weights, float c0, float c1, float k1p1, int k, Tensor(a!) workspace, Tensor(b!) out_scores, Tensor(c!) out_rows) -> ()");
  m.def("fuse_rrf(Tensor dense_rows, Tensor lex_rows, float c, float w_dense, float w_lex, Tensor(a!) rows, Tensor(b!) fused, "
        "Tensor(c!) dense_pos, Tensor(d!) lex_pos, Tensor(e!) count) -> ()");
  m.def("mlm_sparse_pool(Tensor hidden, Tensor lens, Tensor transform_w16, Tensor transform_bias, Tensor ln_gamma, Tensor ln_beta, "
        "float ln_eps, Tensor decoder_w16, Tensor decoder_bias, int max_pos, Tensor(a!) workspace, Tensor(b!) out) -> ()");
  m.def("sparse_compact(Tensor weights, int vocab, Tensor? skip_ids, Tensor(a!) ids, Tensor(b!) out_weights, Tensor(c!) counts) -> ()");
  m.def("sparse_topk(Tensor doc_offsets, Tensor doc_tokens, Tensor doc_weights, int n_rows, Tensor q_offsets, Tensor q_tokens, "
        "Tensor q_weights, int k, Tensor(a!) workspace, Tensor(b!) out_scores, Tensor(c!) out_rows) -> ()");
  m.def("wordpiece_encode(Tensor text, Tensor offsets, int n_bytes, Tensor table, Tensor rep_pool, Tensor slots, Tensor vocab_pool, "
        "int max_probe, int lmax, int mode, int unk_id, int cls_id, int sep_id, int pad_id, int hash_lo, int hash_span, Tensor(a!) ids, "
        "Tensor(b!) lens, Tensor(c!) flags) -> ()");
  m.def("unigram_encode(Tensor text, Tensor offsets, int n_bytes, Tensor table, Tensor rep_pool, Tensor slots, Tensor slot_scores, "
        "Tensor vocab_pool, int max_probe, int lmax, float unk_score, int opts, int unk_id, int cls_id, int sep_id, int pad_id, "
        "Tensor(a!) ids, Tensor(b!) lens, Tensor(c!) flags) -> ()");
  m.def("encoder_forward(Tensor ids, Tensor lens, Tensor[] weights, int[] desc, float ln_eps, Tensor(a!) workspace, Tensor(b!) out, "
        "Tensor(c!)? q16_out, int slab_type, bool normalize, Tensor(d!)? hidden_out) -> ()");
  m.def("encoder_forward_ex(Tensor ids, Tensor lens, Tensor[] weights, int[] desc, float ln_eps, Tensor(a!) workspace, Tensor(b!) out, "
        "Tensor(c!)? q16_out, int slab_type, bool normalize, Tensor(d!)? hidden_out, Tensor? rel_bias=None) -> ()");
  m.def("encoder_forward_rope(Tensor ids, Tensor lens, Tensor[] weights, int[] desc, float ln_eps, Tensor(a!) workspace, Tensor(b!) out, "
        "Tensor(c!)? q16_out, int slab_type, bool normalize, Tensor(d!)? hidden_out, Tensor? rel_bias=None, Tensor? rope_table=None) -> ()");
  m.def("encoder_forward_prenorm(Tensor ids, Tensor lens, Tensor[] weights, int[] desc, float ln_eps, Tensor(a!) workspace, Tensor(b!) out, "
        "Tensor(c!)? q16_out, int slab_type, bool normalize, Tensor(d!)? hidden_out, Tensor rope_global, Tensor rope_local, int window, "
        "int global_every, Tensor final_ln_g, Tensor? final_ln_b=None) -> ()");
  m.def("encoder_score_pairs(Tensor ids, Tensor? type_ids, Tensor lens, Tensor[] weights, Tensor[] head, int[] desc, float ln_eps, "
        "int activation, Tensor(a!) workspace, Tensor(b!) scores, Tensor(c!)? pooled_out, Tensor(d!)? hidden_out) -> ()");
}

TORCH_LIBRARY_IMPL(crs, CUDA, m) {   // the HIP backend of torch-ROCm dispatches under the "CUDA" key
  m.impl("slab_append", &slab_append);
  m.impl("slab_write_rows", &slab_write_rows);
  m.impl("slab_compact", &slab_compact);
  m.impl("queries_to_f16", &queries_to_f16);
  m.impl("rows_norm_max", &rows_norm_max);
  m.impl("slab_append_space", &slab_append_space);
  m.impl("slab_write_rows_space", &slab_write_rows_space);
  m.impl("slab_rescale_space", &slab_rescale_space);
  m.impl("queries_to_space", &queries_to_space);
  m.impl("space_distances", &space_distances);
  m.impl("cosine_topk", &cosine_topk);
  m.impl("cosine_topk_out", &cosine_topk_out);
  m.impl("refine_f32", &refine_f32);
  m.impl("refine_f32_out", &refine_f32_out);
  m.impl("score_rows_f32_out", &score_rows_f32_out);
  m.impl("refine_f32_cert_out", &refine_f32_cert_out);
  m.impl("cosine_topk_cert_out", &cosine_topk_cert_out);
  m.impl("escalate_exact", &escalate_exact);
  m.impl("cosine_topk_large_cert_out", &cosine_topk_large_cert_out);
  m.impl("refine_large_cert_out", &refine_large_cert_out);
  m.impl("merge_topk", &merge_topk);
  m.impl("merge_topk_out", &merge_topk_out);
  m.impl("merge_topk_wire_out", &merge_topk_wire_out);
  m.impl("merge_sorted_out", &merge_sorted_out);
  m.impl("merge_sorted_wire_out", &merge_sorted_wire_out);
  m.impl("mmr_order_out", &mmr_order_out);
  m.impl("token_match_out", &token_match_out);
  m.impl("rerank_lexical", &rerank_lexical);
  m.impl("token_project", &token_project);
  m.impl("maxsim", &maxsim);
  m.impl("pairs_above_out", &pairs_above_out);
  m.impl("pairs_verify_out", &pairs_verify_out);
  m.impl("bm25_topk", &bm25_topk);
  m.impl("fuse_rrf", &fuse_rrf);
  m.impl("mlm_sparse_pool", &mlm_sparse_pool);
  m.impl("sparse_compact", &sparse_compact);
  m.impl("sparse_topk", &sparse_topk);
  m.impl("wordpiece_encode", &wordpiece_encode);
  m.impl("unigram_encode", &unigram_encode);
  m.impl("encoder_forward", &encoder_forward);
  m.impl("encoder_forward_ex", &encoder_forward_ex);
  m.impl("encoder_forward_rope", &encoder_forward_rope);
  m.impl("encoder_forward_prenorm", &encoder_forward_prenorm);
  m.impl("encoder_score_pairs", &encoder_score_pairs);
}
