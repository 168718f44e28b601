/* crs_encoder.h -- C ABI of the sentence-encoder forward in libcrs_hip.so (gfx950).
 *
 * Replaces what runs under `self.model.encode(texts, batch_size, normalize_embeddings=True,
 * convert_to_numpy=True)` at reference rag/embedding.py:65-71: the BertModel forward + Pooling +
 * Normalize of sentence-transformers (not vendored in the reference).  Tokenisation stays on the
 * host; this boundary starts at token ids.
 *
 * Numerics: GEMM operands fp16 (MFMA, fp32 accumulate); residual stream, LayerNorm (eps from the
 * descriptor, 1e-12 for BERT), softmax, GELU (erf form), pooling and the L2 normalisation in fp32.
 * Sequences are right-padded: `lens[b]` tokens of row b are real, the rest are padding.
 * All pointers are device pointers; `stream` is a hipStream_t as void*.  Returns 0 or a negative
 * CRS_E* code (crs_hip.h); message via crs_last_error().
 */
#ifndef CRS_ENCODER_H
#define CRS_ENCODER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CRS_POOL_MEAN 0   /* all-MiniLM-L6-v2: mean over real tokens           */
#define CRS_POOL_CLS 1    /* bge-base-en-v1.5: hidden state of token 0 ([CLS]) */

typedef struct crs_encoder_desc {
  int32_t vocab_size;
  int32_t hidden;      /* H: 384 (MiniLM), 768 (bge-base); multiple of 64, <= 1024 */
  int32_t layers;
  int32_t heads;       /* head_dim = hidden / heads must be 16, 32 or 64          */
  int32_t ffn;         /* intermediate size, multiple of 64                       */
  int32_t max_pos;
  float ln_eps;
  int32_t pooling;     /* CRS_POOL_*                                              */
  int32_t flags;       /* CRS_ENC_* bits (ABI 3); 0 = default kernel selection     */
} crs_encoder_desc;

/* Kernel-form selection for query-batch forwards that run BESIDE a corpus scan (the role-lane layout of
 * rag/_engine.py): only kernel forms of <= 48 KB of LDS per workgroup, so that a forward's workgroups fit on CUs that
 * hold two scan workgroups (2 x 48 KB of 160 KB) instead of waiting for the scan to drain.  Same arithmetic and the same
 * fp16 rounding points; bit-identical results except where the default selection runs the fused QKV + attention kernel
 * (hidden <= 384, head_dim 32 / 64, 16 / 32 / 64-token sequences): there the separate attention kernel sums in another
 * order and the results differ within the encoder's fp16 quantisation error (tests/test_encoder_*_gpu.py).  Slower when
 * the forward runs alone. */
#define CRS_ENC_SMALL_LDS 1

/* Rotary encoders (nomic-embed-text; additive to ABI 3).
 * CRS_ENC_ROTARY: no learned position table (weights->pos_emb may be NULL: no position row is added at the embedding step);
 * instead one rope_qk_kernel launch between the QKV projection and attention rotates the Q and K column blocks of the
 * [T, 3H] fp16 QKV buffer in place, per head, "rotate-half" form (not interleaved), over the whole head dimension:
 *     t'[j]          = t[j]          * cos[pos, j] - t[j + hd/2] * sin[pos, j]          j < hd/2
 *     t'[j + hd/2]   = t[j + hd/2]   * cos[pos, j] + t[j]        * sin[pos, j]
 * read as fp16, computed in fp32, rounded once to fp16; V is not touched.  pos is the token's index in its sequence.  The
 * table is crs_encoder_rope.table_dev: fp32 [positions, hd], row pos holding cos(pos * theta^(-2 j / hd)) for j < hd/2 in
 * its first half and the sines of the same angles in its second half (built on the host in fp64, rounded once to fp32).
 * The flag needs one of the _rope entry points with a table of positions >= seq; it excludes a relative-position bias, and
 * the fused QKV + attention kernel is never selected.  The kernel uses no LDS (CRS_ENC_SMALL_LDS is honoured; under that flag
 * mode 4 runs the panel kernel's <= 48 KB form, except at a hidden size that kernel has no chunk for -- no multiple of 128 --
 * where FFN-up falls to the tiled kernel and its 64 KB of static LDS, as modes 0 / 1 do).
 * CRS_ENC_GATED_SILU: the feed-forward block is gated (SwiGLU): x <- LayerNorm(x + (silu(x Wgate^T + bg) * (x Wup^T + bu)) Wdown^T + b).
 * w_up is then fp16 [2F, H] and b_up fp32 [2F] or NULL, gate and up rows INTERLEAVED IN BLOCKS OF 16: for every block b of
 * 16 output columns, rows [32 b, 32 b + 16) are rows [16 b, 16 b + 16) of Wgate (the half SiLU acts on) and rows
 * [32 b + 16, 32 b + 32) are the same rows of Wup; b_up likewise.  The FFN-up projection runs GEMM mode 4 (below); the
 * [T, 2F] product never exists in memory and the workspace is unchanged.  ffn must be a multiple of 64. */
#define CRS_ENC_ROTARY 2
#define CRS_ENC_GATED_SILU 4

/* Per-layer device pointers.  Matrices are fp16 row-major [out_features, in_features] exactly as
 * torch.nn.Linear stores them (y = x W^T + b); vectors are fp32. */
typedef struct crs_encoder_layer {
  const void* w_qkv;   /* fp16 [3H, H]: query, key, value weights stacked */
  const float* b_qkv;  /* [3H] */
  const void* w_o;     /* fp16 [H, H] */
  const float* b_o;
  const float* ln1_g;  /* attention.output.LayerNorm */
  const float* ln1_b;
  const void* w_up;    /* fp16 [F, H]  intermediate.dense */
  const float* b_up;
  const void* w_down;  /* fp16 [H, F]  output.dense */
  const float* b_down;
  const float* ln2_g;  /* output.LayerNorm */
  const float* ln2_b;
} crs_encoder_layer;

typedef struct crs_encoder_weights {
  const float* word_emb;  /* fp32 [vocab, H] */
  const float* pos_emb;   /* fp32 [max_pos, H] */
  const float* type_emb;  /* fp32 [>=1, H]; row 0 is added to every token (crs_encoder_score_pairs: the row its type ids name) */
  const float* emb_ln_g;
  const float* emb_ln_b;
  const crs_encoder_layer* layers;  /* HOST array of `layers` entries holding device pointers */
} crs_encoder_weights;

int crs_encoder_workspace_bytes(const crs_encoder_desc* d, int batch, int seq, size_t* bytes);

/* ids_dev int32 [batch, seq]; lens_dev int32 [batch] (1 <= len <= seq <= max_pos);
 * out_dev fp32 [batch, H]: pooled (+ L2-normalised when normalize != 0) sentence embeddings.
 * hidden_out_dev (may be NULL): fp32 [batch, seq, H] final hidden states, for parity tests. */
int crs_encoder_forward(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                        const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                        size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                        void* stream);

/* Query-side variant of crs_encoder_forward (always L2-normalised): besides the fp32 embeddings it writes
 * them as the fp16 query block crs_cosine_topk takes -- [batch, crs_row_elems(H, slab_type)], zero padded --
 * from the pooling kernel itself, which saves the separate crs_queries_to_f16 launch on the retrieve path
 * (rag/retrieval.py:113-121: embed the query, then search). */
int crs_encoder_forward_queries(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                                size_t workspace_bytes, float* out_dev, void* q16_out_dev, int slab_type,
                                void* stream);

/* Optional inputs of the _ex entry points (a NULL pointer to it, or a NULL rel_bias_dev, is exactly the forward above).
 * rel_bias_dev: additive relative-position bias of the attention scores, shared by all layers and already resolved
 * per offset -- fp32 [heads, 2 * rel_span - 1], entry (key - query) + rel_span - 1 is added to score(query, key) of that
 * head before the softmax (MPNet: the bucketed relative_attention_bias; bucketing stays on the host).  rel_span >= seq
 * and seq <= 512, else CRS_EINVAL.  Every layer then runs the relative-bias attention kernel (<= 21 KB of LDS, so also
 * under CRS_ENC_SMALL_LDS); the fused QKV + attention kernel and the other attention forms are not selected.
 * Models whose position ids start at an offset p (MPNet: 2) need no more than pos_emb + p * H and max_pos - p in the
 * descriptor; models without token-type embeddings pass a zero row as type_emb. */
typedef struct crs_encoder_ext {
  const float* rel_bias_dev;
  int32_t rel_span;
} crs_encoder_ext;

int crs_encoder_forward_ex(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                           const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                           size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                           void* stream, const crs_encoder_ext* ext);

int crs_encoder_forward_queries_ex(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                   const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                                   size_t workspace_bytes, float* out_dev, void* q16_out_dev, int slab_type,
                                   void* stream, const crs_encoder_ext* ext);

/* The forwards above for descriptors with CRS_ENC_ROTARY (they also serve every other descriptor: a NULL rope, or a NULL
 * table in it, is exactly the _ex entry).  CRS_EINVAL, with a message and before any launch: CRS_ENC_ROTARY without a
 * table, positions < seq, CRS_ENC_ROTARY together with a relative-position bias.  The other entry points of this file refuse
 * a CRS_ENC_ROTARY descriptor (they carry no table). */
typedef struct crs_encoder_rope {
  const float* table_dev;   /* fp32 [positions, head_dim]: cos half | sin half (CRS_ENC_ROTARY above) */
  int32_t positions;
} crs_encoder_rope;

int crs_encoder_forward_rope(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                             const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                             size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                             void* stream, const crs_encoder_ext* ext, const crs_encoder_rope* rope);

int crs_encoder_forward_queries_rope(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                     const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                                     size_t workspace_bytes, float* out_dev, void* q16_out_dev, int slab_type,
                                     void* stream, const crs_encoder_ext* ext, const crs_encoder_rope* rope);

/* Pre-norm encoders with sliding-window layers (ModernBERT; additive to ABI 3).
 * CRS_ENC_PRENORM: every block normalises its INPUT and adds its output to an un-normalised residual stream r,
 *     r <- r + Wo attention(LN1(r)),   r <- r + Wdown ffn(LN2(r)),   hidden states = LN_final(r) after the last layer,
 * with r = the embedding step's LayerNorm output (weights->emb_ln_*) before layer 0.  The layer struct is reused: ln1_g / ln1_b is
 * the norm in front of attention (layer 0 has none: its ln1_g and ln1_b MUST be NULL -- the embedding norm's output feeds its QKV projection -- and every other layer's ln1_g must not),
 * ln2_g / ln2_b the norm in front of the feed-forward block; ln1_b, ln2_b and every projection bias may be NULL.  The flag needs
 * CRS_ENC_ROTARY and one of the _prenorm entry points: TWO rope tables (crs_encoder_rope's layout), one for the full-attention
 * layers and one for the sliding-window layers; layer i attends the whole sequence when i % global_every == 0 and otherwise
 * only the keys with |key - query| <= window (both ends included; ModernBERT's local_attention / 2).  A padding query further
 * than window behind the last real token has no key at all: its context row is zero (finite), and it never reaches a real row.
 * One add_layernorm launch closes a block and opens the next (r is written back and LN(r) leaves as fp16), so a layer has as
 * many launches as a post-norm one; the fused QKV + attention kernel and the fused projection + LayerNorm kernel are never
 * selected.  pos_emb may be NULL.  It excludes a relative-position bias and crs_encoder_score_pairs.
 * CRS_ENC_GATED_GELU: the feed-forward block is GeGLU, Wdown(gelu(x Wa^T) * (x Wb^T)), erf GELU: CRS_ENC_GATED_SILU's layout
 * and kernels (GEMM mode 5) with GELU on the activated half.  For ModernBERT's Wi [2F, H], whose output is chunked into
 * (input, gate), rows [0, F) are the activated half ("gate" rows of the interleaved layout) and rows [F, 2F) the linear half.
 * Not together with CRS_ENC_GATED_SILU. */
#define CRS_ENC_PRENORM 8
#define CRS_ENC_GATED_GELU 16

typedef struct crs_encoder_prenorm {
  const float* rope_global_dev;  /* fp32 [positions, head_dim], full-attention layers (global theta) */
  const float* rope_local_dev;   /* fp32 [positions, head_dim], sliding-window layers (local theta)  */
  int32_t positions;             /* rows of both tables, >= seq                                      */
  int32_t window;                /* >= 1: largest allowed |key - query| of a sliding layer           */
  int32_t global_every;          /* >= 1: layer i is full-attention when i % global_every == 0       */
  const float* final_ln_g;       /* [H] gain of the final norm                                        */
  const float* final_ln_b;       /* [H] or NULL                                                       */
} crs_encoder_prenorm;

/* crs_encoder_forward / crs_encoder_forward_queries for CRS_ENC_PRENORM descriptors.  CRS_EINVAL, with a message and before any
 * launch: a descriptor without CRS_ENC_PRENORM or without CRS_ENC_ROTARY, a NULL pre or NULL tables / final gain, window < 1,
 * global_every < 1, positions < seq, a misaligned (16 bytes) table, a NULL ln1_g on a layer other than 0, a non-NULL ln1_g or ln1_b on layer 0, both gated flags.  Every
 * OTHER entry point of this file refuses a CRS_ENC_PRENORM descriptor (a relative bias and the pair head do not combine with it). */
int crs_encoder_forward_prenorm(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                const int32_t* lens_dev, int batch, int seq, void* workspace_dev, size_t workspace_bytes,
                                float* out_dev, int normalize, float* hidden_out_dev, void* stream, const crs_encoder_prenorm* pre);

int crs_encoder_forward_queries_prenorm(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                        const int32_t* lens_dev, int batch, int seq, void* workspace_dev, size_t workspace_bytes,
                                        float* out_dev, void* q16_out_dev, int slab_type, void* stream,
                                        const crs_encoder_prenorm* pre);

/* The launches of such a forward (crs_encoder_plan_describe's form; that entry refuses the flag, since it carries no window): the
 * full-attention line is followed by the sliding layers' attention_window_kernel line. */
int crs_encoder_prenorm_plan_describe(const crs_encoder_desc* d, int batch, int seq, int window, char* buf, size_t cap);

/* Test-facing (additive to ABI 3): the sliding-window attention step on its own,
 *   ctx[b, q, h*hd : (h+1)*hd] = softmax over {j : |j - q| <= window, j < len_b} of (Q K^T / sqrt(hd)) V
 * Arguments as crs_attention_f16 (no bias, no route).  Rows q < len are the attention output; a row q >= len is finite: the
 * attention over its allowed real keys, or zeros when it has none (q >= len + window).  CRS_EINVAL as crs_attention_f16, and
 * for window < 1. */
int crs_attention_window_f16(const void* qkv_dev, const int32_t* lens_dev, void* ctx_dev, int batch, int seq, int hidden, int heads,
                             int window, void* stream);
int crs_attention_window_plan_describe(int batch, int seq, int hidden, int heads, int window, char* buf, size_t cap);

/* Test-facing (additive to ABI 3): the row step of a pre-norm layer on its own,
 *   r = ((y[0] + ... + y[nsplit - 1]) + bias) + residual   -> r32_dev fp32 [tokens, hidden]  (the new residual stream)
 *   x = LayerNorm(r) g + b                                  -> x16_dev fp16, and n32_dev fp32 where it is not NULL
 * y_dev / nsplit / bias_dev / residual_dev as crs_layernorm_f32 (residual_dev may be r32_dev: in place); b_dev may be NULL (a
 * norm without bias); n32_dev may be NULL and must not overlap y_dev.  CRS_EINVAL as crs_layernorm_f32.  Its launch line is
 * crs_row_plan_describe's kind 4 (rows = tokens, arg = nsplit). */
int crs_add_layernorm_f32(const float* y_dev, int nsplit, const float* bias_dev, const float* residual_dev, const float* g_dev,
                          const float* b_dev, float eps, int tokens, int hidden, float* r32_dev, void* x16_dev, float* n32_dev,
                          void* stream);

/* Test-facing (additive to ABI 3): the rotation step on its own.  qkv_dev: fp16 [batch * seq, 3 * hidden], rotated in place in
 * its Q and K column blocks (columns [0, 2 * hidden)); table_dev / positions as crs_encoder_rope.  CRS_EINVAL: a NULL or
 * misaligned (16 bytes) pointer, head_dim not 16 / 32 / 64, batch or seq < 1, positions < seq. */
int crs_rope_qk_f16(void* qkv_dev, const float* table_dev, int positions, int batch, int seq, int hidden, int heads, void* stream);

/* Test-facing (additive to ABI 3): the attention step on its own, exactly as the forward launches it,
 *   ctx[b, s, h*hd : (h+1)*hd] = softmax(Q K^T / sqrt(hd) + bias[h][key - query] + padding mask) V       per (batch, head)
 * qkv_dev: fp16 [batch * seq, 3 * hidden] (Q | K | V column blocks), only read; lens_dev: int32 [batch], clamped to [1, seq]; ctx_dev:
 * fp16 [batch * seq, hidden], every row written (a padding query attends the real keys).  rel_bias_dev (may be NULL: no bias):
 * fp32 [heads, 2 * rel_span - 1] as crs_encoder_ext takes it.  The kernel is the one the planner answers (csrc/enc_plan.h:
 * plan_attention) for these sizes and knobs, and the entry decides nothing else, so no kernel starts at a shape the planner would
 * not give it.  route < 0: the process's CRS_ATTN_* knobs; route >= 0: the default knobs with these bits applied -- 1 no
 * whole-sequence kernels, 2 no short kernel, 4 the 16-deep whole-sequence kernel, 8 four query tiles per wave -- so that every
 * form is reachable in one process.  With a bias every route gives the blocked kernel.
 * CRS_EINVAL before any launch: a NULL qkv / lens / ctx, a pointer that is not 16-byte aligned, hidden % heads != 0, head_dim not
 * 16 / 32 / 64, batch outside [1, 65535], seq < 1, route > 15, a bias with seq > 512 or rel_span < seq. */
int crs_attention_f16(const void* qkv_dev, const int32_t* lens_dev, void* ctx_dev, int batch, int seq, int hidden, int heads,
                      const float* rel_bias_dev, int rel_span, int route, void* stream);

/* Test-facing (additive to ABI 3): the fused QKV projection + attention kernel of short sequences on its own, with the plan the
 * forward makes for it.  x16_dev: fp16 [batch * seq, hidden]; w_qkv_dev: fp16 [3 * hidden, hidden]; b_qkv_dev: fp32 [3 * hidden];
 * ctx_dev: fp16 [batch * seq, hidden].  It launches only where the forward may: hidden 128 / 256 / 384 with head_dim 32 / 64 whose
 * LDS image fits (csrc/enc_plan.h: qkv_attn_supported), seq 16 / 32 / 64, batch * seq <= 4096; CRS_EINVAL otherwise, and for the
 * pointer, batch, seq and head_dim conditions of crs_attention_f16. */
int crs_qkv_attn_f16(const void* x16_dev, const void* w_qkv_dev, const float* b_qkv_dev, const int32_t* lens_dev, void* ctx_dev,
                     int batch, int seq, int hidden, int heads, void* stream);

/* The launch crs_attention_f16 would make (route as there; rel_bias != 0: with a bias), as one line of crs_encoder_plan_describe's
 * form; route 16: the launch of crs_qkv_attn_f16.  The grid depends on batch, heads and seq alone: it needs no device.  Returns the
 * length of the text as snprintf does, or a negative error code (CRS_EINVAL where the launching entry would refuse the sizes). */
int crs_attention_plan_describe(int batch, int seq, int hidden, int heads, int rel_bias, int route, char* buf, size_t cap);

/* Test-facing (additive to ABI 3): the encoder's HBM-bound row kernels on their own (csrc/enc_misc.hip, csrc/enc_pair.hip).  Each entry
 * checks its arguments and calls the launcher the forward calls, nothing else.  All of them refuse with CRS_EINVAL before any launch: a
 * NULL required pointer; a pointer that is not 16-byte aligned; hidden outside the multiples of 64 up to 1024; tokens, batch or seq
 * < 1; and what each lists below.
 *
 * crs_embed_ln_f32: x = LayerNorm((word[id] + type[type id]) + pos[t % seq]) per token t < tokens -> x32_dev fp32 [tokens, hidden] and
 * x16_dev fp16 [tokens, hidden].  ids_dev int32 [tokens], clamped to [0, vocab); type_ids_dev int32 [tokens] clamped to [0, type_rows),
 * or NULL: row 0 of type_dev for every token (type_rows is then not read); word_dev fp32 [vocab, hidden]; pos_dev fp32 [>= seq, hidden]
 * or NULL: no position row (rotary models); type_dev fp32 [type_rows, hidden]; g_dev / b_dev: the LayerNorm's gain and bias.
 * Also CRS_EINVAL: vocab < 1, type ids with type_rows < 1. */
int crs_embed_ln_f32(const int32_t* ids_dev, const int32_t* type_ids_dev, int type_rows, const float* word_dev, const float* pos_dev,
                     const float* type_dev, const float* g_dev, const float* b_dev, float eps, int tokens, int seq, int hidden,
                     int vocab, float* x32_dev, void* x16_dev, void* stream);

/* crs_layernorm_f32: x = LayerNorm(((y[0] + y[1] + ... + y[nsplit - 1]) + bias) + residual), summed in that order, -> x32_dev, x16_dev as
 * above.  y_dev fp32 [nsplit, tokens, hidden] (the split-K slabs of a GEMM); bias_dev fp32 [hidden] or NULL; residual_dev fp32
 * [tokens, hidden] or NULL, and it may be x32_dev (in place, as the forward runs it).  Also CRS_EINVAL: an nsplit outside 1, 2, 3, 4, 6,
 * 8, 16 (csrc/enc_forms.h: ln_slabs_ok). */
int crs_layernorm_f32(const float* y_dev, int nsplit, const float* bias_dev, const float* residual_dev, const float* g_dev,
                      const float* b_dev, float eps, int tokens, int hidden, float* x32_dev, void* x16_dev, void* stream);

/* crs_pool_f32: the forward's tail.  x32_dev fp32 [batch, seq, hidden]; lens_dev int32 [batch], clamped to [0, seq]; pooling CRS_POOL_MEAN
 * (the mean of tokens [0, len); len 0: the zero vector) or CRS_POOL_CLS (token 0, whatever len); normalize != 0: x / max(||x||, 1e-12).
 * out_dev fp32 [batch, hidden]; out16_dev (may be NULL): the fp16 query block [batch, crs_row_elems(hidden, slab_type)], columns
 * [hidden, row length) written as +0, exactly as crs_encoder_forward_queries_rope asks for it.  Tokens at positions >= max(len, 1) are
 * never read.  Also CRS_EINVAL: a pooling mode other than the two, an unknown slab_type (with or without out16_dev). */
int crs_pool_f32(const float* x32_dev, const int32_t* lens_dev, int batch, int seq, int hidden, int pooling, int normalize,
                 float* out_dev, void* out16_dev, int slab_type, void* stream);

/* crs_pair_head_f32: the head of crs_encoder_score_pairs (below) on hidden states given by the caller.  hidden_dev fp32
 * [batch, seq, hidden], of which only token 0 of every pair is read; w_pool_dev fp32 [hidden, hidden], b_pool_dev [hidden], w_cls_dev
 * [hidden], b_cls_dev [1]; scores_dev fp32 [batch]; pooled_out_dev (may be NULL) fp32 [batch, hidden].  Also CRS_EINVAL: activation
 * outside {0, 1}. */
int crs_pair_head_f32(const float* hidden_dev, int batch, int seq, int hidden, const float* w_pool_dev, const float* b_pool_dev,
                      const float* w_cls_dev, const float* b_cls_dev, int activation, float* scores_dev, float* pooled_out_dev,
                      void* stream);

/* The launch one of the four entries above makes, as one line of crs_encoder_plan_describe's form, built from the expressions the
 * forward's plan is built from.  kind 0: crs_embed_ln_f32, rows = tokens, arg != 0: with type ids; 1: crs_layernorm_f32, rows = tokens,
 * arg = nsplit; 2: crs_pool_f32, rows = batch; 3: crs_pair_head_f32, rows = batch (arg is not read by kinds 2 and 3); 4:
 * crs_add_layernorm_f32, rows = tokens, arg = nsplit.  It needs no
 * device.  Returns the length of the text as snprintf does, or a negative error code (CRS_EINVAL for an unknown kind and where the
 * launching entry would refuse the sizes). */
int crs_row_plan_describe(int kind, int rows, int hidden, int arg, char* buf, size_t cap);

/* Sentence-pair scoring (cross-encoder re-ranking): BertForSequenceClassification with one label.  The rows of ids_dev hold
 * "[CLS] a [SEP] b [SEP]" (tokenised and truncated on the host), type_ids_dev int32 [batch, seq] names the token-type row of every
 * token (0 for "[CLS] a [SEP]", 1 for "b [SEP]", anything for padding; values outside [0, type_rows) are clamped, as token ids
 * are); NULL means all 0 and launches exactly the kernels of crs_encoder_forward.  The layer stack is that of
 * crs_encoder_forward (the descriptor's pooling field is not used; CRS_ENC_SMALL_LDS is honoured); then, per pair and in fp32,
 *   pooled = tanh(w_pool h + b_pool)      h: final hidden state of token 0; w_pool fp32 [H, H] row-major (out, in), b_pool [H]
 *   score  = w_cls . pooled + b_cls[0]    w_cls fp32 [H]; activation 1: score = 1 / (1 + exp(-score))
 * scores_dev fp32 [batch].  pooled_out_dev (may be NULL): fp32 [batch, H]; hidden_out_dev (may be NULL): fp32 [batch, seq, H],
 * both for parity tests.  The workspace is the one crs_encoder_workspace_bytes(d, batch, seq) sizes: the head keeps its operands
 * in LDS and needs no device scratch.  A pair's score does not depend on which other pairs share the call's head launch.
 * CRS_EINVAL, with a message and before any launch: a NULL head or a NULL pointer inside it, type_rows < 1, activation outside
 * {0, 1}, batch < 1, seq > max_pos. */
typedef struct crs_encoder_head {
  const float* w_pool; const float* b_pool;   /* bert.pooler.dense */
  const float* w_cls;  const float* b_cls;    /* classifier, num_labels == 1 */
  int32_t type_rows;                          /* rows of weights->type_emb */
  int32_t activation;                         /* 0 identity (logit), 1 sigmoid */
} crs_encoder_head;

int crs_encoder_score_pairs(const crs_encoder_desc* d, const crs_encoder_weights* w, const crs_encoder_head* head,
                            const int32_t* ids_dev, const int32_t* type_ids_dev /* may be NULL = all 0 */,
                            const int32_t* lens_dev, int batch, int seq, void* workspace_dev, size_t workspace_bytes,
                            float* scores_dev, float* pooled_out_dev /* may be NULL */, float* hidden_out_dev /* may be NULL */,
                            void* stream);

/* Which kernels a forward of this shape launches on the current device: one line per launch of the embedding step, ONE layer and
 * the tail, in launch order -- "<kernel><template arguments> grid=XxYxZ wg=Nx1x1 lds=BYTES\n", the grid in workgroups, the dynamic
 * LDS in bytes.  rel_bias != 0: with a relative-position bias (crs_encoder_ext); pair: 0 the pooling tail, 1 crs_encoder_score_pairs
 * with type ids, 2 without.  d->flags counts (CRS_ENC_SMALL_LDS).  Writes at most cap bytes, the terminating 0 included, and returns
 * the length of the whole text (as snprintf does: >= cap means it was cut), or a negative error code.  It launches nothing. */
int crs_encoder_plan_describe(const crs_encoder_desc* d, int batch, int seq, int rel_bias, int pair, char* buf, size_t cap);

/* Building block exported for parity tests and for users with their own layer stack:
 *   C[M, N] = epilogue(A[M, K] (fp16) x W[N, K]^T (fp16) + bias[N])
 *   mode 0: fp16 out;  mode 1: erf-GELU, fp16 out;  mode 2: + residual fp32 [M, N], fp32 out.
 *   (crs_gemm_f16_routed only) mode 4, the gated epilogue: W has n rows in the interleaved gate / up layout of CRS_ENC_GATED_SILU
 *   and the output is fp16 [M, n / 2]:  out[m, j] = fp16(silu(acc[m, g] + bias[g]) * (acc[m, g + 16] + bias[g + 16])),
 *   g = 32 (j / 16) + j % 16, silu(x) = x / (1 + exp(-x)) in fp32, one rounding; bias fp32 [n] or NULL; n even and n / 2 a
 *   multiple of 32 (CRS_EINVAL otherwise).  Routes 0 (the phase-scheduled 256 x 256 kernel where plan_gemm takes it for
 *   modes 0 / 1, else the tiled 128 x 128 kernel; never the 256-row or row-streaming kernels) and 1 (the panel kernel).
 *   (crs_gemm_f16_routed only) mode 5: mode 4 with the erf GELU in place of SiLU on the activated half (CRS_ENC_GATED_GELU):
 *   out[m, j] = fp16(gelu(acc[m, g] + bias[g]) * (acc[m, g + 16] + bias[g + 16])); same layout, shapes, routes and kernels.
 * Any n > 0: every kernel family makes its 16-byte epilogue accesses only where n keeps the rows 16-byte aligned (a multiple of 8
 * for fp16 outputs, of 4 for fp32 ones) and goes element by element otherwise.  K a multiple of 64; all pointers 16-byte aligned
 * (CRS_EINVAL otherwise).  This is crs_gemm_f16_routed with route 0 and flags 0. */
int crs_gemm_f16(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev,
                 void* out_dev, int m, int n, int k, int mode, void* stream);

/* Test-facing (additive to ABI 3): the same launch with the planner function named by the caller, so that every GEMM kernel family
 * can be run on its own.  route 0: plan_gemm (modes 0..2: the phase-scheduled 256 x 256 kernel, the 256-row pipelined kernel, the
 * row-streaming kernels or the tiled 128 x 128 kernel, by the sizes, the CU count and the CRS_* knobs); route 1: plan_gemm_panel, the
 * panel kernel, modes 0 / 1 / 3, K a multiple of 128; route 2: the split-K form of the 256 x 256 kernel, mode 3 only, CRS_EINVAL for
 * a shape that form does not take (csrc/enc_plan.cpp: gemm8_splitk).  Modes 4 and 5 (above): routes 0 and 1.  flags & 1: the small-LDS forms (CRS_ENC_SMALL_LDS).
 * mode 3 takes no bias (bias_dev must be NULL) and writes the raw fp32 partial products as out_dev[slabs][m][n]; slab z of the
 * panel kernel holds the contraction over columns [z * K / slabs, (z + 1) * K / slabs) of K, and so does slab z of the 256 x 256
 * kernel; crs_gemm_plan_describe answers the slab count.  The entry only chooses which planner function makes the plan; the
 * launchers decide nothing. */
int crs_gemm_f16_routed(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev, void* out_dev,
                        int m, int n, int k, int mode, int route, int flags, void* stream);

/* The launch crs_gemm_f16_routed would make on the current device (its CU count; the knobs), as one line of
 * crs_encoder_plan_describe's form; *slabs (may be NULL): the fp32 slabs a mode-3 launch writes, else 1.  Returns the length of the
 * text as snprintf does, or a negative error code (CRS_EINVAL where crs_gemm_f16_routed would refuse).  It launches nothing. */
int crs_gemm_plan_describe(int m, int n, int k, int mode, int route, int flags, int* slabs, char* buf, size_t cap);

/* Test-facing (additive to ABI 3): the out-projection / FFN-down step of a layer exactly as the forward runs it,
 *   x = LayerNorm(a[tokens, k] (fp16) x w[hidden, k]^T (fp16) + bias + x32) -> x32_inout (fp32, in place), x16_out (fp16),
 * on the route the planner picks (csrc/enc_plan.cpp: plan_proj_ln): with big_ln != 0 and hidden 384, k a multiple of 64 from 192 on,
 * the fused projection + LayerNorm kernel; else split-K panel slabs + LayerNorm, split-K slabs of the 256 x 256 kernel +
 * LayerNorm, or the mode-2 GEMM of crs_gemm_f16 + LayerNorm.  (The forward passes big_ln = tokens > 4096, unless CRS_ENC_BIGLN=0.)
 * y32_ws_dev: slabs * tokens * hidden floats of scratch, slabs as crs_proj_ln_plan_describe answers (1 for the fused kernel, which
 * does not touch it).  g / b: the LayerNorm's gain and bias; flags & 1: CRS_ENC_SMALL_LDS.  hidden a multiple of 64 up to 1024, k a
 * multiple of 64, no NULL pointer, all pointers 16-byte aligned (CRS_EINVAL otherwise). */
int crs_proj_ln_f16(const void* a_dev, const void* w_dev, const float* bias_dev, const float* g_dev, const float* b_dev, float eps,
                    int tokens, int hidden, int k, int flags, int big_ln, float* y32_ws_dev, float* x32_inout_dev, void* x16_out_dev,
                    void* stream);

/* The launches of crs_proj_ln_f16 for these sizes on the current device, one line each (crs_encoder_plan_describe's form), and
 * *slabs (may be NULL).  Returns the length of the text, or a negative error code.  It launches nothing. */
int crs_proj_ln_plan_describe(int tokens, int hidden, int k, int flags, int big_ln, int* slabs, char* buf, size_t cap);

/* ---- learned sparse retrieval (SPLADE): the masked-language-model head with the max-pool in its epilogue (additive to ABI 3;
 * csrc/mlm_pool.hip).  For every text b of a batch and every vocabulary id v,
 *     t_i       = LayerNorm(GELU(W_t h_i + b_t))              i < lens[b]; BertForMaskedLM's cls.predictions.transform
 *     out[b, v] = log1p(max(0, max_i (t_i . Wd_v + bias_v)))  the decoder and cls.predictions.bias
 *   hidden_dev  fp32 [batch, seq, hidden]  final hidden states as crs_encoder_forward leaves them in hidden_out_dev, 16-byte aligned.
 *                                          Positions at or past lens[b] are padding: they are NEVER read, so they may hold anything
 *   lens_dev    int32 [batch]              real tokens per text, clamped to [0, seq] (0: an all-zero row)
 *   out_dev     fp32 [batch, vp]           vp >= vocab; columns [vocab, vp) are not written
 * Numerics: h rounded to fp16 on load, W_t fp16, fp32 accumulation (v_mfma_f32_16x16x32_f16), bias, erf-GELU and LayerNorm in fp32,
 * t rounded to fp16 once; the vocabulary projection is fp16 x fp16 with fp32 accumulation in ascending k, the bias added in fp32;
 * the maximum is exact (an integer maximum over the bit patterns of the non-negative candidates, so it does not depend on the
 * order in which tiles finish) and log1p is evaluated in fp64 and rounded once.  The [tokens, vocab] logits never exist in
 * memory.  A text's row is a pure function of its own real tokens, bit for bit, whatever else shares the call and wherever it
 * sits in the batch.  Rows of the decoder at or past vocab are never read.
 * Workspace: crs_mlm_workspace_bytes() bytes, 256-byte aligned; after the call it begins with t as fp16 [tokens_padded, hidden]
 * (zeros at padding positions), which parity tests read.  crs_mlm_pool_plan() gives the geometry of the launches for these sizes
 * on any host (it touches no device).
 * CRS_EINVAL, with a message and before any launch: a NULL pointer (in the head too), batch < 1, seq < 1, seq > head->max_pos,
 * vocab < 1 or > 2^20, vp < vocab, batch * seq > 2^22, hidden not one of 64, 128, 256, 384, 512, 768, 1024, a pointer that is
 * not 16-byte aligned.  No host synchronisation. */
typedef struct crs_mlm_head {
  int32_t hidden;
  int32_t vocab;
  int32_t max_pos;             /* of the encoder in front: the longest seq */
  float ln_eps;
  const void* transform_w16;   /* fp16 [hidden, hidden] row-major (out, in): cls.predictions.transform.dense.weight */
  const float* transform_bias; /* [hidden] */
  const float* ln_gamma;       /* cls.predictions.transform.LayerNorm */
  const float* ln_beta;
  const void* decoder_w16;     /* fp16 [vocab, hidden]: cls.predictions.decoder.weight (or a fp16 copy of the word embeddings) */
  const float* decoder_bias;   /* fp32 [vocab] */
} crs_mlm_head;

typedef struct crs_mlm_plan {
  int32_t tile_m, tile_n, tile_k;            /* the vocabulary projection's tile: token rows, vocabulary columns, k per step */
  int32_t tokens, tokens_padded;             /* batch * seq, and that rounded up to whole row tiles */
  int32_t grid_m, grid_n;                    /* row tiles and column tiles; the projection launches grid_m * grid_n workgroups */
  int32_t pool_grid, pool_threads, pool_lds_bytes;
  int32_t xform_grid, xform_threads, xform_lds_bytes;   /* the transform: one workgroup per 32 token rows */
  int32_t ew_grid_x, ew_threads;             /* zeroing before and log1p after: grid (ew_grid_x, batch) */
  size_t t16_bytes, workspace_bytes;
} crs_mlm_plan;

int crs_mlm_pool_plan(int batch, int seq, int hidden, int vocab, crs_mlm_plan* plan);
int crs_mlm_workspace_bytes(int batch, int seq, int hidden, int vocab, size_t* bytes);
int crs_mlm_sparse_pool(const float* hidden_dev, const int32_t* lens_dev, int batch, int seq, const crs_mlm_head* head,
                        void* workspace_dev, size_t workspace_bytes, float* out_dev, int vp, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CRS_ENCODER_H */
