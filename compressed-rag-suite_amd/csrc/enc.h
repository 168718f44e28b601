// Internal declarations of the encoder translation units (enc_*.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/crs_encoder.h"
#include "enc_plan.h"

namespace crs {

// Workgroup ids go round-robin over the 8 XCDs (id % 8), each with its own L2.  xcd_chunked_id turns the hardware id into
// a work index such that every XCD walks ONE contiguous range of indices (in id order): tiles that share an operand
// panel are neighbours in index space, so they meet in the same L2 instead of being fetched by eight of them.
__device__ __forceinline__ int xcd_chunked_id(int id, int total) {
  const int x = id & 7, q = total >> 3, r = total & 7;
  return x * q + (x < r ? x : r) + (id >> 3);
}

// Launchers: each takes the plan (or the step of it) that enc_plan.cpp made, switches on its fields to pick the
// instantiation, and launches with the plan's grid, workgroup size and dynamic LDS.  They decide nothing.  Return 0, a hipError_t,
// or -1 for a plan of another file's family.

// enc_gemm.hip: C = epilogue(A[M,K] W[N,K]^T + bias) on the plan's family (GemmPlan: modes and families).  residual: mode 2 only;
// mode 3 takes no bias and writes out as fp32 [slabs][M][N], summed by layernorm_launch; mode 4 (gemm8, tiled and panel families only:
// the planner routes it nowhere else) writes fp16 [M, N / 2].
int gemm_launch(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, const float* residual, void* out,
                hipStream_t stream);
// the families of the other files, reached through gemm_launch: enc_gemm8.hip (256 x 256 x 64 tiles, eight-barrier phase
// schedule, whole or split K), enc_gemm_big.hip (256-row tiles for large M), enc_gemm_stream.hip (row-streaming, W resident in VGPRs)
int gemm8_launch(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, const float* residual, void* out,
                 hipStream_t stream);
int gemm_big_launch(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, const float* residual, void* out,
                    hipStream_t stream);
int gemm_stream_launch(const GemmPlan& p, const _Float16* a, const _Float16* w, const float* bias, const float* residual, void* out,
                       hipStream_t stream);

// enc_qkvattn.hip: QKV projection + attention of short sequences (16 / 32 / 64 tokens) in one kernel (AttnForm::Fused)
int qkv_attn_launch(const AttnPlan& p, const _Float16* x16, const _Float16* w_qkv, const float* b_qkv, const int* lens, _Float16* ctx,
                    int tokens, int seq, int hidden, hipStream_t stream);

// enc_rowln.hip, pipelined projection + LayerNorm for large token counts (index build), hidden = 384 (ProjLnPlan::rowln2)
int gemm_rowln2_launch(const ProjLnPlan& p, const _Float16* a, const _Float16* w, const float* bias, const float* residual,
                       const float* g, const float* b, float eps, int m, int k, float* x32, _Float16* x16, hipStream_t stream);

// enc_attn.hip: ctx[T, H] = softmax(QK^T / sqrt(hd) + padding mask) V per (batch, head), every form but Fused;
// qkv is [T, 3H] fp16 (Q | K | V column blocks), lens[b] real tokens per row (right padding).
// rel_bias (Blocked with bias): bias[h][key - query] added to every score before the softmax, fp32 [heads, 2 span - 1], entry
// (key - query) + span - 1; span >= seq, seq <= 512 (-1 otherwise).  <= 21 KB of static LDS.
int attention_launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int batch, int seq, int hidden, int heads,
                     const float* rel_bias, int span, hipStream_t stream);

// AttnForm::Window (plan_attention_window): the blocked kernel restricted to the keys with |key - query| <= p.window; a query without
// any allowed key (padding at q >= len + window) gets a zero row.  No bias.  -1 for another form or a head_dim other than 16 / 32 / 64.
int attention_window_launch(const AttnPlan& p, const _Float16* qkv, const int* lens, _Float16* ctx, int seq, int hidden, hipStream_t stream);

// enc_rope.hip: rotates the Q and K column blocks of qkv [tokens, 3 hidden] fp16 in place against table fp32 [positions, hd]
// (cos half | sin half, include/crs_encoder.h: CRS_ENC_ROTARY); d: EncPlan::rope; the caller checked positions >= seq.  No LDS.
int rope_qk_launch(const Dims& d, int hd, _Float16* qkv, const float* table, int tokens, int seq, int hidden, hipStream_t stream);

// enc_misc.hip
// type_ids (may be null: row 0 of type_tab for every token): int32 [tokens], clamped to [0, type_rows); an all-zero block
// gives the bits of the null form.  pos may be null: no position row is added (rotary models)
int embed_ln_launch(const int* ids, const int* type_ids, const float* word, const float* pos, const float* type_tab,
                    int type_rows, const float* g, const float* b, float eps, int tokens, int seq, int hidden, int vocab,
                    float* x32, _Float16* x16, hipStream_t stream);
// LayerNorm( sum_{s<nsplit} y[s] + bias + residual ): bias / residual may be null (already folded in)
int layernorm_launch(const float* y, int nsplit, const float* bias, const float* residual, const float* g,
                     const float* b, float eps, int tokens, int hidden, float* x32, _Float16* x16,
                     hipStream_t stream);
int pool_launch(const float* x32, const int* lens, int batch, int seq, int hidden, int pooling, int normalize,
                float* out, _Float16* out16, int pdim16, hipStream_t stream);
// enc_addln.hip
// The row step of a pre-norm layer: r = (sum_{s<nsplit} y[s] + bias) + residual -> r32 (the new residual stream; residual may be
// r32, in place), x16 = fp16(LayerNorm(r) g + b), and n32 (may be null; the final norm) = the same normalised row in fp32.
// bias, residual and b may be null (b: a norm without bias).  -1 for a slab count outside CRS_LN_SLABS.
int add_layernorm_launch(const float* y, int nsplit, const float* bias, const float* residual, const float* g, const float* b,
                         float eps, int tokens, int hidden, float* r32, _Float16* x16, float* n32, hipStream_t stream);

// enc_pair.hip
// scores[b] = w_cls . tanh(w_pool hidden32[b, 0, :] + b_pool) + b_cls[0] (activation 1: then 1 / (1 + exp(-score))), all fp32;
// pooled_out (may be null): the tanh vectors [batch, hidden].  -1: hidden not a multiple of 64 up to 1024
int pair_head_launch(const float* hidden32, int batch, int seq, int hidden, const float* w_pool, const float* b_pool,
                     const float* w_cls, const float* b_cls, int activation, float* scores, float* pooled_out,
                     hipStream_t stream);

// mlm_pool.hip
// out[b, v] = log1p(max(0, max_{i < lens[b]} (t_i . Wd_v + bias_v))), t = LayerNorm(GELU(W_t h + b_t)) left as fp16 in t16
// [p.tokens_padded, hidden] (the workspace); four launches walking the plan (mlm_plan.h).  -1: a hidden the transform has no
// instantiation for
int mlm_sparse_pool_launch(const crs_mlm_plan& p, const float* hidden32, const int* lens, int batch, int seq, const crs_mlm_head& head,
                           _Float16* t16, float* out, int vp, hipStream_t stream);

}  // namespace crs
