// enc_capi.hip -- extern "C" surface of include/crs_encoder.h: the layer loop of the encoder.
//
// Per layer (7 launches on one stream, no host sync):
//   qkv  = x16 Wqkv^T + b                     gemm mode 0      [T, 3H] fp16
//   ctx  = attention(qkv, lens)               enc_attn.hip     [T, H]  fp16
//   y32  = ctx Wo^T + b + x32                 gemm mode 2      fp32
//   x    = LayerNorm(y32)                     -> x32 (fp32 residual stream), x16 (next GEMM input)
//   ffn  = gelu(x16 Wup^T + b)                gemm mode 1      [T, F] fp16
//   y32  = ffn Wdown^T + b + x32              gemm mode 2
//   x    = LayerNorm(y32)
// Rotary models (CRS_ENC_ROTARY): one rope_qk launch on qkv between the first two steps; gated ones (CRS_ENC_GATED_SILU):
//   ffn  = silu(x16 Wgate^T + b) * (x16 Wup^T + b)   gemm mode 4 over the interleaved [2F, H] weight      [T, F] fp16
// Pre-norm models (CRS_ENC_PRENORM, with CRS_ENC_ROTARY and CRS_ENC_GATED_GELU: ModernBERT) take the second arm of the layer loop:
//   qkv  = x16 Wqkv^T                          x16 = LN_attn(r) from the previous add_layernorm (layer 0: the embedding norm's output)
//   rope with the layer type's table; ctx = attention (full layers: plan_attention's kernel) or attention_window (the others)
//   r, x16 = add_layernorm(ctx Wo^T, r)        r <- r + product, x16 <- fp16(LN_mlp(r))             enc_addln.hip
//   ffn  = gelu(x16 Wa^T) * (x16 Wb^T)         gemm mode 5 over the interleaved [2F, H] weight
//   r, x16 = add_layernorm(ffn Wdown^T, r)     x16 <- the NEXT layer's LN_attn(r); after the last layer the final norm, kept in fp32 too
// then pooling + L2 normalise -- or, for crs_encoder_score_pairs, the pair head (enc_pair.hip) on the [CLS] rows; its embedding
// step takes a token-type row per token (embed_ln_launch with type_ids).  The launch function allocates nothing and never synchronises, so
// a caller may capture it into a hipGraph for the launch-bound single-query case.
// Which kernel each of these steps runs on is the plan's business (enc_plan.cpp: make_enc_plan, once per call); this file walks it.
#include "../../include/crs_encoder.h"
#include "../../include/crs_hip.h"

#include <stdio.h>

#include <initializer_list>

#include "enc.h"
#include "mlm_plan.h"

namespace crs {
int set_error(int code, const char* msg);  // capi.hip
int device_cus();                          // capi.hip: per device, 0 without one
}

namespace {

// the knobs are read once, at the first encoder plan of the process
const crs::EncKnobs& knobs() {
  static const crs::EncKnobs kn = crs::enc_knobs_from_env();
  return kn;
}

crs::EncPlan plan_for(const crs_encoder_desc* d, int batch, int seq, int rel_bias, int pair, int cus, int window = 0) {
  return crs::make_enc_plan(d->hidden, d->heads, d->ffn, d->flags, batch, seq, rel_bias, pair, cus, knobs(), window);
}

int check_desc(const crs_encoder_desc* d) {
  if (!d) return crs::set_error(CRS_EINVAL, "null descriptor");
  if (d->hidden <= 0 || d->hidden > 1024 || d->hidden % 64) return crs::set_error(CRS_EINVAL, "hidden must be a multiple of 64, <= 1024");
  if (d->heads <= 0 || d->hidden % d->heads) return crs::set_error(CRS_EINVAL, "hidden must divide by heads");
  const int hd = d->hidden / d->heads;
  if (hd != 16 && hd != 32 && hd != 64) return crs::set_error(CRS_EINVAL, "head_dim must be 16, 32 or 64");
  if (d->ffn <= 0 || d->ffn % 64) return crs::set_error(CRS_EINVAL, "ffn must be a multiple of 64");
  if (d->layers <= 0 || d->vocab_size <= 0 || d->max_pos <= 0) return crs::set_error(CRS_EINVAL, "bad layers/vocab/max_pos");
  if (d->pooling != CRS_POOL_MEAN && d->pooling != CRS_POOL_CLS) return crs::set_error(CRS_EINVAL, "bad pooling mode");
  if ((d->flags & CRS_ENC_GATED_SILU) && (d->flags & CRS_ENC_GATED_GELU)) return crs::set_error(CRS_EINVAL, "CRS_ENC_GATED_SILU and CRS_ENC_GATED_GELU exclude each other");
  // (ffn % 64 above is what CRS_ENC_GATED_SILU needs: whole [16 gate | 16 up] blocks in every 128-row tile of the 2 ffn rows)
  return CRS_OK;
}

// modes 4, 5: n rows of interleaved gate / up weights, n / 2 output columns in whole blocks of 16 pairs
bool gated_n_ok(int n) { return n % 2 == 0 && (n / 2) % 32 == 0; }

// what crs_encoder_score_pairs adds to the forward: per-token type ids at the embedding step (null: row 0, the kernels of the
// plain forward) and the pair head in place of pooling
struct PairTail {
  const crs_encoder_head* head;
  const int32_t* type_ids;
  float* scores;
  float* pooled_out;
};

#define CRS_TRY(expr, what)                                                             \
  do {                                                                                  \
    const int e_ = (expr);                                                              \
    if (e_ == -1) return crs::set_error(CRS_EINVAL, what ": unsupported shape");        \
    if (e_) { char m_[160]; snprintf(m_, sizeof m_, what ": %s", hipGetErrorString((hipError_t)e_)); return crs::set_error(CRS_EHIP, m_); } \
  } while (0)

// route: which planner function makes the GemmPlan (the launchers still decide nothing).  *why: the message of a refusal
crs::GemmPlan routed_plan(int m, int n, int k, int mode, int route, int flags, int cus, const char** why) {
  crs::GemmPlan p;
  const int small = flags & 1;
  *why = "bad gemm arguments";
  if (m <= 0 || n <= 0 || k <= 0) return p;
  *why = "gemm K must be a multiple of 64";
  if (k % 64) return p;
  if ((mode == 4 || mode == 5) && route <= 1) {
    *why = mode == 4 ? "gemm mode 4 (gated): n must be even and n / 2 a multiple of 32"
                     : "gemm mode 5 (gated): n must be even and n / 2 a multiple of 32";
    if (!gated_n_ok(n)) return p;
    *why = "panel gemm: modes 0, 1, 3, 4 and 5, K a multiple of 128";
    return route == 0 ? crs::plan_gemm(m, n, k, mode, small, cus, knobs()) : crs::plan_gemm_panel(m, n, k, mode, small, knobs());
  }
  if (route == 0) {
    *why = "bad gemm mode / missing residual";
    if (mode < 0 || mode > 2) return p;
    return crs::plan_gemm(m, n, k, mode, small, cus, knobs());
  }
  if (route == 1) {
    *why = "panel gemm: modes 0, 1 and 3, K a multiple of 128";
    if (mode != 0 && mode != 1 && mode != 3) return p;
    return crs::plan_gemm_panel(m, n, k, mode, small, knobs());   // family None where K has no chunk
  }
  if (route == 2) {
    *why = "gemm8 split-K: mode 3, and a shape gemm8_splitk takes (m >= 2048 in whole 256-row tiles, n in whole 256-column blocks, < 128 tiles)";
    const int s8 = mode == 3 ? crs::gemm8_splitk(m, n, k, knobs()) : 0;
    if (!s8) return p;
    return crs::plan_gemm8(m, n, k, 3, s8, cus, knobs());
  }
  *why = "bad gemm route";
  return p;
}

// out-projection / FFN-down + LayerNorm into x32 / x16: one fused launch, or the GEMM (fp32 slabs in y32, or bias + residual
// folded in) and the LayerNorm that sums the slabs.  The residual is x32, updated in place.  Returns as the launchers do.
int proj_ln_run(const crs::ProjLnPlan& s, const _Float16* a, const void* wt, const float* bias, const float* g, const float* b,
                float eps, int T, int H, int k, float* x32, float* y32, _Float16* x16, hipStream_t st) {
  if (s.rowln2) return crs::gemm_rowln2_launch(s, a, (const _Float16*)wt, bias, x32, g, b, eps, T, k, x32, x16, st);
  const bool folded = s.gemm.mode == 2;
  const int e = crs::gemm_launch(s.gemm, a, (const _Float16*)wt, folded ? bias : nullptr, folded ? x32 : nullptr, y32, st);
  if (e) return e;
  return crs::layernorm_launch(y32, s.gemm.slabs, folded ? nullptr : bias, folded ? nullptr : x32, g, b, eps, T, H, x32, x16, st);
}

int check_proj_ln(int tokens, int hidden, int k) {
  if (tokens <= 0 || hidden <= 0 || hidden > 1024 || hidden % 64) return crs::set_error(CRS_EINVAL, "proj_ln: tokens > 0, hidden a multiple of 64, <= 1024");
  if (k <= 0 || k % 64) return crs::set_error(CRS_EINVAL, "proj_ln: K must be a multiple of 64");
  return CRS_OK;
}

// the attention step on its own (crs_attention_f16, crs_qkv_attn_f16): what both refuse by the sizes, and the knobs of a route
const char* attn_sizes_refusal(int batch, int seq, int hidden, int heads) {
  if (heads < 1 || hidden < 1 || hidden % heads) return "attention: hidden must divide by heads";
  const int hd = hidden / heads;
  if (hd != 16 && hd != 32 && hd != 64) return "attention: head_dim must be 16, 32 or 64";
  if (batch < 1 || batch > 65535) return "attention: batch must be in [1, 65535]";
  if (seq < 1) return "attention: seq must be >= 1";
  return nullptr;
}

const char* attn_bias_refusal(int seq, int rel_span) {
  return (seq > crs::forms::kAttnMaxBiasSeq || rel_span < seq) ? "attention: a relative bias needs seq <= 512 and rel_span >= seq" : nullptr;
}

crs::EncKnobs attn_knobs(int route) { return route < 0 ? knobs() : crs::attn_route_knobs(route); }

// the row kernels on their own (crs_embed_ln_f32, crs_layernorm_f32, crs_pool_f32, crs_pair_head_f32): the hidden sizes they are
// written for, and the alignment of every pointer given (a null optional pointer passes)
const char* row_hidden_refusal(int hidden) {
  return (hidden <= 0 || hidden > 1024 || hidden % 64) ? "hidden must be a multiple of 64, <= 1024" : nullptr;
}

bool row_misaligned(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) != 0;
}

}  // namespace

extern "C" {

int crs_encoder_workspace_bytes(const crs_encoder_desc* d, int batch, int seq, size_t* bytes) {
  const int rc = check_desc(d);
  if (rc) return rc;
  if (!bytes || batch <= 0 || seq <= 0 || seq > d->max_pos) return crs::set_error(CRS_EINVAL, "bad batch/seq (seq <= max_pos)");
  *bytes = plan_for(d, batch, seq, 0, 0, 1).total;   // the layout depends on no CU count: a pure host call
  return CRS_OK;
}

int crs_gemm_f16_routed(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev, void* out_dev,
                        int m, int n, int k, int mode, int route, int flags, void* stream) {
  if (!a_dev || !w_dev || !out_dev) return crs::set_error(CRS_EINVAL, "bad gemm arguments");
  if (mode == 2 && !residual_dev) return crs::set_error(CRS_EINVAL, "bad gemm mode / missing residual");
  if (mode == 3 && bias_dev) return crs::set_error(CRS_EINVAL, "gemm mode 3 takes no bias (the LayerNorm that sums the slabs adds it)");
  if (((uintptr_t)a_dev | (uintptr_t)w_dev | (uintptr_t)out_dev | (uintptr_t)bias_dev | (uintptr_t)residual_dev) & 15)
    return crs::set_error(CRS_EINVAL, "gemm pointers must be 16-byte aligned");
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "gemm: no device");
  const char* why = "";
  const crs::GemmPlan p = routed_plan(m, n, k, mode, route, flags, cus, &why);
  if (p.family == crs::GemmFamily::None) return crs::set_error(CRS_EINVAL, why);
  CRS_TRY(crs::gemm_launch(p, (const _Float16*)a_dev, (const _Float16*)w_dev, bias_dev, mode == 2 ? residual_dev : nullptr, out_dev,
                           (hipStream_t)stream), "gemm");
  return CRS_OK;
}

int crs_gemm_f16(const void* a_dev, const void* w_dev, const float* bias_dev, const float* residual_dev,
                 void* out_dev, int m, int n, int k, int mode, void* stream) {
  if (mode < 0 || mode > 2) return crs::set_error(CRS_EINVAL, "bad gemm mode / missing residual");
  return crs_gemm_f16_routed(a_dev, w_dev, bias_dev, residual_dev, out_dev, m, n, k, mode, 0, 0, stream);
}

int crs_gemm_plan_describe(int m, int n, int k, int mode, int route, int flags, int* slabs, char* buf, size_t cap) {
  if (cap && !buf) return crs::set_error(CRS_EINVAL, "plan describe: null buffer");
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "plan describe: no device");
  const char* why = "";
  const crs::GemmPlan p = routed_plan(m, n, k, mode, route, flags, cus, &why);
  if (p.family == crs::GemmFamily::None) return crs::set_error(CRS_EINVAL, why);
  if (slabs) *slabs = p.slabs;
  return crs::gemm_plan_describe(p, buf, cap);
}

int crs_proj_ln_f16(const void* a_dev, const void* w_dev, const float* bias_dev, const float* g_dev, const float* b_dev, float eps,
                    int tokens, int hidden, int k, int flags, int big_ln, float* y32_ws_dev, float* x32_inout_dev, void* x16_out_dev,
                    void* stream) {
  const int rc = check_proj_ln(tokens, hidden, k);
  if (rc) return rc;
  if (!a_dev || !w_dev || !bias_dev || !g_dev || !b_dev || !y32_ws_dev || !x32_inout_dev || !x16_out_dev) return crs::set_error(CRS_EINVAL, "proj_ln: null pointer");
  if (((uintptr_t)a_dev | (uintptr_t)w_dev | (uintptr_t)bias_dev | (uintptr_t)g_dev | (uintptr_t)b_dev | (uintptr_t)y32_ws_dev |
       (uintptr_t)x32_inout_dev | (uintptr_t)x16_out_dev) & 15)
    return crs::set_error(CRS_EINVAL, "proj_ln pointers must be 16-byte aligned");
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "proj_ln: no device");
  const crs::ProjLnPlan s = crs::plan_proj_ln(tokens, hidden, k, big_ln != 0, flags & 1, cus, knobs());
  CRS_TRY(proj_ln_run(s, (const _Float16*)a_dev, w_dev, bias_dev, g_dev, b_dev, eps, tokens, hidden, k, x32_inout_dev, y32_ws_dev,
                      (_Float16*)x16_out_dev, (hipStream_t)stream), "projection + layernorm");
  return CRS_OK;
}

int crs_proj_ln_plan_describe(int tokens, int hidden, int k, int flags, int big_ln, int* slabs, char* buf, size_t cap) {
  const int rc = check_proj_ln(tokens, hidden, k);
  if (rc) return rc;
  if (cap && !buf) return crs::set_error(CRS_EINVAL, "plan describe: null buffer");
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "plan describe: no device");
  const crs::ProjLnPlan s = crs::plan_proj_ln(tokens, hidden, k, big_ln != 0, flags & 1, cus, knobs());
  if (slabs) *slabs = s.rowln2 ? 1 : s.gemm.slabs;
  return crs::proj_ln_plan_describe(s, hidden, buf, cap);
}

int crs_encoder_plan_describe(const crs_encoder_desc* d, int batch, int seq, int rel_bias, int pair, char* buf, size_t cap) {
  const int rc = check_desc(d);
  if (rc) return rc;
  if (batch <= 0 || seq <= 0 || seq > d->max_pos || pair < 0 || pair > 2 || (cap && !buf)) return crs::set_error(CRS_EINVAL, "bad batch/seq (seq <= max_pos), pair or buffer");
  if (d->flags & CRS_ENC_PRENORM) return crs::set_error(CRS_EINVAL, "a CRS_ENC_PRENORM descriptor needs crs_encoder_prenorm_plan_describe (it carries the window)");
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "plan describe: no device");
  return crs::enc_plan_describe(plan_for(d, batch, seq, rel_bias != 0, pair, cus), buf, cap);
}

static int encoder_forward(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                           const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                           size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                           _Float16* q16_out_dev, int q16_row_elems, void* stream, const crs_encoder_ext* ext,
                           const PairTail* pair = nullptr, const crs_encoder_rope* rope = nullptr,
                           const crs_encoder_prenorm* pre = nullptr) {
  const int rc = check_desc(d);
  if (rc) return rc;
  const bool rotary = (d->flags & CRS_ENC_ROTARY) != 0;
  const bool prenorm = (d->flags & CRS_ENC_PRENORM) != 0;
  if (prenorm) {
    if (pair || (ext && ext->rel_bias_dev)) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM does not combine with a relative-position bias or the pair head");
    if (!rotary) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM needs CRS_ENC_ROTARY");
    if (!pre || !pre->rope_global_dev || !pre->rope_local_dev) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM needs both rope tables (crs_encoder_forward_prenorm / crs_encoder_forward_queries_prenorm)");
    if (pre->window < 1) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM: window must be >= 1");
    if (pre->global_every < 1) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM: global_every must be >= 1");
    if (!pre->final_ln_g) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM needs the final norm's gain");
    if (pre->positions < seq || (((uintptr_t)pre->rope_global_dev | (uintptr_t)pre->rope_local_dev) & 15)) {
      char m[160];
      snprintf(m, sizeof m, "rope tables: positions %d must be >= seq %d, and the tables 16-byte aligned", pre->positions, seq);
      return crs::set_error(CRS_EINVAL, m);
    }
    if (w && w->layers) {
      // layer 0 has no attention norm: its QKV projection reads the embedding norm's output, and a norm given there would be ignored
      if (w->layers[0].ln1_g || w->layers[0].ln1_b) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM: layer 0 has no attention norm (ln1_g and ln1_b must be NULL)");
      for (int li = 1; li < d->layers; ++li)
        if (!w->layers[li].ln1_g) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM: only layer 0 may have a NULL ln1_g (identity)");
    }
  } else if (pre) {
    return crs::set_error(CRS_EINVAL, "the _prenorm entry points need a CRS_ENC_PRENORM descriptor");
  }
  const float* rope_table = prenorm ? pre->rope_global_dev : rope ? rope->table_dev : nullptr;
  if (rotary && !rope_table) return crs::set_error(CRS_EINVAL, "CRS_ENC_ROTARY needs a rope table (crs_encoder_forward_rope / crs_encoder_forward_queries_rope)");
  if (rotary && ext && ext->rel_bias_dev) return crs::set_error(CRS_EINVAL, "CRS_ENC_ROTARY does not combine with a relative-position bias");
  if (rotary && !prenorm && (rope->positions < seq || ((uintptr_t)rope_table & 15))) {
    char m[160];
    snprintf(m, sizeof m, "rope table: positions %d must be >= seq %d, and the table 16-byte aligned", rope->positions, seq);
    return crs::set_error(CRS_EINVAL, m);
  }
  const float* rel_bias = ext ? ext->rel_bias_dev : nullptr;   // additive relative-position bias (crs_encoder_ext)
  const int rel_span = rel_bias ? ext->rel_span : 0;
  if (!w || !w->layers || !ids_dev || !lens_dev || !workspace_dev || !(pair ? (void*)pair->scores : (void*)out_dev)) return crs::set_error(CRS_EINVAL, "null pointer");
  if (batch <= 0 || seq <= 0 || seq > d->max_pos) return crs::set_error(CRS_EINVAL, "bad batch/seq (seq <= max_pos)");
  if (rel_bias && (rel_span < seq || seq > 512)) {
    char m[160];
    snprintf(m, sizeof m, "relative bias: rel_span %d must be >= seq %d, and seq <= 512", rel_span, seq);
    return crs::set_error(CRS_EINVAL, m);
  }
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "encoder forward: no device");
  // integer arithmetic only: no allocation, no device call, legal inside graph capture
  const crs::EncPlan p = plan_for(d, batch, seq, rel_bias != nullptr, pair ? (pair->type_ids ? 1 : 2) : 0, cus, prenorm ? pre->window : 0);
  if (workspace_bytes < p.total) return crs::set_error(CRS_ENOSPC, "encoder workspace too small");
  hipStream_t st = (hipStream_t)stream;
  char* ws = reinterpret_cast<char*>(workspace_dev);
  float* x32 = reinterpret_cast<float*>(ws + p.x32);
  float* y32 = reinterpret_cast<float*>(ws + p.y32);
  _Float16* x16 = reinterpret_cast<_Float16*>(ws + p.x16);
  _Float16* ctx = reinterpret_cast<_Float16*>(ws + p.ctx);
  _Float16* qkv = reinterpret_cast<_Float16*>(ws + p.qkv_off);
  _Float16* ffn = reinterpret_cast<_Float16*>(ws + p.ffn_off);
  const int T = p.tokens, H = d->hidden, F = d->ffn;

  auto proj_ln = [&](const crs::ProjLnPlan& s, const _Float16* a, const void* wt, const float* bias, const float* g, const float* b, int k) -> int {
    return proj_ln_run(s, a, wt, bias, g, b, d->ln_eps, T, H, k, x32, y32, x16, st);
  };

  CRS_TRY(crs::embed_ln_launch(ids_dev, pair ? pair->type_ids : nullptr, w->word_emb, w->pos_emb, w->type_emb,
                               pair ? pair->head->type_rows : 1, w->emb_ln_g, w->emb_ln_b, d->ln_eps, T, seq, H, d->vocab_size, x32,
                               x16, st), "embed_ln");
  // pre-norm: x32 is the un-normalised residual stream r; a block's GEMM leaves its product in y32 (slabs, or bias + r folded in) and
  // add_layernorm writes r back and the NEXT block's normalised input to x16.  Layer 0's attention reads the embedding norm's x16.
  // The final norm's fp32 rows go to the (then free) QKV buffer: 6 T H bytes hold the 4 T H.
  auto add_ln = [&](const crs::ProjLnPlan& s, const _Float16* a, const void* wt, const float* bias, const float* g, const float* b, float* n32) -> int {
    const bool folded = s.gemm.mode == 2;
    const int e = crs::gemm_launch(s.gemm, a, (const _Float16*)wt, folded ? bias : nullptr, folded ? x32 : nullptr, y32, st);
    if (e) return e;
    return crs::add_layernorm_launch(y32, s.gemm.slabs, folded ? nullptr : bias, folded ? nullptr : x32, g, b, d->ln_eps, T, H, x32, x16, n32, st);
  };
  const float* final32 = x32;   // what pooling and hidden_out read
  for (int li = 0; prenorm && li < d->layers; ++li) {
    const crs_encoder_layer& L = w->layers[li];
    const bool full = li % pre->global_every == 0, last = li + 1 == d->layers;
    CRS_TRY(crs::gemm_launch(p.qkv, x16, (const _Float16*)L.w_qkv, L.b_qkv, nullptr, qkv, st), "qkv gemm");
    CRS_TRY(crs::rope_qk_launch(p.rope, p.attn.hd, qkv, full ? pre->rope_global_dev : pre->rope_local_dev, T, seq, H, st), "rope");
    if (full) CRS_TRY(crs::attention_launch(p.attn, qkv, lens_dev, ctx, batch, seq, H, d->heads, nullptr, 0, st), "attention");
    else CRS_TRY(crs::attention_window_launch(p.win, qkv, lens_dev, ctx, seq, H, st), "windowed attention");
    CRS_TRY(add_ln(p.out, ctx, L.w_o, L.b_o, L.ln2_g, L.ln2_b, nullptr), "out projection + add + mlp norm");
    CRS_TRY(crs::gemm_launch(p.up, x16, (const _Float16*)L.w_up, L.b_up, nullptr, ffn, st), "ffn up gemm");
    float* n32 = last ? reinterpret_cast<float*>(qkv) : nullptr;
    CRS_TRY(add_ln(p.down, ffn, L.w_down, L.b_down, last ? pre->final_ln_g : w->layers[li + 1].ln1_g,
                   last ? pre->final_ln_b : w->layers[li + 1].ln1_b, n32), "ffn down projection + add + next norm");
    if (last) final32 = n32;
  }
  for (int li = 0; !prenorm && li < d->layers; ++li) {
    const crs_encoder_layer& L = w->layers[li];
    if (p.attn.form == crs::AttnForm::Fused) {
      CRS_TRY(crs::qkv_attn_launch(p.attn, x16, (const _Float16*)L.w_qkv, L.b_qkv, lens_dev, ctx, T, seq, H, st), "qkv + attention");
    } else {
      CRS_TRY(crs::gemm_launch(p.qkv, x16, (const _Float16*)L.w_qkv, L.b_qkv, nullptr, qkv, st), "qkv gemm");
      if (p.rotary) CRS_TRY(crs::rope_qk_launch(p.rope, p.attn.hd, qkv, rope_table, T, seq, H, st), "rope");
      CRS_TRY(crs::attention_launch(p.attn, qkv, lens_dev, ctx, batch, seq, H, d->heads, rel_bias, rel_span, st), "attention");
    }
    CRS_TRY(proj_ln(p.out, ctx, L.w_o, L.b_o, L.ln1_g, L.ln1_b, H), "out projection + layernorm 1");
    CRS_TRY(crs::gemm_launch(p.up, x16, (const _Float16*)L.w_up, L.b_up, nullptr, ffn, st), "ffn up gemm");
    CRS_TRY(proj_ln(p.down, ffn, L.w_down, L.b_down, L.ln2_g, L.ln2_b, F), "ffn down projection + layernorm 2");
  }
  if (hidden_out_dev) {
    const hipError_t e = hipMemcpyAsync(hidden_out_dev, final32, (size_t)T * H * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return crs::set_error(CRS_EHIP, hipGetErrorString(e));
  }
  if (pair) {
    const crs_encoder_head* hd = pair->head;
    CRS_TRY(crs::pair_head_launch(x32, batch, seq, H, hd->w_pool, hd->b_pool, hd->w_cls, hd->b_cls, hd->activation, pair->scores,
                                  pair->pooled_out, st), "pair head");
    return CRS_OK;
  }
  CRS_TRY(crs::pool_launch(final32, lens_dev, batch, seq, H, d->pooling, normalize, out_dev, q16_out_dev, q16_row_elems, st), "pool");
  return CRS_OK;
}

int crs_encoder_forward_prenorm(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                const int32_t* lens_dev, int batch, int seq, void* workspace_dev, size_t workspace_bytes,
                                float* out_dev, int normalize, float* hidden_out_dev, void* stream, const crs_encoder_prenorm* pre) {
  if (!pre) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM needs both rope tables (crs_encoder_prenorm)");
  return encoder_forward(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, normalize, hidden_out_dev,
                         nullptr, 0, stream, nullptr, nullptr, nullptr, pre);
}

int crs_encoder_forward_queries_prenorm(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                        const int32_t* lens_dev, int batch, int seq, void* workspace_dev, size_t workspace_bytes,
                                        float* out_dev, void* q16_out_dev, int slab_type, void* stream,
                                        const crs_encoder_prenorm* pre) {
  if (!q16_out_dev) return crs::set_error(CRS_EINVAL, "null pointer");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return crs::set_error(CRS_EINVAL, "bad slab_type");
  if (!d) return crs::set_error(CRS_EINVAL, "null descriptor");
  if (!pre) return crs::set_error(CRS_EINVAL, "CRS_ENC_PRENORM needs both rope tables (crs_encoder_prenorm)");
  return encoder_forward(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, 1, nullptr,
                         reinterpret_cast<_Float16*>(q16_out_dev), crs_row_elems(d->hidden, slab_type), stream, nullptr, nullptr, nullptr, pre);
}

int crs_encoder_prenorm_plan_describe(const crs_encoder_desc* d, int batch, int seq, int window, char* buf, size_t cap) {
  const int rc = check_desc(d);
  if (rc) return rc;
  if (!(d->flags & CRS_ENC_PRENORM) || !(d->flags & CRS_ENC_ROTARY)) return crs::set_error(CRS_EINVAL, "prenorm plan describe: the descriptor needs CRS_ENC_PRENORM and CRS_ENC_ROTARY");
  if (batch <= 0 || seq <= 0 || seq > d->max_pos || window < 1 || (cap && !buf)) return crs::set_error(CRS_EINVAL, "bad batch/seq (seq <= max_pos), window or buffer");
  const int cus = crs::device_cus();
  if (cus <= 0) return crs::set_error(CRS_EHIP, "plan describe: no device");
  return crs::enc_plan_describe(plan_for(d, batch, seq, 0, 0, cus, window), buf, cap);
}

int crs_encoder_score_pairs(const crs_encoder_desc* d, const crs_encoder_weights* w, const crs_encoder_head* head,
                            const int32_t* ids_dev, const int32_t* type_ids_dev, const int32_t* lens_dev, int batch, int seq,
                            void* workspace_dev, size_t workspace_bytes, float* scores_dev, float* pooled_out_dev,
                            float* hidden_out_dev, void* stream) {
  const int rc = check_desc(d);
  if (rc) return rc;
  if (!head) return crs::set_error(CRS_EINVAL, "score_pairs: null head");
  if (!head->w_pool || !head->b_pool || !head->w_cls || !head->b_cls) return crs::set_error(CRS_EINVAL, "score_pairs: null pointer in the head (w_pool, b_pool, w_cls, b_cls)");
  if (head->type_rows < 1) return crs::set_error(CRS_EINVAL, "score_pairs: type_rows must be >= 1");
  if (head->activation != 0 && head->activation != 1) return crs::set_error(CRS_EINVAL, "score_pairs: activation must be 0 (identity) or 1 (sigmoid)");
  if (batch < 1) return crs::set_error(CRS_EINVAL, "score_pairs: batch must be >= 1");
  if (seq < 1 || seq > d->max_pos) {
    char m[160];
    snprintf(m, sizeof m, "score_pairs: seq %d must be in [1, max_pos %d]", seq, d->max_pos);
    return crs::set_error(CRS_EINVAL, m);
  }
  const PairTail pair{head, type_ids_dev, scores_dev, pooled_out_dev};
  return encoder_forward(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, nullptr, 0, hidden_out_dev, nullptr, 0,
                         stream, nullptr, &pair);
}

int crs_encoder_forward_rope(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                             const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                             size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                             void* stream, const crs_encoder_ext* ext, const crs_encoder_rope* rope) {
  return encoder_forward(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, normalize,
                         hidden_out_dev, nullptr, 0, stream, ext, nullptr, rope);
}

int crs_encoder_forward_ex(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                           const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                           size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                           void* stream, const crs_encoder_ext* ext) {
  return crs_encoder_forward_rope(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, normalize,
                                  hidden_out_dev, stream, ext, nullptr);
}

int crs_encoder_forward(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                        const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                        size_t workspace_bytes, float* out_dev, int normalize, float* hidden_out_dev,
                        void* stream) {
  return crs_encoder_forward_ex(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, normalize,
                                hidden_out_dev, stream, nullptr);
}

int crs_encoder_forward_queries_rope(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                     const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                                     size_t workspace_bytes, float* out_dev, void* q16_out_dev, int slab_type,
                                     void* stream, const crs_encoder_ext* ext, const crs_encoder_rope* rope) {
  if (!q16_out_dev) return crs::set_error(CRS_EINVAL, "null pointer");
  if (slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) return crs::set_error(CRS_EINVAL, "bad slab_type");
  if (!d) return crs::set_error(CRS_EINVAL, "null descriptor");
  return encoder_forward(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, 1, nullptr,
                         reinterpret_cast<_Float16*>(q16_out_dev), crs_row_elems(d->hidden, slab_type), stream, ext, nullptr, rope);
}

int crs_encoder_forward_queries_ex(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                   const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                                   size_t workspace_bytes, float* out_dev, void* q16_out_dev, int slab_type,
                                   void* stream, const crs_encoder_ext* ext) {
  return crs_encoder_forward_queries_rope(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev, q16_out_dev,
                                          slab_type, stream, ext, nullptr);
}

int crs_rope_qk_f16(void* qkv_dev, const float* table_dev, int positions, int batch, int seq, int hidden, int heads, void* stream) {
  if (!qkv_dev || !table_dev || (((uintptr_t)qkv_dev | (uintptr_t)table_dev) & 15)) return crs::set_error(CRS_EINVAL, "rope: NULL or misaligned (16 bytes) pointer");
  if (batch < 1 || seq < 1 || heads < 1 || hidden < 1 || hidden % heads) return crs::set_error(CRS_EINVAL, "rope: bad batch / seq / hidden / heads");
  const int hd = hidden / heads;
  if (hd != 16 && hd != 32 && hd != 64) return crs::set_error(CRS_EINVAL, "rope: head_dim must be 16, 32 or 64");
  if (positions < seq) return crs::set_error(CRS_EINVAL, "rope: positions must be >= seq");
  if ((long)batch * seq > (1L << 24)) return crs::set_error(CRS_EINVAL, "rope: more than 2^24 tokens");
  CRS_TRY(crs::rope_qk_launch(crs::plan_rope(batch * seq, hidden), hd, (_Float16*)qkv_dev, table_dev, batch * seq, seq, hidden, (hipStream_t)stream), "rope");
  return CRS_OK;
}

// ---- the attention step on its own: the plan is plan_attention's (or plan_qkv_attn's), the launch attention_launch's ----
int crs_attention_f16(const void* qkv_dev, const int32_t* lens_dev, void* ctx_dev, int batch, int seq, int hidden, int heads,
                      const float* rel_bias_dev, int rel_span, int route, void* stream) {
  if (!qkv_dev || !lens_dev || !ctx_dev) return crs::set_error(CRS_EINVAL, "attention: null pointer");
  if (((uintptr_t)qkv_dev | (uintptr_t)lens_dev | (uintptr_t)ctx_dev | (uintptr_t)rel_bias_dev) & 15)
    return crs::set_error(CRS_EINVAL, "attention pointers must be 16-byte aligned");
  const char* why = attn_sizes_refusal(batch, seq, hidden, heads);
  if (!why && rel_bias_dev) why = attn_bias_refusal(seq, rel_span);
  if (!why && route > 15) why = "attention: route must be < 0 (the process's knobs) or a sum of 1, 2, 4, 8";
  if (why) return crs::set_error(CRS_EINVAL, why);
  const crs::AttnPlan p = crs::plan_attention(batch, seq, heads, hidden / heads, rel_bias_dev != nullptr, attn_knobs(route));
  CRS_TRY(crs::attention_launch(p, (const _Float16*)qkv_dev, lens_dev, (_Float16*)ctx_dev, batch, seq, hidden, heads, rel_bias_dev,
                                rel_bias_dev ? rel_span : 0, (hipStream_t)stream), "attention");
  return CRS_OK;
}

int crs_attention_window_f16(const void* qkv_dev, const int32_t* lens_dev, void* ctx_dev, int batch, int seq, int hidden, int heads,
                             int window, void* stream) {
  if (!qkv_dev || !lens_dev || !ctx_dev) return crs::set_error(CRS_EINVAL, "attention: null pointer");
  if (((uintptr_t)qkv_dev | (uintptr_t)lens_dev | (uintptr_t)ctx_dev) & 15) return crs::set_error(CRS_EINVAL, "attention pointers must be 16-byte aligned");
  const char* why = attn_sizes_refusal(batch, seq, hidden, heads);
  if (!why && window < 1) why = "attention: window must be >= 1";
  if (why) return crs::set_error(CRS_EINVAL, why);
  const crs::AttnPlan p = crs::plan_attention_window(batch, seq, heads, hidden / heads, window, knobs());
  CRS_TRY(crs::attention_window_launch(p, (const _Float16*)qkv_dev, lens_dev, (_Float16*)ctx_dev, seq, hidden, (hipStream_t)stream), "windowed attention");
  return CRS_OK;
}

int crs_attention_window_plan_describe(int batch, int seq, int hidden, int heads, int window, char* buf, size_t cap) {
  if (cap && !buf) return crs::set_error(CRS_EINVAL, "plan describe: null buffer");
  const char* why = attn_sizes_refusal(batch, seq, hidden, heads);
  if (!why && window < 1) why = "attention: window must be >= 1";
  if (why) return crs::set_error(CRS_EINVAL, why);
  return crs::attn_plan_describe(crs::plan_attention_window(batch, seq, heads, hidden / heads, window, knobs()), buf, cap);
}

int crs_qkv_attn_f16(const void* x16_dev, const void* w_qkv_dev, const float* b_qkv_dev, const int32_t* lens_dev, void* ctx_dev,
                     int batch, int seq, int hidden, int heads, void* stream) {
  if (!x16_dev || !w_qkv_dev || !b_qkv_dev || !lens_dev || !ctx_dev) return crs::set_error(CRS_EINVAL, "qkv + attention: null pointer");
  if (((uintptr_t)x16_dev | (uintptr_t)w_qkv_dev | (uintptr_t)b_qkv_dev | (uintptr_t)lens_dev | (uintptr_t)ctx_dev) & 15)
    return crs::set_error(CRS_EINVAL, "qkv + attention pointers must be 16-byte aligned");
  const char* why = attn_sizes_refusal(batch, seq, hidden, heads);
  if (!why && (!crs::qkv_attn_supported(hidden, heads, seq) || (long)batch * seq > 4096))
    why = "qkv + attention: hidden 128 / 256 / 384, head_dim 32 / 64 within the LDS image, seq 16 / 32 / 64, batch * seq <= 4096";
  if (why) return crs::set_error(CRS_EINVAL, why);
  const crs::AttnPlan p = crs::plan_qkv_attn(batch * seq, hidden, heads);
  CRS_TRY(crs::qkv_attn_launch(p, (const _Float16*)x16_dev, (const _Float16*)w_qkv_dev, b_qkv_dev, lens_dev, (_Float16*)ctx_dev,
                               batch * seq, seq, hidden, (hipStream_t)stream), "qkv + attention");
  return CRS_OK;
}

int crs_attention_plan_describe(int batch, int seq, int hidden, int heads, int rel_bias, int route, char* buf, size_t cap) {
  if (cap && !buf) return crs::set_error(CRS_EINVAL, "plan describe: null buffer");
  const char* why = attn_sizes_refusal(batch, seq, hidden, heads);
  if (!why && route > 16) why = "attention: route must be < 0, a sum of 1, 2, 4, 8, or 16 (crs_qkv_attn_f16's launch)";
  if (!why && route == 16 && (rel_bias || !crs::qkv_attn_supported(hidden, heads, seq) || (long)batch * seq > 4096))
    why = "qkv + attention: no bias, hidden 128 / 256 / 384, head_dim 32 / 64 within the LDS image, seq 16 / 32 / 64, batch * seq <= 4096";
  if (!why && route != 16 && rel_bias && seq > crs::forms::kAttnMaxBiasSeq) why = "attention: a relative bias needs seq <= 512";
  if (why) return crs::set_error(CRS_EINVAL, why);
  if (route == 16) return crs::attn_plan_describe(crs::plan_qkv_attn(batch * seq, hidden, heads), buf, cap);
  return crs::attn_plan_describe(crs::plan_attention(batch, seq, heads, hidden / heads, rel_bias != 0, attn_knobs(route)), buf, cap);
}

// ---- the row kernels on their own (enc_misc.hip, enc_pair.hip): each entry checks its arguments and calls the launcher the forward calls ----
int crs_embed_ln_f32(const int32_t* ids_dev, const int32_t* type_ids_dev, int type_rows, const float* word_dev, const float* pos_dev,
                     const float* type_dev, const float* g_dev, const float* b_dev, float eps, int tokens, int seq, int hidden,
                     int vocab, float* x32_dev, void* x16_dev, void* stream) {
  if (!ids_dev || !word_dev || !type_dev || !g_dev || !b_dev || !x32_dev || !x16_dev) return crs::set_error(CRS_EINVAL, "embed_ln: null pointer");
  if (row_misaligned({ids_dev, type_ids_dev, word_dev, pos_dev, type_dev, g_dev, b_dev, x32_dev, x16_dev}))
    return crs::set_error(CRS_EINVAL, "embed_ln pointers must be 16-byte aligned");
  const char* why = row_hidden_refusal(hidden);
  if (!why && (tokens < 1 || seq < 1)) why = "embed_ln: tokens and seq must be >= 1";
  if (!why && vocab < 1) why = "embed_ln: vocab must be >= 1";
  if (!why && type_ids_dev && type_rows < 1) why = "embed_ln: type_rows must be >= 1";
  if (why) return crs::set_error(CRS_EINVAL, why);
  CRS_TRY(crs::embed_ln_launch(ids_dev, type_ids_dev, word_dev, pos_dev, type_dev, type_rows, g_dev, b_dev, eps, tokens, seq, hidden,
                               vocab, x32_dev, (_Float16*)x16_dev, (hipStream_t)stream), "embed_ln");
  return CRS_OK;
}

int crs_layernorm_f32(const float* y_dev, int nsplit, const float* bias_dev, const float* residual_dev, const float* g_dev,
                      const float* b_dev, float eps, int tokens, int hidden, float* x32_dev, void* x16_dev, void* stream) {
  if (!y_dev || !g_dev || !b_dev || !x32_dev || !x16_dev) return crs::set_error(CRS_EINVAL, "layernorm: null pointer");
  if (row_misaligned({y_dev, bias_dev, residual_dev, g_dev, b_dev, x32_dev, x16_dev}))
    return crs::set_error(CRS_EINVAL, "layernorm pointers must be 16-byte aligned");
  const char* why = row_hidden_refusal(hidden);
  if (!why && tokens < 1) why = "layernorm: tokens must be >= 1";
  if (!why && !crs::forms::ln_slabs_ok(nsplit)) why = "layernorm: nsplit must be 1, 2, 3, 4, 6, 8 or 16";
  if (why) return crs::set_error(CRS_EINVAL, why);
  CRS_TRY(crs::layernorm_launch(y_dev, nsplit, bias_dev, residual_dev, g_dev, b_dev, eps, tokens, hidden, x32_dev, (_Float16*)x16_dev,
                                (hipStream_t)stream), "layernorm");
  return CRS_OK;
}

int crs_add_layernorm_f32(const float* y_dev, int nsplit, const float* bias_dev, const float* residual_dev, const float* g_dev,
                          const float* b_dev, float eps, int tokens, int hidden, float* r32_dev, void* x16_dev, float* n32_dev,
                          void* stream) {
  if (!y_dev || !g_dev || !r32_dev || !x16_dev) return crs::set_error(CRS_EINVAL, "add_layernorm: null pointer");
  if (row_misaligned({y_dev, bias_dev, residual_dev, g_dev, b_dev, r32_dev, x16_dev, n32_dev}))
    return crs::set_error(CRS_EINVAL, "add_layernorm pointers must be 16-byte aligned");
  const char* why = row_hidden_refusal(hidden);
  if (!why && tokens < 1) why = "add_layernorm: tokens must be >= 1";
  if (!why && !crs::forms::ln_slabs_ok(nsplit)) why = "add_layernorm: nsplit must be 1, 2, 3, 4, 6, 8 or 16";
  if (why) return crs::set_error(CRS_EINVAL, why);
  CRS_TRY(crs::add_layernorm_launch(y_dev, nsplit, bias_dev, residual_dev, g_dev, b_dev, eps, tokens, hidden, r32_dev, (_Float16*)x16_dev,
                                    n32_dev, (hipStream_t)stream), "add_layernorm");
  return CRS_OK;
}

int crs_pool_f32(const float* x32_dev, const int32_t* lens_dev, int batch, int seq, int hidden, int pooling, int normalize,
                 float* out_dev, void* out16_dev, int slab_type, void* stream) {
  if (!x32_dev || !lens_dev || !out_dev) return crs::set_error(CRS_EINVAL, "pool: null pointer");
  if (row_misaligned({x32_dev, lens_dev, out_dev, out16_dev})) return crs::set_error(CRS_EINVAL, "pool pointers must be 16-byte aligned");
  const char* why = row_hidden_refusal(hidden);
  if (!why && (batch < 1 || seq < 1)) why = "pool: batch and seq must be >= 1";
  if (!why && pooling != CRS_POOL_MEAN && pooling != CRS_POOL_CLS) why = "bad pooling mode";
  if (!why && slab_type != CRS_SLAB_F16 && slab_type != CRS_SLAB_I8) why = "bad slab_type";
  if (why) return crs::set_error(CRS_EINVAL, why);
  CRS_TRY(crs::pool_launch(x32_dev, lens_dev, batch, seq, hidden, pooling, normalize, out_dev, (_Float16*)out16_dev,
                           crs_row_elems(hidden, slab_type), (hipStream_t)stream), "pool");
  return CRS_OK;
}

int crs_pair_head_f32(const float* hidden_dev, int batch, int seq, int hidden, const float* w_pool_dev, const float* b_pool_dev,
                      const float* w_cls_dev, const float* b_cls_dev, int activation, float* scores_dev, float* pooled_out_dev,
                      void* stream) {
  if (!hidden_dev || !w_pool_dev || !b_pool_dev || !w_cls_dev || !b_cls_dev || !scores_dev) return crs::set_error(CRS_EINVAL, "pair_head: null pointer");
  if (row_misaligned({hidden_dev, w_pool_dev, b_pool_dev, w_cls_dev, b_cls_dev, scores_dev, pooled_out_dev}))
    return crs::set_error(CRS_EINVAL, "pair_head pointers must be 16-byte aligned");
  const char* why = row_hidden_refusal(hidden);
  if (!why && (batch < 1 || seq < 1)) why = "pair_head: batch and seq must be >= 1";
  if (!why && activation != 0 && activation != 1) why = "pair_head: activation must be 0 (identity) or 1 (sigmoid)";
  if (why) return crs::set_error(CRS_EINVAL, why);
  CRS_TRY(crs::pair_head_launch(hidden_dev, batch, seq, hidden, w_pool_dev, b_pool_dev, w_cls_dev, b_cls_dev, activation, scores_dev,
                                pooled_out_dev, (hipStream_t)stream), "pair head");
  return CRS_OK;
}

int crs_row_plan_describe(int kind, int rows, int hidden, int arg, char* buf, size_t cap) {
  if (cap && !buf) return crs::set_error(CRS_EINVAL, "plan describe: null buffer");
  const char* why = row_hidden_refusal(hidden);
  if (!why && (kind < crs::kRowEmbed || kind > crs::kRowAddLayerNorm)) why = "row plan describe: kind must be 0 (embedding), 1 (LayerNorm), 2 (pool), 3 (pair head) or 4 (add + LayerNorm)";
  if (!why && rows < 1) why = "row plan describe: rows (tokens, or the batch of the pool and pair-head kernels) must be >= 1";
  if (!why && (kind == crs::kRowLayerNorm || kind == crs::kRowAddLayerNorm) && !crs::forms::ln_slabs_ok(arg)) why = "layernorm: nsplit must be 1, 2, 3, 4, 6, 8 or 16";
  if (why) return crs::set_error(CRS_EINVAL, why);
  return crs::row_plan_describe(kind, rows, hidden, arg, buf, cap);
}

int crs_encoder_forward_queries(const crs_encoder_desc* d, const crs_encoder_weights* w, const int32_t* ids_dev,
                                const int32_t* lens_dev, int batch, int seq, void* workspace_dev,
                                size_t workspace_bytes, float* out_dev, void* q16_out_dev, int slab_type,
                                void* stream) {
  return crs_encoder_forward_queries_ex(d, w, ids_dev, lens_dev, batch, seq, workspace_dev, workspace_bytes, out_dev,
                                        q16_out_dev, slab_type, stream, nullptr);
}

// ---- the masked-language-model head with the max-pool epilogue (mlm_pool.hip; the geometry is mlm_plan.cpp's) ----
int crs_mlm_pool_plan(int batch, int seq, int hidden, int vocab, crs_mlm_plan* plan) {
  if (!plan) return crs::set_error(CRS_EINVAL, "null pointer");
  const char* why = "";
  if (crs::make_mlm_plan(batch, seq, hidden, vocab, plan, &why)) return crs::set_error(CRS_EINVAL, why);
  return CRS_OK;
}

int crs_mlm_workspace_bytes(int batch, int seq, int hidden, int vocab, size_t* bytes) {
  if (!bytes) return crs::set_error(CRS_EINVAL, "null pointer");
  crs_mlm_plan p;
  const int rc = crs_mlm_pool_plan(batch, seq, hidden, vocab, &p);
  if (rc) return rc;
  *bytes = p.workspace_bytes;
  return CRS_OK;
}

int crs_mlm_sparse_pool(const float* hidden_dev, const int32_t* lens_dev, int batch, int seq, const crs_mlm_head* head,
                        void* workspace_dev, size_t workspace_bytes, float* out_dev, int vp, void* stream) {
  if (!head) return crs::set_error(CRS_EINVAL, "null head");
  if (!hidden_dev || !lens_dev || !out_dev || !head->transform_w16 || !head->transform_bias || !head->ln_gamma || !head->ln_beta ||
      !head->decoder_w16 || !head->decoder_bias)
    return crs::set_error(CRS_EINVAL, "null pointer");
  crs_mlm_plan p;
  const int rc = crs_mlm_pool_plan(batch, seq, head->hidden, head->vocab, &p);
  if (rc) return rc;
  if (seq > head->max_pos) return crs::set_error(CRS_EINVAL, "bad seq (seq <= max_pos)");
  if (vp < head->vocab) return crs::set_error(CRS_EINVAL, "bad vp (vp >= vocab)");
  if (((uintptr_t)hidden_dev | (uintptr_t)head->transform_w16 | (uintptr_t)head->decoder_w16) & 15)
    return crs::set_error(CRS_EINVAL, "hidden_dev / transform_w16 / decoder_w16 must be 16-byte aligned");
  if (!workspace_dev || ((uintptr_t)workspace_dev & 255)) return crs::set_error(CRS_EINVAL, "workspace must be a 256-byte aligned device pointer");
  if (workspace_bytes < p.workspace_bytes) return crs::set_error(CRS_ENOSPC, "workspace smaller than crs_mlm_workspace_bytes");
  CRS_TRY(crs::mlm_sparse_pool_launch(p, hidden_dev, lens_dev, batch, seq, *head, reinterpret_cast<_Float16*>(workspace_dev), out_dev, vp,
                                      (hipStream_t)stream), "mlm_sparse_pool");
  return CRS_OK;
}

}  // extern "C"
