// enc_plan.h -- the plan of an encoder forward: which kernel every step of a layer runs on, with its grid, workgroup size, dynamic
// LDS and every launch argument that is not a pointer, plus the workspace layout.  make_enc_plan and plan_gemm are pure functions
// of the sizes, the CU count and the knobs (enc_plan.cpp: plain C++17, no HIP, no allocation), so tools/enc_plan_table.cpp and
// tests/test_enc_plan_cpu.py run them without a device.  The launchers of the enc_*.hip files switch on a plan's fields to pick
// the instantiation and launch; they decide nothing.
#pragma once
#include <stddef.h>

#include "enc_forms.h"

namespace crs {

// Every CRS_* knob that planning an encoder call reads; enc_knobs_from_env() is the only reader, once, at the first plan of the process.
struct EncKnobs {
  // knob = default             variable                 meaning
  bool bigln = true;          // CRS_ENC_BIGLN          0: tiled GEMM + separate LayerNorm on the index-build side (A/B runs)
  bool qkvattn = true;        // CRS_ENC_QKVATTN        0: separate QKV GEMM and attention launches (A/B runs, tests)
  int splitk_max_tokens = 2048;  // CRS_SPLITK_MAX_TOKENS  most tokens whose multi-chunk contractions leave split-K panel slabs
  bool panel_multi = true;    // CRS_ENC_PANEL_MULTI    0: QKV / FFN-up on the panel kernel only when K = hidden is one chunk
  int panel_kc = 0;           // CRS_PANEL_KC           128 | 256 | 384: forces the panel kernel's staged chunk (A/B runs); else 0
  bool gemm_stream = true;    // CRS_GEMM_STREAM        0: no row-streaming kernel (A/B runs)
  int panel_max_split = 0;    // CRS_PANEL_MAX_SPLIT    > 0: cap of the panel's slab count (A/B runs); else by the row count
  int gemm8_var = 0;          // CRS_GEMM8_VAR          0..3: schedule variant of the 256 x 256 kernel; 1: one workgroup per item everywhere
  bool gemm8 = true;          // CRS_GEMM8              0: no 256 x 256 phase-scheduled kernel, whole-K or split-K (A/B runs)
  bool gemm8_half = true;     // CRS_GEMM8_HALF         0: N must be whole 256-column blocks (no last block of 128)
  long gemm8_min_wgs = 128;   // CRS_GEMM8_MIN_WGS      fewest 256 x 256 tiles the phase-scheduled kernel takes
  bool gemm_big = true;       // CRS_GEMM_BIG           0: no 256-row pipelined kernel (A/B runs)
  long gemm_big_min_wgs = 128;   // CRS_GEMM_BIG_MIN_WGS   fewest workgroups it takes
  bool attn_seq = true;       // CRS_ATTN_SEQ           0: no whole-sequence attention kernels
  bool attn_short = true;     // CRS_ATTN_SHORT         0: query-length sequences on the blocked kernel (A/B runs)
  bool attn_x32 = true;       // CRS_ATTN_X32           0: the 16x16x16 whole-sequence kernel (A/B runs)
  bool attn_qt4 = false;      // CRS_ATTN_QT            4: four query tiles per wave (A/B)
  int rowln2_variant = 1;     // CRS_ROWLN2_VARIANT     0: four-stage ring of 64-byte pieces; default 128-byte pieces, two stages
};
EncKnobs enc_knobs_from_env();

struct Dims { int gx = 0, gy = 1, gz = 1, threads = 0, lds = 0; };   // grid in workgroups, workgroup size, dynamic LDS bytes

enum class GemmFamily { None, Tiled, Panel, Stream, StreamKS, Big, Gemm8, Gemm8SplitK };

// C = epilogue(A[M,K] W[N,K]^T): mode 0 fp16 (+ bias), 1 GELU fp16, 2 + bias + residual fp32, 3 fp32 partial slabs [slabs][M][N]
// without bias (the LayerNorm that follows sums them and adds bias and residual), 4 silu(gate) * up fp16 [M, N / 2] (gate / up rows
// of W interleaved in blocks of 16, include/crs_encoder.h: CRS_ENC_GATED_SILU), 5 gelu(gate) * up in the same layout (CRS_ENC_GATED_GELU)
struct GemmPlan {
  GemmFamily family = GemmFamily::None;
  int m = 0, n = 0, k = 0, mode = 0;
  Dims d;
  int slabs = 1;          // fp32 slabs a mode-3 launch leaves
  int tm = 0;             // Panel: rows per tile, 64 or 128
  int kc = 0, kin = 0;    // Panel: staged chunk and chunks walked per workgroup; kin * slabs * kc == k
  bool persist = false;   // Gemm8: one workgroup per CU walks the items; else one workgroup per item
  int var = 0;            // Gemm8: schedule variant
  int items = 0, ksplit = 0;      // Gemm8: (tile, slab) items; contraction length per item
  int colblocks = 0, streams = 0; // Stream / StreamKS: 128-column blocks; row streams per block
};

// What crs_gemm_f16 and the encoder's fp16 / fp32 + residual projections run (modes 0..2): gemm8, then big, then stream, then tiled.
// Modes 4 and 5: gemm8, else tiled (the big and stream families have no gated epilogue and are never planned for them).
GemmPlan plan_gemm(int m, int n, int k, int mode, int small_lds, int cus, const EncKnobs& kn);
// The panel kernel on modes 0 / 1 / 3 / 4 / 5 (family None where K has no chunk); the caller decides that the shape is one for it.
GemmPlan plan_gemm_panel(int m, int n, int k, int mode, int small_lds, const EncKnobs& kn);

// The phase-scheduled 256 x 256 kernel's split-K form (mode 3, fp32 slabs summed by the LayerNorm): gemm8_splitk answers the slab
// count of a shape, 0 where the form does not apply (then no plan may be made); plan_gemm8 with mode 3 and that count is its plan.
int gemm8_splitk(int m, int n, int k, const EncKnobs& kn);
GemmPlan plan_gemm8(int m, int n, int k, int mode, int splits, int cus, const EncKnobs& kn);

enum class AttnForm { Fused, Blocked, Short, Seq, Seq32, Window };
struct AttnPlan {
  AttnForm form = AttnForm::Blocked;   // Fused: QKV projection + attention in one kernel (enc_qkvattn.hip), no QKV GEMM
  int hd = 0;
  bool bias = false;                   // Blocked only: relative-position bias
  int smax = 0, nw = 0, qt = 0;        // Seq / Seq32: template arguments
  int window = 0;                      // Window only: the largest allowed |key - query|
  Dims d;
};

// What the forward's attention step runs on when it is not Fused (crs_attention_f16 launches exactly this): the blocked kernel with
// a bias at every length; else the short kernel up to 16 tokens (head_dim 32 / 64), a whole-sequence kernel from 65 tokens up to the
// length its LDS image holds (256, or 512 at head_dim 64), the blocked kernel otherwise -- as the attn_* knobs allow.
AttnPlan plan_attention(int batch, int seq, int heads, int hd, bool bias, const EncKnobs& kn);
// The sliding-window layers of a pre-norm model (attention_window_kernel): the blocked kernel's grid at every length, window >= 1 the
// largest allowed |key - query|.  No knob moves it today.
AttnPlan plan_attention_window(int batch, int seq, int heads, int hd, int window, const EncKnobs& kn);
// The shapes qkv_attn_kernel takes (hidden a multiple of 128 up to 384, head_dim 32 / 64, its LDS image within kMaxLds, 16 / 32 / 64
// tokens per sequence) and its plan, the one make_enc_plan puts into EncPlan::attn; the caller checked qkv_attn_supported.
bool qkv_attn_supported(int hidden, int heads, int seq);
AttnPlan plan_qkv_attn(int tokens, int hidden, int heads);
// Default knobs with the attention bits of a test route applied: 1 attn_seq off, 2 attn_short off, 4 attn_x32 off, 8 attn_qt4 on
// (include/crs_encoder.h: crs_attention_f16).
EncKnobs attn_route_knobs(int route);

// out-projection / FFN-down + LayerNorm: one rowln2 launch, or a GEMM and the LayerNorm summing its slabs
struct ProjLnPlan {
  bool rowln2 = false;
  int variant = 0;     // rowln2: 0 = <32, 4>, 1 = <64, 2>
  Dims d;              // rowln2
  GemmPlan gemm;       // mode 3 (the LayerNorm adds bias and residual) or mode 2 (already folded in, slabs = 1)
  Dims ln;
  bool prenorm = false;   // the row kernel is add_layernorm*_kernel (never rowln2)
};

// big_ln: the index-build side (make_enc_plan: more than 4096 tokens and CRS_ENC_BIGLN); then rowln2 where it has the shape, else
// panel slabs, else gemm8 split-K, else the mode-2 GEMM of plan_gemm
ProjLnPlan plan_proj_ln(int tokens, int hidden, int k, bool big_ln, int small_lds, int cus, const EncKnobs& kn);

// rope_qk_kernel's launch: hidden / 8 threads per token (enc_forms.h), no LDS; a function of the two sizes alone
Dims plan_rope(int tokens, int hidden);

// The launches of the row kernels (enc_misc.hip, enc_pair.hip), functions of the sizes alone: the embedding and LayerNorm kernels
// give a wave to each token row, four rows per workgroup; pool_kernel a workgroup per sentence; pair_head_kernel a workgroup
// and kPairGroup x hidden floats of LDS per kPairGroup pairs.  make_enc_plan and plan_proj_ln take their Dims from these.
Dims plan_rows(int tokens);
Dims plan_pool(int batch);
Dims plan_pair_head(int batch, int hidden);

struct EncPlan {
  int hidden, heads, ffn, batch, seq, tokens;
  bool typed;          // embedding with a token-type row per token (pair forward with type ids)
  bool rotary, gated;  // CRS_ENC_ROTARY: rope between qkv and attn, never Fused; CRS_ENC_GATED_SILU / _GELU: up is mode 4 / 5 over 2 ffn rows
  bool prenorm;        // CRS_ENC_PRENORM: out / down are a GEMM + add_layernorm (never Fused, never rowln2); win is the sliding layers' attention
  AttnPlan win;        // prenorm only (form Window); attn is the full-attention layers' plan
  Dims rope;           // rotary only
  int pair;            // 0: pooling tail; else the pair head
  Dims embed, tail;
  AttnPlan attn;
  GemmPlan qkv;        // family None when attn.form == Fused
  ProjLnPlan out, down;
  GemmPlan up;
  // workspace: [x32 | y32 (max_split slabs) | x16 | ctx | qkv | ffn], each 256-byte aligned
  size_t x32, y32, x16, ctx, qkv_off, ffn_off, total;
  int max_split;
};

// flags: crs_encoder_desc.flags (SMALL_LDS 1, ROTARY 2, GATED_SILU 4, PRENORM 8, GATED_GELU 16); window: PRENORM only, >= 1; rel_bias: 1 with a relative-position bias; pair: 0 pooling tail, 1 pair head with type ids,
// 2 pair head without.  The sizes are check_desc's (hidden % 64 == 0 <= 1024, head_dim 16 / 32 / 64, ffn % 64 == 0).
EncPlan make_enc_plan(int hidden, int heads, int ffn, int flags, int batch, int seq, int rel_bias, int pair, int cus, const EncKnobs& kn,
                      int window = 0);

// One line per launch of embedding, ONE layer and the tail, in launch order: "<kernel><template arguments> grid=XxYxZ wg=Nx1x1 lds=BYTES\n"
// (grid in workgroups, dynamic LDS).  Returns the length of the whole text (snprintf): > cap - 1 means it was cut.
int gemm_plan_describe(const GemmPlan& p, char* buf, size_t cap);
int proj_ln_plan_describe(const ProjLnPlan& p, int hidden, char* buf, size_t cap);   // rowln2: one line; else the GEMM's and the LayerNorm's
int attn_plan_describe(const AttnPlan& p, char* buf, size_t cap);                    // the attention step's line, any form
int enc_plan_describe(const EncPlan& p, char* buf, size_t cap);
// One row kernel's line, as enc_plan_describe and proj_ln_plan_describe print it (include/crs_encoder.h: crs_row_plan_describe).
// kind 0: embedding, rows = tokens, arg != 0 with type ids; 1: LayerNorm, rows = tokens, arg = slabs; 2: pooling, rows = batch;
// 3: pair head, rows = batch.  The caller has checked the sizes; an unknown kind gives the empty text.
// 4: the pre-norm add + LayerNorm, rows = tokens, arg = slabs.
enum RowKind { kRowEmbed = 0, kRowLayerNorm = 1, kRowPool = 2, kRowPairHead = 3, kRowAddLayerNorm = 4 };
int row_plan_describe(int kind, int rows, int hidden, int arg, char* buf, size_t cap);

}  // namespace crs
