// enc_plan.cpp -- the encoder's planner: plain C++17, no HIP, no device, no allocation (enc_plan.h).  tools/enc_plan_table.cpp
// builds it alone.
#include "enc_plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

namespace crs {

using namespace forms;

EncKnobs enc_knobs_from_env() {
  EncKnobs k;
  auto off = [](const char* name) { const char* e = getenv(name); return !(e && e[0] == '0'); };   // on unless "0..."
  k.bigln = off("CRS_ENC_BIGLN");
  k.qkvattn = off("CRS_ENC_QKVATTN");
  if (const char* e = getenv("CRS_SPLITK_MAX_TOKENS")) k.splitk_max_tokens = atoi(e);
  k.panel_multi = off("CRS_ENC_PANEL_MULTI");
  if (const char* e = getenv("CRS_PANEL_KC")) { k.panel_kc = atoi(e); if (k.panel_kc != 128 && k.panel_kc != 256 && k.panel_kc != 384) k.panel_kc = 0; }
  k.gemm_stream = off("CRS_GEMM_STREAM");
  if (const char* e = getenv("CRS_PANEL_MAX_SPLIT")) k.panel_max_split = atoi(e);
  if (const char* e = getenv("CRS_GEMM8_VAR")) k.gemm8_var = (e[0] >= '0' && e[0] <= '3') ? e[0] - '0' : 0;
  k.gemm8 = off("CRS_GEMM8");
  k.gemm8_half = off("CRS_GEMM8_HALF");
  if (const char* e = getenv("CRS_GEMM8_MIN_WGS")) k.gemm8_min_wgs = atol(e);
  k.gemm_big = off("CRS_GEMM_BIG");
  if (const char* e = getenv("CRS_GEMM_BIG_MIN_WGS")) k.gemm_big_min_wgs = atol(e);
  k.attn_seq = off("CRS_ATTN_SEQ");
  k.attn_short = off("CRS_ATTN_SHORT");
  k.attn_x32 = off("CRS_ATTN_X32");
  if (const char* e = getenv("CRS_ATTN_QT")) k.attn_qt4 = e[0] == '4';
  k.rowln2_variant = off("CRS_ROWLN2_VARIANT") ? 1 : 0;
  return k;
}

namespace {

int cdiv(int a, int b) { return (a + b - 1) / b; }
size_t up256(size_t x) { return (x + 255) / 256 * 256; }

// Small token counts are latency-bound: use the one-shot panel GEMM (+ split-K partials reduced in
// the LayerNorm); large ones (index build) use the pipelined 128 x 128 kernel.
constexpr int kPanelMaxTokens = 4096;
// split-K panels (fp32 partials summed by the LayerNorm): round 1 measured them losing at 4096 tokens of bge (C3 step 2.79 ms
// against 2.05 through the tiled kernel's fused epilogue) -- with one-shot 384-column staging and 2 / 8 slabs.  With the
// workgroups walking their K range in 128-column pieces and the slab count capped by the row count (panel_splits) a
// SINGLE forward at 4096 tokens is faster through split-K panels (bge-base 256 x 16 tokens: 1996 -> 1855 us, one stream), but
// with eight batches in flight the extra slab traffic costs more than the latency it saves (C3: 2.21 against 2.11 ms per
// batch, tools/ab_c3.sh) -- so the limit stays at 2048 tokens (bge-base 128 x 16: 1500 -> 1140 us); CRS_SPLITK_MAX_TOKENS
// moves it (EncKnobs::splitk_max_tokens)

// How many fp32 partial slabs a mode-3 panel launch of m rows over contraction length k leaves (the LayerNorm kernel that
// follows sums them): k / chunk, capped -- past the cap the workgroups walk several chunks each (kernel: kin).  The
// cap falls with the row count, because the slabs are m x N x 4 bytes each and the launch no longer lacks workgroups
// (bge-base FFN-down, K = 3072, tools/enc_chain_profile.py, whole forward): 1024 tokens: 8 / 4 / 2 slabs = 806 / 792 /
// 850 us; 2048 tokens: - / 1138 / 1132; 4096 tokens: 2109 / 1945 / 1855 (and 1996 through the 128 x 128 kernel).
int panel_splits(int k, int m, const EncKnobs& kn) {
  const int kc = panel_chunk(k);
  if (kc == 0) return 0;
  const int cap = kn.panel_max_split > 0 ? kn.panel_max_split : (m <= 1024 ? 4 : 2);
  int s = k / kc;
  while (s > cap && (s % 2) == 0) s /= 2;
  return s;
}

// out-projection / FFN-down as split-K panel slabs: the slab count must be one the LayerNorm kernel sums (16 is left to A/B
// settings of the cap: not taken)
bool use_panel(int tokens, int k, const EncKnobs& kn) {
  const int kc = panel_chunk(k);
  if (tokens > kPanelMaxTokens || kc == 0) return false;
  if (k / kc > 1 && tokens > kn.splitk_max_tokens) return false;
  const int ns = panel_splits(k, tokens, kn);
  return ns != 16 && ln_slabs_ok(ns);
}

// Shapes the phase-scheduled kernel takes: whole 256-row tiles, N whole 256-column blocks or (CRS_GEMM8_HALF) a last block of
// 128 -- MiniLM's 384 / 1152 --, K a multiple of 128 and >= 256 (two k-tiles in the prologue), 16-byte aligned rows, and enough
// tiles (CRS_GEMM8_MIN_WGS).
bool gemm8_applies(int m, int n, int k, const EncKnobs& kn) {
  const bool n_ok = n % kG8N == 0 || (kn.gemm8_half && n % 128 == 0 && n > kG8N);
  if (!kn.gemm8 || m % kG8M || !n_ok || k % 128 || k < 256) return false;
  return (long)(m / kG8M) * cdiv(n, kG8N) >= kn.gemm8_min_wgs;
}

}  // namespace

// Split-K form for projections whose output has too few 256 x 256 tiles to fill the chip (bge-base's N = 768 at a few
// thousand tokens): the number of K slabs (0 = not applicable) such that tiles x slabs >= 128 workgroups, every slab a
// multiple of 128 columns and >= 256; the LayerNorm kernel that follows sums the fp32 slabs.
int gemm8_splitk(int m, int n, int k, const EncKnobs& kn) {
  if (!kn.gemm8 || m % kG8M || n % kG8N || m < 2048) return 0;
  const long tiles = (long)(m / kG8M) * (n / kG8N);
  if (tiles >= 128) return 0;
  for (int s : kG8SplitK)
    if (k % s == 0 && (k / s) % 128 == 0 && k / s >= 256 && tiles * s >= 128) return s;
  return 0;
}

GemmPlan plan_gemm8(int m, int n, int k, int mode, int splits, int cus, const EncKnobs& kn) {
  GemmPlan p;
  p.family = mode == 3 ? GemmFamily::Gemm8SplitK : GemmFamily::Gemm8;
  p.m = m, p.n = n, p.k = k, p.mode = mode, p.slabs = mode == 3 ? splits : 1, p.var = kn.gemm8_var;
  p.items = cdiv(n, kG8N) * (m / kG8M) * p.slabs;
  // the stream pays for the fp16 epilogues (bias / GELU; + 8 % at K = 768 and 384: their VALU and stores sit beside the next item's
  // first phases) and measured 4 % slower for the fp32 + residual ones (the residual loads of the 16-row passes drain behind the
  // transfers in flight): those keep one workgroup per item.  CRS_GEMM8_VAR=1: one workgroup per item everywhere (A/B)
  p.persist = p.var != 1 && p.items > cus && (mode < 2 || mode >= 4);   // (4, 5: fp16 epilogues too)
  p.ksplit = k / p.slabs;
  p.d = {p.persist ? cus : p.items, 1, 1, kG8Threads, kG8Lds};
  return p;
}

namespace {

// Shapes the 256 x 256 tiles of enc_gemm_big.hip take (measured, tools/bench_gemm.py, same box): fp16-epilogue projections with
// N a multiple of 256 and K >= 512 at index-build row counts -- bge-base QKV 32768 x 2304 x 768: 457 -> 686 TFLOP/s, FFN-up
// 32768 x 3072 x 768: 507 -> 659 (both were on the row-streaming kernel); 4096^3: 742 -> 970.  NOT taken: the fp32 +
// residual epilogue at N = 768 (three column blocks = 384 workgroups = one and a half waves of the chip: 582 against
// 667 for the 128 x 128 kernel's 1536 workgroups), and MiniLM's K = 384 shapes (six k-steps: the row-streaming kernel's
// resident weights win, 733 / 541 against 419 / 439 with 256 x 128 tiles).  CRS_GEMM_BIG=0 disables it (A/B runs).
// It is taken from 128 workgroups on (CRS_GEMM_BIG_MIN_WGS): at 4096 tokens of bge-base (C3's query batch) 144 / 192
// workgroups of 256 x 256 beat the row-streaming kernel's 144 (QKV 42.0 -> 35.9 us, FFN-up 57.4 -> 41.5); at 2048 tokens
// (72 / 96 workgroups) they lose (25.7 -> 31.5, 33.1 -> 36.6).
bool gemm_big_applies(int m, int n, int k, int mode, const EncKnobs& kn) {
  if (!kn.gemm_big || mode == 2 || k % 64 != 0 || k < 512 || n % kBigN != 0) return false;
  return (long)(n / kBigN) * cdiv(m, kBigM) >= kn.gemm_big_min_wgs;
}

GemmPlan plan_stream(int m, int n, int k, int mode, int cus) {
  GemmPlan p;
  const bool ks = k == 768;   // the K-split form: one workgroup per CU; else 2 workgroups / CU resident
  p.family = ks ? GemmFamily::StreamKS : GemmFamily::Stream;
  p.m = m, p.n = n, p.k = k, p.mode = mode;
  p.colblocks = cdiv(n, kStreamN);
  const int n_tiles = cdiv(m, kStreamRows);
  int streams = (ks ? cus : cus * 2) / p.colblocks;   // column blocks of a stream run together
  if (streams < 1) streams = 1;
  if (streams > n_tiles) streams = n_tiles;
  if (streams >= 8) streams &= ~7;                    // whole rounds over the 8 XCDs
  p.streams = streams;
  p.d = {p.colblocks * streams, 1, 1, ks ? kStreamKsThreads : kStreamThreads, ks ? stream_ks_lds(k) : stream_lds(k)};
  return p;
}

}  // namespace

AttnPlan plan_attention(int batch, int seq, int heads, int hd, bool bias, const EncKnobs& kn) {
  AttnPlan a;
  a.hd = hd;
  a.form = AttnForm::Blocked, a.bias = bias, a.d = {cdiv(seq, kAttnQ), heads, batch, kAttnThreads, 0};
  if (bias) return a;   // the blocked kernel at every sequence length: the short and whole-sequence kernels carry no bias
  if (kn.attn_short && seq <= 16 && (hd == 32 || hd == 64)) {
    a.form = AttnForm::Short, a.d = {cdiv(heads * batch, 4), 1, 1, 256, 0};
    return a;
  }
  // whole sequence per workgroup when it is long enough to matter and short enough for LDS
  if (!kn.attn_seq || seq <= 64 || seq > 512 || (seq > 256 && hd != 64)) return a;
  a.smax = seq <= 256 ? 256 : 512, a.nw = a.smax / 64;
  a.form = (kn.attn_x32 && hd != 16) ? AttnForm::Seq32 : AttnForm::Seq;
  // four query tiles per wave (CRS_ATTN_QT=4) exist for <32, 256> and <64, 512>
  a.qt = a.form == AttnForm::Seq32 ? ((kn.attn_qt4 && ((hd == 32 && a.smax == 256) || (hd == 64 && a.smax == 512))) ? 4 : 2) : 0;
  a.d = {heads * batch, 1, 1, a.nw * 64, a.form == AttnForm::Seq32 ? attn_seq32_lds(hd, a.smax) : attn_seq_lds(hd, a.smax)};
  return a;
}

AttnPlan plan_attention_window(int batch, int seq, int heads, int hd, int window, const EncKnobs& kn) {
  (void)kn;
  AttnPlan a;
  a.hd = hd, a.form = AttnForm::Window, a.window = window;
  a.d = {cdiv(seq, kAttnQ), heads, batch, kAttnThreads, 0};
  return a;
}

bool qkv_attn_supported(int hidden, int heads, int seq) {
  if (hidden > 384 || hidden % 128) return false;
  const int hd = hidden / heads;
  if (hd != 32 && hd != 64) return false;
  if (qa_lds(hidden, hd) > kMaxLds) return false;
  return seq == 16 || seq == 32 || seq == 64;
}

AttnPlan plan_qkv_attn(int tokens, int hidden, int heads) {
  AttnPlan a;
  a.form = AttnForm::Fused, a.hd = hidden / heads;
  a.d = {cdiv(tokens, kQaTokens), heads, 1, kQaThreads, qa_lds(hidden, a.hd)};
  return a;
}

Dims plan_rope(int tokens, int hidden) {
  return {(int)((rope_items(tokens, hidden) + kRopeThreads - 1) / kRopeThreads), 1, 1, kRopeThreads, 0};
}

Dims plan_rows(int tokens) { return {cdiv(tokens, kRowTokens), 1, 1, kRowThreads, 0}; }
Dims plan_pool(int batch) { return {batch, 1, 1, 256, 0}; }
Dims plan_pair_head(int batch, int hidden) { return {cdiv(batch, kPairGroup), 1, 1, kPairThreads, kPairGroup * hidden * 4}; }

ProjLnPlan plan_proj_ln(int tokens, int hidden, int k, bool big_ln, int small_lds, int cus, const EncKnobs& kn) {
  ProjLnPlan p;
  p.ln = plan_rows(tokens);
  if (big_ln && rowln2_supported(hidden, k)) {   // (a pre-norm plan passes big_ln = false)
    // index-build side (large token counts), hidden = 384: projection + bias + residual + LayerNorm in one pipelined kernel
    p.rowln2 = true, p.variant = kn.rowln2_variant, p.d = {cdiv(tokens, kRowlnRows), 1, 1, kRowlnThreads, kRowlnLds};
  } else if (use_panel(tokens, k, kn)) {
    p.gemm = plan_gemm_panel(tokens, hidden, k, 3, small_lds, kn);
  } else if (const int s8 = gemm8_splitk(tokens, hidden, k, kn)) {
    p.gemm = plan_gemm8(tokens, hidden, k, 3, s8, cus, kn);
  } else {
    p.gemm = plan_gemm(tokens, hidden, k, 2, small_lds, cus, kn);
  }
  return p;
}

GemmPlan plan_gemm_panel(int m, int n, int k, int mode, int small_lds, const EncKnobs& kn) {
  GemmPlan p;
  int kc = panel_chunk(k);
  if (kc == 0 || (mode != 0 && mode != 1 && mode != 3 && mode != 4 && mode != 5)) return p;
  p.family = GemmFamily::Panel;
  p.m = m, p.n = n, p.k = k, p.mode = mode;
  p.slabs = mode == 3 ? panel_splits(k, m, kn) : 1;
  int kin = k / kc / p.slabs;
  const int nb = cdiv(n, kPanelN);
  // 128-row tiles once 64-row tiles would need more than one wave of workgroups on the chip
  // (forcing 64- or 128-row tiles everywhere measured within 2 % either way on both models' query chains)
  p.tm = ((long)nb * cdiv(m, 64) * p.slabs > kPanelWave && m > 64) ? 128 : 64;
  // small_lds (crs_encoder_desc.flags & CRS_ENC_SMALL_LDS): stage the K range in 128-column chunks (<= 48 KB of LDS: the
  // forward can then run beside a scan's resident workgroups).  CRS_PANEL_KC=128|256|384 forces a chunk size (A/B runs).
  const int kc_cap = kn.panel_kc ? kn.panel_kc : (small_lds ? 128 : 0);
  // A launch of more workgroups than CUs stages 128 columns at a time: 48 KB of LDS, up to three workgroups resident
  // per CU, one workgroup's transfers under another's MFMAs (bge-base at query-batch sizes: QKV 288, FFN-up 384, FFN-down
  // 768 workgroups).  Measured on the bge-base query chain (tools/enc_chain_profile.py): 64 x 16 tokens 945 -> ~800 us per
  // forward, 16 x 16: 793 -> 584, 256 x 16: 2222 -> 2000.  A single wave of workgroups keeps the one-shot fetch (MiniLM:
  // every launch <= 192 workgroups; 237 us one-shot against 244-253 in 128-column pieces).
  const long wgs = (long)nb * cdiv(m, p.tm) * p.slabs;
  if (kc_cap && kc > kc_cap && kc % kc_cap == 0) { kin *= kc / kc_cap; kc = kc_cap; }
  else if (!kc_cap && wgs > kPanelWave && kc > 128 && kc % 128 == 0) { kin *= kc / 128; kc = 128; }
  p.kc = kc, p.kin = kin;
  p.d = {nb, cdiv(m, p.tm), p.slabs, kPanelThreads, panel_lds(p.tm, kc, mode)};
  return p;
}

GemmPlan plan_gemm(int m, int n, int k, int mode, int small_lds, int cus, const EncKnobs& kn) {
  (void)small_lds;   // none of these families has a small-LDS form
  GemmPlan p;
  if (mode == 4 || mode == 5) {
    // the gated epilogue (4: SiLU, 5: GELU on the activated half) exists on the 256 x 256 phase-scheduled kernel, the tiled kernel (and the panel kernel, plan_gemm_panel):
    // every gated plan made here is Gemm8 or Tiled, whatever the shape and the knobs, so the 256-row and row-streaming
    // families never see the mode
    if (gemm8_applies(m, n, k, kn)) return plan_gemm8(m, n, k, mode, 1, cus, kn);
    p.m = m, p.n = n, p.k = k, p.mode = mode, p.family = GemmFamily::Tiled;
    p.d = {cdiv(n, kTiledN) * cdiv(m, kTiledM), 1, 1, kTiledThreads, 0};
    return p;
  }
  if (mode < 0 || mode > 2) return p;
  if (gemm8_applies(m, n, k, kn)) return plan_gemm8(m, n, k, mode, 1, cus, kn);
  p.m = m, p.n = n, p.k = k, p.mode = mode;
  if (gemm_big_applies(m, n, k, mode, kn)) {
    p.family = GemmFamily::Big;
    p.d = {(n / kBigN) * cdiv(m, kBigM), 1, 1, kBigThreads, big_lds(kBigN)};
    return p;
  }
  // short contraction, many rows, wide output (the index-build side's QKV and FFN-up projections): the tiled kernel
  // spends as long in its prologue and epilogue as in its K / 64 steps; stream rows past resident W
  if (m >= 512 && n >= 512 && mode != 2 && stream_k(k) && kn.gemm_stream) return plan_stream(m, n, k, mode, cus);
  p.family = GemmFamily::Tiled;
  p.d = {cdiv(n, kTiledN) * cdiv(m, kTiledM), 1, 1, kTiledThreads, 0};
  return p;
}

EncPlan make_enc_plan(int hidden, int heads, int ffn, int flags, int batch, int seq, int rel_bias, int pair, int cus, const EncKnobs& kn,
                      int window) {
  EncPlan p{};
  const int T = batch * seq, H = hidden, F = ffn, hd = H / heads, small = (flags & 1) ? 1 : 0;   // CRS_ENC_SMALL_LDS
  p.hidden = H, p.heads = heads, p.ffn = F, p.batch = batch, p.seq = seq, p.tokens = T;
  p.typed = pair == 1, p.pair = pair;
  p.rotary = (flags & 2) != 0, p.gated = (flags & (4 | 16)) != 0;   // CRS_ENC_ROTARY, CRS_ENC_GATED_SILU / CRS_ENC_GATED_GELU
  p.prenorm = (flags & 8) != 0;                                      // CRS_ENC_PRENORM
  const int gate_mode = (flags & 16) ? 5 : 4;
  p.embed = plan_rows(T);
  p.tail = pair ? plan_pair_head(batch, H) : plan_pool(batch);
  // fp16-epilogue projections (QKV, FFN-up) on the panel kernel: K = H in one chunk, or (CRS_ENC_PANEL_MULTI != 0) walked in
  // chunks by the workgroup -- bge-base at query-batch sizes, where the row-streaming kernel pays a 196 KB weight prologue
  // per workgroup for a handful of tiles
  // (the phase-scheduled 256 x 256 kernel takes QKV / FFN-up as soon as it has a chip's worth of tiles: bge-base from 4096 tokens)
  const bool single_h = T <= kPanelMaxTokens && panel_chunk(H) != 0 && (panel_chunk(H) == H || kn.panel_multi) &&
                        !gemm8_applies(T, 3 * H, H, kn);
  // short sequences in the launch-bound regime: QKV projection + attention as one kernel (enc_qkvattn.hip)
  // (never for a rotary model: the rotation runs between the projection and attention)
  if (!rel_bias && !p.rotary && !p.prenorm && T <= kPanelMaxTokens && !small && kn.qkvattn && qkv_attn_supported(H, heads, seq)) {
    p.attn = plan_qkv_attn(T, H, heads);
  } else {
    p.qkv = single_h ? plan_gemm_panel(T, 3 * H, H, 0, small, kn) : plan_gemm(T, 3 * H, H, 0, small, cus, kn);
    p.attn = plan_attention(batch, seq, heads, hd, rel_bias != 0, kn);
  }
  if (p.rotary) p.rope = plan_rope(T, H);
  if (p.prenorm) p.win = plan_attention_window(batch, seq, heads, hd, window, kn);
  // pre-norm: the norm does not follow the projection's residual add in the same stream position (it belongs to the NEXT block), so
  // the fused projection + LayerNorm kernel is never taken: mode-3 slabs or the mode-2 GEMM, then add_layernorm
  const bool big_ln = T > kPanelMaxTokens && kn.bigln && !p.prenorm;
  p.out = plan_proj_ln(T, H, H, big_ln, small, cus, kn);
  // gated: W holds 2 F interleaved gate / up rows and the epilogue (mode 4) leaves F columns; ffn_off is T x F either way
  if (p.gated) p.up = single_h ? plan_gemm_panel(T, 2 * F, H, gate_mode, small, kn) : plan_gemm(T, 2 * F, H, gate_mode, small, cus, kn);
  else p.up = single_h ? plan_gemm_panel(T, F, H, 1, small, kn) : plan_gemm(T, F, H, 1, small, cus, kn);
  p.down = plan_proj_ln(T, H, F, big_ln, small, cus, kn);
  p.out.prenorm = p.down.prenorm = p.prenorm;

  // The workspace's slab count: an UPPER BOUND of the slab counts above (out.gemm.slabs, down.gemm.slabs), kept as the rule
  // crs_encoder_workspace_bytes has always answered by.  It takes the gemm8 split-K count of a shape even where the panel path
  // is taken first: bge-base at 2048 tokens (hidden 768, ffn 3072) sizes y32 for 6 slabs, gemm8_splitk(2048, 768, 3072), while
  // the forward writes the panel's 2.
  const size_t t = (size_t)T, h = H, f = F;
  int split = 1;
  if (use_panel(T, F, kn)) split = panel_splits(F, T, kn);
  if (use_panel(T, H, kn) && panel_splits(H, T, kn) > split) split = panel_splits(H, T, kn);
  if (gemm8_splitk(T, H, F, kn) > split) split = gemm8_splitk(T, H, F, kn);
  if (gemm8_splitk(T, H, H, kn) > split) split = gemm8_splitk(T, H, H, kn);
  p.max_split = split;
  size_t off = 0;
  p.x32 = off; off += up256(t * h * 4);
  p.y32 = off; off += up256(t * h * 4 * split);
  p.x16 = off; off += up256(t * h * 2);
  p.ctx = off; off += up256(t * h * 2);
  p.qkv_off = off; off += up256(t * 3 * h * 2);
  p.ffn_off = off; off += up256(t * f * 2);
  p.total = off;
  return p;
}

namespace {

struct Text {
  char* buf; size_t cap; int len = 0;
  Text(char* b, size_t c) : buf(b), cap(c) { if (buf && cap) buf[0] = '\0'; }   // a plan without launches is the empty text
  void line(const Dims& d, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    len += vsnprintf(rest(), room(), fmt, ap);
    va_end(ap);
    len += snprintf(rest(), room(), " grid=%dx%dx%d wg=%dx1x1 lds=%d\n", d.gx, d.gy, d.gz, d.threads, d.lds);
  }
  char* rest() const { return (size_t)len < cap ? buf + len : nullptr; }
  size_t room() const { return (size_t)len < cap ? cap - len : 0; }
};

void gemm_line(Text& t, const GemmPlan& g) {
  switch (g.family) {
    case GemmFamily::None: break;
    case GemmFamily::Tiled: t.line(g.d, "gemm_f16_kernel<%d>", g.mode); break;
    case GemmFamily::Panel: t.line(g.d, "gemm_panel_kernel<%d, %d>", g.mode, g.tm); break;
    case GemmFamily::Stream: t.line(g.d, "gemm_stream_kernel<%d, %d>", g.k, g.mode); break;
    case GemmFamily::StreamKS: t.line(g.d, "gemm_stream_ks_kernel<%d, %d>", g.k, g.mode); break;
    case GemmFamily::Big: t.line(g.d, "gemm_big_kernel<%d, %d>", g.mode, kBigN); break;
    case GemmFamily::Gemm8:
    case GemmFamily::Gemm8SplitK: t.line(g.d, "gemm8_kernel<%d, %s, %d>", g.mode, g.persist ? "true" : "false", g.var); break;
  }
}

void attn_line(Text& t, const AttnPlan& a) {
  switch (a.form) {
    case AttnForm::Fused: t.line(a.d, "qkv_attn_kernel<%d>", a.hd); break;
    case AttnForm::Blocked: t.line(a.d, "attention_kernel<%d, %s>", a.hd, a.bias ? "true" : "false"); break;
    case AttnForm::Short: t.line(a.d, "attention_short_kernel<%d>", a.hd); break;
    case AttnForm::Seq: t.line(a.d, "attention_seq_kernel<%d, %d, %d>", a.hd, a.smax, a.nw); break;
    case AttnForm::Seq32: t.line(a.d, "attention_seq32_kernel<%d, %d, %d, %d>", a.hd, a.smax, a.nw, a.qt); break;
    case AttnForm::Window: t.line(a.d, "attention_window_kernel<%d>", a.hd); break;   // (window is a launch argument)
  }
}

// the row kernels' lines: enc_plan_describe, proj_ln_plan_describe and row_plan_describe print them through these
void embed_line(Text& t, const Dims& d, int hidden, bool typed) {
  t.line(d, "embed_ln%s_kernel<%d, %s>", row_form2(hidden) ? "2" : "", row_form(hidden), typed ? "true" : "false");
}

void ln_line(Text& t, const Dims& d, int hidden, int slabs) {
  t.line(d, "layernorm%s_kernel<%d, %d>", row_form2(hidden) ? "2" : "", row_form(hidden), slabs);
}

void add_ln_line(Text& t, const Dims& d, int hidden, int slabs) {
  t.line(d, "add_layernorm%s_kernel<%d, %d>", row_form2(hidden) ? "2" : "", row_form(hidden), slabs);
}

void tail_line(Text& t, const Dims& d, int hidden, bool pair) {
  if (pair) t.line(d, "pair_head_kernel<%d>", hidden % 128 == 0 ? 2 : 1);
  else t.line(d, "pool_kernel");
}

void proj_ln_lines(Text& t, const ProjLnPlan& s, int hidden) {
  if (s.rowln2) { t.line(s.d, s.variant ? "gemm_rowln2_kernel<64, 2>" : "gemm_rowln2_kernel<32, 4>"); return; }
  gemm_line(t, s.gemm);
  if (s.prenorm) add_ln_line(t, s.ln, hidden, s.gemm.slabs); else ln_line(t, s.ln, hidden, s.gemm.slabs);
}

}  // namespace

int gemm_plan_describe(const GemmPlan& p, char* buf, size_t cap) {
  Text t{buf, cap};
  gemm_line(t, p);
  return t.len;
}

int proj_ln_plan_describe(const ProjLnPlan& p, int hidden, char* buf, size_t cap) {
  Text t{buf, cap};
  proj_ln_lines(t, p, hidden);
  return t.len;
}

int attn_plan_describe(const AttnPlan& p, char* buf, size_t cap) {
  Text t{buf, cap};
  attn_line(t, p);
  return t.len;
}

EncKnobs attn_route_knobs(int route) {
  EncKnobs k;
  if (route & 1) k.attn_seq = false;
  if (route & 2) k.attn_short = false;
  if (route & 4) k.attn_x32 = false;
  if (route & 8) k.attn_qt4 = true;
  return k;
}

int enc_plan_describe(const EncPlan& p, char* buf, size_t cap) {
  Text t{buf, cap};
  embed_line(t, p.embed, p.hidden, p.typed);
  gemm_line(t, p.qkv);
  if (p.rotary) t.line(p.rope, "rope_qk_kernel<%d>", p.attn.hd);
  attn_line(t, p.attn);
  if (p.prenorm) attn_line(t, p.win);   // the sliding layers run this one in place of the line above
  proj_ln_lines(t, p.out, p.hidden);
  gemm_line(t, p.up);
  proj_ln_lines(t, p.down, p.hidden);
  tail_line(t, p.tail, p.hidden, p.pair != 0);
  return t.len;
}

int row_plan_describe(int kind, int rows, int hidden, int arg, char* buf, size_t cap) {
  Text t{buf, cap};
  switch (kind) {
    case kRowEmbed: embed_line(t, plan_rows(rows), hidden, arg != 0); break;
    case kRowLayerNorm: ln_line(t, plan_rows(rows), hidden, arg); break;
    case kRowPool: tail_line(t, plan_pool(rows), hidden, false); break;
    case kRowPairHead: tail_line(t, plan_pair_head(rows, hidden), hidden, true); break;
    case kRowAddLayerNorm: add_ln_line(t, plan_rows(rows), hidden, arg); break;
    default: break;
  }
  return t.len;
}

}  // namespace crs
