// enc_forms.h -- what the encoder's planner (enc_plan.cpp) and its launchers (enc_*.hip) must agree on, stated once: tile
// sizes, workgroup sizes, the dynamic-LDS formulas and the instantiation lists of the kernels.  Plain C++ (no HIP).
#pragma once

namespace crs {
namespace forms {

// enc_gemm.hip, tiled kernel: 128 x 128 output tiles, static LDS
constexpr int kTiledM = 128, kTiledN = 128, kTiledThreads = 256;

// enc_gemm.hip, panel kernel: TM (64 or 128) x 64 output tiles, the K range staged in chunks
constexpr int kPanelN = 64, kPanelThreads = 512;
constexpr int kPanelChunks[3] = {384, 256, 128};   // the chunk of a contraction is the first that divides K
constexpr int kPanelMaxChunk = 384;
constexpr int kPanelWave = 256;                    // workgroups of one wave of the chip, as the panel thresholds were measured
constexpr int panel_chunk(int k) {                 // 0: none
  for (int kc : kPanelChunks)
    if (k % kc == 0) return kc;
  return 0;
}
// staged A and W chunks; the epilogue's wave-private tiles (fp32 rows of 36 floats in modes 3 and 4, fp16 rows of 40 halves) re-use the buffer
constexpr int panel_lds(int tm, int kc, int mode) {
  const int stage = (tm + kPanelN) * kc * 2, ep = (mode >= 3 ? 36 * 4 : 40 * 2) * 32 * ((tm / 32) * (kPanelN / 32));
  return stage > ep ? stage : ep;
}

// enc_gemm8.hip: 256 x 256 x 64 tiles, two k-tile buffers of [A0 | A1 | W0 | W1] half tiles, eight staging tiles behind them
constexpr int kG8M = 256, kG8N = 256, kG8K = 64, kG8Threads = 512;
constexpr int kG8EpiRow16 = 144;
constexpr int kG8Lds = 2 * 4 * (128 * kG8K * 2) + 8 * 16 * kG8EpiRow16;   // 146 KB
constexpr int kG8SplitK[5] = {2, 3, 4, 6, 8};      // slab counts of the split-K form, tried in this order

// enc_gemm_big.hip: 256 x BN tiles, four LDS stages of depth 32
constexpr int kBigM = 256, kBigN = 256, kBigK = 32, kBigStages = 4, kBigThreads = 512;
constexpr int big_lds(int bn) { return kBigStages * (kBigM + bn) * kBigK * 2; }

// enc_gemm_stream.hip: 32-row A tiles streamed past W fragments resident in registers, 128 output columns per workgroup
constexpr int kStreamRows = 32, kStreamN = 128, kStreamThreads = 256, kStreamKsThreads = 512, kStreamEpiStride = 40;
constexpr bool stream_k(int k) { return k == 128 || k == 256 || k == 384 || k == 512 || k == 768; }   // 768: the K-split form, fp16 outputs only
constexpr int stream_lds(int k) { return 2 * kStreamRows * k * 2 + 4 * 32 * kStreamEpiStride * 2; }
constexpr int stream_ks_lds(int k) { return stream_lds(k) + 4 * 2 * 16 * 64 * 4; }

// enc_rowln.hip: projection + LayerNorm of 128-row blocks at hidden 384
constexpr int kRowlnRows = 128, kRowlnHidden = 384, kRowlnThreads = 512, kRowlnLds = 128 * 1024;
constexpr bool rowln2_supported(int hidden, int k) { return hidden == kRowlnHidden && k % 64 == 0 && k >= 192; }

// enc_misc.hip: slab counts the LayerNorm kernels are instantiated for; four tokens per 256-thread workgroup
#define CRS_LN_SLABS(X, A, B) X(A, B, 1) X(A, B, 2) X(A, B, 3) X(A, B, 4) X(A, B, 6) X(A, B, 8) X(A, B, 16)
constexpr bool ln_slabs_ok(int ns) {
#define CRS_LN_EQ(A, B, N) || A == N
  return false CRS_LN_SLABS(CRS_LN_EQ, ns, );
#undef CRS_LN_EQ
}
constexpr int kRowThreads = 256, kRowTokens = 4;
// per-lane width of the embedding / LayerNorm forms: exact counts for the hot shapes (the *2 kernels), else generic
constexpr int row_form(int hidden) { return hidden == 384 ? 3 : hidden == 768 ? 6 : hidden <= 64 ? 1 : 16; }
constexpr bool row_form2(int hidden) { return hidden == 384 || hidden == 768; }

// enc_attn.hip
constexpr int kAttnQ = 64, kAttnThreads = 256, kAttnMaxBiasSeq = 512;
constexpr int attn_seq_lds(int hd, int smax) { return (smax * (hd + 4) + hd * (smax + 4)) * 2; }     // 16x16x16 whole-sequence kernel
constexpr int attn_seq32_lds(int hd, int smax) { return (smax * (hd + 8) + hd * (smax + 8)) * 2; }   // 16x16x32 form

// enc_qkvattn.hip: 64 tokens x one head per workgroup
constexpr int kQaTokens = 64, kQaThreads = 512;
constexpr int qa_lds(int hidden, int hd) {
  return (kQaTokens + 3 * hd) * hidden * 2 + (2 * kQaTokens * (hd + 8) + hd * (kQaTokens + 8)) * 2 + 4 * 16 * (64 + 8) * 2;
}
constexpr int kMaxLds = 160 * 1024;

// enc_rope.hip: a thread rotates 8 column pairs (j, j + hd / 2) of one head of Q or K: hidden / 8 threads per token, no LDS
constexpr int kRopeThreads = 256;
constexpr long rope_items(long tokens, int hidden) { return tokens * (hidden / 8); }

// enc_pair.hip: 8 pairs per workgroup, their [CLS] rows in LDS
constexpr int kPairGroup = 8, kPairThreads = 256;

}  // namespace forms
}  // namespace crs
