"""Case tables and reference bounds shared by the per-layer encoder tests (test_encoder_ref_cpu.py on the CPU,
test_encoder_layer_gpu.py / test_encoder_shapes_gpu.py / test_encoder_hard_gpu.py on the GPU).

Every GPU assertion of those files has the form

    max over valid tokens |gpu - fp64|  <=  2 * E_q + a

    E_q = max |emulated - fp64|   the quantisation floor: oracle/encoder_ref.py with emulate_fp16=True (fp64 arithmetic,
                                  fp16 round trips exactly where the kernels store fp16) against the plain fp64 model
    a   = 4 * max |fp32 - fp64|   accumulation order: the plain fp32 oracle's own distance from fp64 on the same case,
                                  times 4 because the GPU's summation order differs from torch's as torch's from fp64's

all three computed here, from the reference alone, for the exact inputs of the case.  The factor 2 is the triangle
inequality (GPU to its numerics model, model to truth); it is not a tuning knob.  A case is ADMISSIBLE only if its E_q on
the hidden state is <= COND_CAP = 3e-2 / 2, i.e. the bound is never looser than the 3e-2 of test_encoder_gpu.py;
test_encoder_ref_cpu.py enforces that for every case below, without a GPU.

The `why` of a case names the branch of the planner (csrc/enc_plan.cpp: make_enc_plan, plan_gemm) it is in the table for.
tests/test_enc_plan_cpu.py checks, without a GPU, that the planner gives every case the kernels it launched on an MI355X
(tests/golden/enc_plans.json.xz; profiles/enc_cases_kernels.txt is that list in words) and that every (step, kernel family) pair
the planner can produce is reached by a case: a moved threshold that changes what a case exercises fails there.
"""
from __future__ import annotations

from dataclasses import dataclass, field, replace
from typing import Dict, Tuple

import numpy as np
import torch

from oracle import encoder_ref as er

COND_CAP = 3e-2 / 2
ACC_MARGIN = 4.0


@dataclass(frozen=True)
class Case:
    name: str
    cfg: er.EncoderConfig           # already truncated to the layers the case runs
    batch: int
    seq: int
    seed: int
    why: str                        # the branch this case is in the table for
    lens: Tuple[int, ...] | str = "ragged"      # "full", "ragged" (synth_tokens), "ragged1" (random, one row of 1 token) or explicit
    wkw: Tuple[Tuple[str, float], ...] = ()     # make_weights variants
    query_batch: bool = False       # run again with CRS_ENC_SMALL_LDS

    @property
    def tokens(self) -> int:
        return self.batch * self.seq


def _small(hidden, heads, ffn, layers=1, max_pos=512):
    return er.EncoderConfig(vocab_size=1000, hidden=hidden, layers=layers, heads=heads, ffn=ffn, max_pos=max_pos,
                            max_seq=max_pos)


def _first(cfg, n):
    return er.truncate_layers(cfg, None, n)[0]


TINY1, MINI1, BGE1 = _first(er.TINY, 1), _first(er.MINILM_L6, 1), _first(er.BGE_BASE, 1)
TINY2, MINI2, BGE2 = _first(er.TINY, 2), _first(er.MINILM_L6, 2), _first(er.BGE_BASE, 2)

# ---------------------------------------------------------------------------------------------------------------------
# B1: one layer of the three real configurations at every token regime that selects different kernels for the same math
LAYER_CASES = [
    # query batches.  MiniLM: embed_ln2<3>, qkv_attn<32>, panel mode 3 (1 slab for K = 384, 4 for K = 1536) + layernorm2<3, NS>,
    # panel mode 1.  bge: embed_ln2<6>, multi-chunk panel modes 0 / 1 / 3 (2 and 4 slabs), attention_short<64> (seq 16) or the
    # blocked attention_kernel<64>.  TINY (hidden 64: no panel chunk for K = 64; FFN-down, K = 256, is a 1-slab panel): tiled gemm modes 0 / 1 / 2, attention_kernel<16>, <1, 1> LN forms
    Case("tiny-8x16", TINY1, 8, 16, 101, "tiled gemm, attention_kernel<16>, embed_ln<1>, layernorm<1,1>", "full", query_batch=True),
    Case("tiny-5x32r", TINY1, 5, 32, 102, "the same with ragged rows and a 1-token row", "ragged1", query_batch=True),
    Case("tiny-3x64r", TINY1, 3, 64, 103, "one whole 64-key block, ragged", "ragged1", query_batch=True),
    Case("minilm-8x16", MINI1, 8, 16, 111, "qkv_attn<32> seq 16 (4 sequences per token block), panel 1 / 4 slabs", "full", query_batch=True),
    Case("minilm-7x16r", MINI1, 7, 16, 112, "qkv_attn<32>: token block tail (112 tokens), 1-token row", "ragged1", query_batch=True),
    Case("minilm-5x32r", MINI1, 5, 32, 113, "qkv_attn<32> seq 32", "ragged1", query_batch=True),
    Case("minilm-3x64r", MINI1, 3, 64, 114, "qkv_attn<32> seq 64", "ragged1", query_batch=True),
    Case("minilm-4x64", MINI1, 4, 64, 115, "qkv_attn<32> seq 64, full rows", "full", query_batch=True),
    Case("bge-8x16", BGE1, 8, 16, 121, "attention_short<64>, multi-chunk panel, layernorm2<6, 2 / 4>", "full", query_batch=True),
    Case("bge-7x16r", BGE1, 7, 16, 122, "attention_short<64> with masked keys and a 1-token row", "ragged1", query_batch=True),
    Case("bge-5x32r", BGE1, 5, 32, 123, "blocked attention_kernel<64>, one key block", "ragged1", query_batch=True),
    Case("bge-3x64r", BGE1, 3, 64, 124, "blocked attention_kernel<64>, a whole key block", "ragged1", query_batch=True),
    # mid sizes: whole-sequence attention (16x16x32 form), panel GEMMs with 128-row tiles
    Case("minilm-3x150", MINI1, 3, 150, 131, "attention_seq32<32, 256>, 450 tokens", "ragged"),
    Case("minilm-4x256", MINI1, 4, 256, 132, "attention_seq32<32, 256> full length, 1024 tokens", "ragged"),
    Case("bge-3x150", BGE1, 3, 150, 133, "attention_seq32<64, 256>", "ragged"),
    Case("bge-4x256", BGE1, 4, 256, 134, "attention_seq32<64, 256>, 1024 tokens", "ragged"),
    # index build: > 4096 tokens with a ragged last 128-row block
    Case("tiny-79x64", TINY1, 79, 64, 141, "5056 tokens (39 x 128 + 64): tiled / stream gemm at K = 64 / 256", "ragged"),
    Case("minilm-29x160", MINI1, 29, 160, 142, "4640 tokens (36 x 128 + 32): gemm_stream + gemm_rowln2 K = 384 / 1536", "ragged"),
    Case("bge-19x250", BGE1, 19, 250, 143, "4750 tokens (37 x 128 + 14): stream / big / tiled gemm, attention_seq32<64, 256>", "ragged"),
    Case("bge-10x470", BGE1, 10, 470, 144, "4700 tokens: attention_seq32<64, 512>", "ragged"),
    # two layers: layer 2 consumes what layer 1 wrote in place (x32 aliases the residual)
    Case("tiny2-5x32r", TINY2, 5, 32, 151, "2 layers, tiled path", "ragged1", query_batch=True),
    Case("minilm2-7x16r", MINI2, 7, 16, 152, "2 layers, fused QKV + attention", "ragged1", query_batch=True),
    Case("minilm2-3x150", MINI2, 3, 150, 153, "2 layers, mid size", "ragged"),
    Case("minilm2-29x160", MINI2, 29, 160, 154, "2 layers, gemm_rowln2 in place", "ragged"),
    Case("bge2-7x16r", BGE2, 7, 16, 155, "2 layers, split-K panels", "ragged1", query_batch=True),
    Case("bge2-4x256", BGE2, 4, 256, 156, "2 layers, 1024 tokens", "ragged"),
]

# ---------------------------------------------------------------------------------------------------------------------
# B2: the model space check_desc accepts (hidden % 64 == 0 <= 1024, head_dim 16 / 32 / 64, ffn % 64 == 0)
H128_2, H128_4 = _small(128, 2, 512), _small(128, 4, 512)
H256_8, H256_4, H256_16 = _small(256, 8, 1024), _small(256, 4, 1024), _small(256, 16, 1024)
H320 = _small(320, 10, 1280)
H384_1088, H384_2304 = _small(384, 12, 1088), _small(384, 12, 2304)
H512, H512_3072, H512_1152 = _small(512, 8, 2048), _small(512, 8, 3072), _small(512, 8, 1152)
H512_16 = _small(512, 16, 2048)
H640 = _small(640, 10, 2560)
H768_6144 = _small(768, 12, 6144)
H1024, H1024_2 = _small(1024, 16, 4096), _small(1024, 16, 4096, layers=2)
H1024_6144, H1024_256 = _small(1024, 16, 6144), _small(1024, 16, 256)
MINI1_LONG = MINI1     # max_pos 512 allows seq 300 / 512

SHAPE_CASES = [
    Case("h128x2-6x32r", H128_2, 6, 32, 201, "qkv_attn_kernel<64> (only reachable at hidden 128, 2 heads); generic embed_ln<16> / layernorm<16, NS> with lanes 128.. masked", "ragged1", query_batch=True),
    Case("h128x2-8x16", H128_2, 8, 16, 202, "qkv_attn_kernel<64>, seq 16", "full", query_batch=True),
    Case("h128x4-3x64r", H128_4, 3, 64, 203, "qkv_attn_kernel<32> at hidden 128", "ragged1", query_batch=True),
    Case("h256x8-7x16r", H256_8, 7, 16, 204, "qkv_attn_kernel<32> at hidden 256; panel chunk 256", "ragged1", query_batch=True),
    Case("h256x4-5x32r", H256_4, 5, 32, 205, "hidden 256 / head_dim 64 exceeds the fused kernel's LDS check: panel QKV + attention_kernel<64>", "ragged1", query_batch=True),
    Case("h256x4-7x16r", H256_4, 7, 16, 206, "... and attention_short<64> at seq 16", "ragged1", query_batch=True),
    Case("h256x16-3x100", H256_16, 3, 100, 207, "attention_seq_kernel<16, 256, 4> (head_dim 16, seq > 64)", "ragged"),
    Case("h256x16-2x300", H256_16, 2, 300, 208, "blocked attention_kernel<16> over 5 key blocks (online rescale)", "ragged"),
    Case("h320-5x32r", H320, 5, 32, 209, "panel_chunk(320) == 0: every GEMM on the tiled kernel, N = 960 / 320 not multiples of 128; ffn 1280 = 5 chunks refused", "ragged1", query_batch=True),
    Case("h384f1088-5x32r", H384_1088, 5, 32, 210, "ffn 1088 = 64 mod 128: FFN-down on the tiled kernel, FFN-up panel with N = 17 x 64", "ragged1", query_batch=True),
    Case("h384f1088-29x160", H384_1088, 29, 160, 211, "gemm_rowln2 with K = 1088 (neither 384 nor 1536), 4640 tokens", "ragged"),
    Case("h384f2304-5x32r", H384_2304, 5, 32, 212, "ffn 2304 = 6 chunks -> 3 slabs: layernorm2<3, 3>", "ragged1", query_batch=True),
    Case("h512-5x32r", H512, 5, 32, 213, "hidden 512 / head_dim 64: 2 and 4 slabs on the generic layernorm<16, NS>", "ragged1", query_batch=True),
    Case("h512x16-8x12", H512_16, 8, 12, 214, "attention_short<32> (head_dim 32 outside the fused kernel: hidden 512)", "ragged1", query_batch=True),
    Case("h640-5x32r", H640, 5, 32, 215, "hidden 640 = 5 chunks of 128: use_panel refuses (5 slabs), tiled mode 2; multi-chunk panel modes 0 / 1 with kin = 5", "ragged1", query_batch=True),
    Case("h768f6144-5x32r", H768_6144, 5, 32, 216, "ffn 6144 = 16 chunks -> 4 slabs, 4 chunks walked per workgroup", "ragged1", query_batch=True),
    Case("h1024-5x32r", H1024, 5, 32, 217, "bge-large / BERT-large shape: 4 slabs both projections, generic LN forms at full width", "ragged1", query_batch=True),
    Case("h1024-8x16", H1024_2, 8, 16, 218, "the same, 2 layers, attention_short<64>", "full", query_batch=True),
    Case("h1024-18x250", H1024, 18, 250, 219, "hidden 1024 at 4500 tokens (35 x 128 + 20): index-build branches without gemm_rowln2", "ragged"),
    Case("minilm-2x300", MINI1_LONG, 2, 300, 220, "blocked attention_kernel<32> over 5 key blocks (256 < seq <= 512)", "ragged"),
    Case("minilm-2x512", MINI1_LONG, 2, 512, 221, "blocked attention_kernel<32> over 8 key blocks, 1024 tokens", "ragged"),
    # token counts on both sides of the dispatch thresholds, bge-base
    Case("bge-T1024", BGE1, 64, 16, 231, "1024 tokens: panel slab cap 4", "ragged", query_batch=True),
    Case("bge-T1025", BGE1, 25, 41, 232, "1025 tokens: panel slab cap 2", "ragged"),
    Case("bge-T2048", BGE1, 128, 16, 233, "2048 tokens: last split-K panel size (kSplitKMaxTokens)", "ragged", query_batch=True),
    Case("bge-T2049", BGE1, 683, 3, 234, "2049 tokens: multi-chunk K leaves the panel kernel for mode 2", "ragged"),
    Case("bge-T2304", BGE1, 9, 256, 235, "gemm8_splitk window (T % 256 == 0, >= 2048, < 128 tiles): 6 slabs for K = 3072, none for K = 768", "ragged"),
    Case("bge-T2432", BGE1, 19, 128, 236, "one 128-row block off the window: tiled mode 2", "ragged"),
    Case("bge-T4096", BGE1, 16, 256, 237, "4096 tokens: gemm8 for QKV / FFN-up, gemm8_splitk 3 slabs", "ragged"),
    Case("bge-T4097", BGE1, 17, 241, 238, "4097 tokens: past kPanelMaxTokens", "ragged"),
    Case("h512-9x256", H512, 9, 256, 239, "2304 tokens: gemm8_splitk 8 slabs (K = 2048) on the generic layernorm<16, 8>", "ragged"),
    Case("h512f3072-11x256", H512_3072, 11, 256, 240, "2816 tokens: gemm8_splitk 6 slabs (K = 3072) on layernorm<16, 6>", "ragged"),
    Case("h512f1152-5x32r", H512_1152, 5, 32, 241, "ffn 1152 = 3 chunks of 384: layernorm<16, 3>", "ragged1", query_batch=True),
    # forms that tests/test_enc_plan_cpu.py found no case for, each at the fewest tokens the planner gives them (256 CUs)
    Case("h1024f6144-11x256", H1024_6144, 11, 256, 242, "2816 tokens: persistent gemm8 for FFN-up (24 x 11 = 264 items > 256 CUs); QKV 12 x 11 = 132 tiles, one workgroup per item", "ragged"),
    Case("h1024f256-22x256", H1024_256, 22, 256, 243, "5632 tokens: persistent gemm8 for QKV (12 x 22 = 264 items)", "ragged"),
    Case("h1024f256-32x256", H1024_256, 32, 256, 244, "8192 tokens: out-projection and FFN-down (K = 256) on whole-K gemm8 mode 2 (4 x 32 = 128 tiles), layernorm<16, 1>", "ragged"),
]

# ---------------------------------------------------------------------------------------------------------------------
# B4: hard numeric regimes, 1-2 layers
PEAKED = (("qk_mult", 3.0),)
LN_HARD = (("dense_bias_offset", 0.5), ("ln_outliers", 4.0), ("ln_outlier_gain", 4.0))
GELU_WIDE = (("ffn_up_mult", 3.0),)
# last real key = first / last of a 16-, 32-, 64-key group
EDGE150 = (150, 1, 16, 17, 32, 33, 64, 65, 128, 129, 149)
EDGE300 = (300, 1, 64, 65, 128, 129, 256, 257, 288, 289)
EDGE64 = (64, 1, 16, 17, 32, 33, 48, 49, 63)
EDGE16 = (16, 1, 2, 4, 5, 8, 9, 15)

HARD_CASES = [
    # peaked attention (scores x 9) on every attention kernel form
    Case("peak-tiny-9x64", TINY1, 9, 64, 301, "attention_kernel<16>", EDGE64, PEAKED, True),
    Case("peak-minilm-8x16", MINI1, 8, 16, 302, "qkv_attn<32>", EDGE16, PEAKED, True),
    Case("peak-minilm-9x64", MINI1, 9, 64, 303, "qkv_attn<32> over 4 key tiles", EDGE64, PEAKED, True),
    Case("peak-h128x2-9x64", H128_2, 9, 64, 304, "qkv_attn<64>", EDGE64, PEAKED, True),
    Case("peak-bge-8x16", BGE1, 8, 16, 305, "attention_short<64>", EDGE16, PEAKED, True),
    Case("peak-h512x16-8x16", H512_16, 8, 16, 306, "attention_short<32>", EDGE16, PEAKED, True),
    Case("peak-minilm-9x48", MINI1, 9, 48, 307, "attention_kernel<32>, one block", (48, 1, 16, 17, 32, 33, 47, 48, 2), PEAKED, True),
    Case("peak-bge-9x64", BGE1, 9, 64, 308, "attention_kernel<64>", EDGE64, PEAKED, True),
    Case("peak-minilm-11x150", MINI1, 11, 150, 309, "attention_seq32<32, 256>", EDGE150, PEAKED),
    Case("peak-bge-11x150", BGE1, 11, 150, 310, "attention_seq32<64, 256>", EDGE150, PEAKED),
    Case("peak-bge-10x300", BGE1, 10, 300, 311, "attention_seq32<64, 512>", EDGE300, PEAKED),
    Case("peak-h256x16-11x150", H256_16, 11, 150, 312, "attention_seq_kernel<16, 256, 4>", EDGE150, PEAKED),
    Case("peak-minilm-10x300", MINI1, 10, 300, 313, "attention_kernel<32>, 5 key blocks, online rescale", EDGE300, PEAKED),
    Case("peak-h256x16-10x300", H256_16, 10, 300, 314, "attention_kernel<16>, 5 key blocks", EDGE300, PEAKED),
    # (2 layers at scores x 9 put E_q at 1.5e-2, over the conditioning cap: scores x 4 for the two-layer run)
    Case("peak-minilm2-10x300", MINI2, 10, 300, 315, "2 layers, blocked attention over 5 key blocks", EDGE300, (("qk_mult", 2.0),)),
    # LayerNorm inputs with a non-zero mean and a few wide channels, every slab count the dispatch can produce
    Case("ln-tiny-5x32r", TINY2, 5, 32, 321, "layernorm<1, 1>", "ragged1", LN_HARD, True),
    Case("ln-minilm-5x32r", MINI2, 5, 32, 322, "layernorm2<3, 1 / 4>", "ragged1", LN_HARD, True),
    # (bge-base and the 4640-token MiniLM run are over the conditioning cap at 2 layers in this regime: 1 layer)
    Case("ln-bge-5x32r", BGE1, 5, 32, 323, "layernorm2<6, 2 / 4>", "ragged1", LN_HARD, True),
    Case("ln-bge-T4096", BGE1, 16, 256, 324, "layernorm2<6, 3> after gemm8_splitk", "ragged", LN_HARD),
    Case("ln-bge-T2304", BGE1, 9, 256, 325, "layernorm2<6, 6> after gemm8_splitk", "ragged", LN_HARD),
    Case("ln-h384f2304-5x32r", H384_2304, 5, 32, 326, "layernorm2<3, 3>", "ragged1", LN_HARD, True),
    Case("ln-h512-5x32r", H512, 5, 32, 327, "layernorm<16, 2 / 4>", "ragged1", LN_HARD, True),
    Case("ln-h512f1152-5x32r", H512_1152, 5, 32, 328, "layernorm<16, 3>", "ragged1", LN_HARD, True),
    Case("ln-h512f3072-11x256", H512_3072, 11, 256, 329, "layernorm<16, 6>", "ragged", LN_HARD),
    Case("ln-h512-9x256", H512, 9, 256, 330, "layernorm<16, 8>", "ragged", LN_HARD),
    Case("ln-h1024-5x32r", H1024, 5, 32, 331, "layernorm<16, 4> at full width", "ragged1", LN_HARD, True),
    Case("ln-minilm-29x160", MINI1, 29, 160, 332, "gemm_rowln2's own LayerNorm", "ragged", LN_HARD),
    # GELU pre-activations out to |x| ~ 10 on every epilogue form
    Case("gelu-tiny-5x32r", TINY1, 5, 32, 341, "tiled mode 1", "ragged1", GELU_WIDE, True),
    Case("gelu-minilm-5x32r", MINI1, 5, 32, 342, "panel mode 1", "ragged1", GELU_WIDE, True),
    Case("gelu-bge-5x32r", BGE1, 5, 32, 343, "multi-chunk panel mode 1", "ragged1", GELU_WIDE, True),
    Case("gelu-minilm-29x160", MINI1, 29, 160, 344, "gemm_stream mode 1", "ragged", GELU_WIDE),
    Case("gelu-bge-T4096", BGE1, 16, 256, 345, "gemm8 mode 1", "ragged", GELU_WIDE),
    Case("gelu-bge-19x250", BGE1, 19, 250, 346, "gemm_big / stream mode 1 at K = 768", "ragged", GELU_WIDE),
]

ALL_CASES = LAYER_CASES + SHAPE_CASES + HARD_CASES
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------
def case_weights(case: Case) -> Dict[str, np.ndarray]:
    kw = dict(case.wkw)
    if "ln_outliers" in kw:
        kw["ln_outliers"] = int(kw["ln_outliers"])
    return er.make_weights(case.cfg, seed=case.seed, **kw)


def case_inputs(case: Case):
    """ids int32 [B, S], mask int32 [B, S], lens int32 [B]."""
    cfg = case.cfg
    if case.lens == "full":
        ids, mask = er.synth_tokens(cfg, case.batch, case.seq, seed=case.seed + 1, ragged=False)
    elif case.lens == "ragged":
        ids, mask = er.synth_tokens(cfg, case.batch, case.seq, seed=case.seed + 1, ragged=True)
    else:
        ids, _ = er.synth_tokens(cfg, case.batch, case.seq, seed=case.seed + 1, ragged=False)
        if case.lens == "ragged1":
            rng = np.random.default_rng(case.seed + 2)
            lens = rng.integers(1, case.seq + 1, size=case.batch)
            lens[0] = case.seq
            if case.batch > 1:
                lens[-1] = 1
        else:
            lens = np.asarray(case.lens)
            assert lens.shape == (case.batch,) and lens.min() >= 1 and lens.max() <= case.seq, case.name
        mask = (np.arange(case.seq)[None, :] < lens[:, None]).astype(np.int32)
        ids = (ids * mask).astype(np.int32)
    return ids, mask, mask.sum(1).astype(np.int32)


POOLED_MODES = (("mean", True), ("cls", True), ("mean", False), ("cls", False))


@dataclass
class Reference:
    h64: np.ndarray                 # fp64 hidden state [B, S, H]
    valid: np.ndarray               # bool [B, S]
    eq_hidden: float                # E_q on the hidden state
    acc_hidden: float               # max |fp32 - fp64| on the hidden state
    pooled64: Dict[Tuple[str, bool], np.ndarray] = field(default_factory=dict)
    eq_pooled: Dict[Tuple[str, bool], float] = field(default_factory=dict)
    acc_pooled: Dict[Tuple[str, bool], float] = field(default_factory=dict)
    h_emu: np.ndarray | None = None

    def bound_hidden(self) -> float:
        return 2.0 * self.eq_hidden + ACC_MARGIN * self.acc_hidden

    def bound_pooled(self, mode) -> float:
        return 2.0 * self.eq_pooled[mode] + ACC_MARGIN * self.acc_pooled[mode]


def pool(hidden: np.ndarray, mask: np.ndarray, pooling: str, normalize: bool) -> np.ndarray:
    """sentence-transformers Pooling + Normalize on a hidden state, in the hidden state's precision."""
    m = mask.astype(hidden.dtype)
    if pooling == "mean":
        p = (hidden * m[..., None]).sum(1) / np.maximum(m.sum(1, keepdims=True), 1e-9)
    else:
        p = hidden[:, 0]
    if normalize:
        p = p / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-12)
    return p


def reference(case: Case, weights=None, inputs=None, keep_emulated: bool = False) -> Reference:
    w = weights if weights is not None else case_weights(case)
    ids, mask, _ = inputs if inputs is not None else case_inputs(case)
    h64 = er.encode_ref(ids, mask, w, case.cfg, return_hidden=True, dtype=torch.float64)
    hem = er.encode_ref(ids, mask, w, case.cfg, return_hidden=True, dtype=torch.float64, emulate_fp16=True)
    h32 = er.encode_ref(ids, mask, w, case.cfg, return_hidden=True).astype(np.float64)
    valid = mask.astype(bool)
    ref = Reference(h64, valid, float(np.abs(hem - h64)[valid].max()), float(np.abs(h32 - h64)[valid].max()))
    for mode in POOLED_MODES:
        p64 = pool(h64, mask, *mode)
        ref.pooled64[mode] = p64
        ref.eq_pooled[mode] = float(np.abs(pool(hem, mask, *mode) - p64).max())
        ref.acc_pooled[mode] = float(np.abs(pool(h32, mask, *mode) - p64).max())
    if keep_emulated:
        ref.h_emu = hem
    return ref


_REF_CACHE: Dict[str, Reference] = {}


def cached_reference(case: Case) -> Reference:
    """Query-batch cases are visited twice (default forms, CRS_ENC_SMALL_LDS): keep their small references."""
    if case.name not in _REF_CACHE:
        r = reference(case)
        if case.tokens > 2048:
            return r
        _REF_CACHE[case.name] = r
    return _REF_CACHE[case.name]


# ---------------------------------------------------------------------------------------------------------------------
# GPU side (imported lazily: the CPU tests above never touch rag._encoder)
GUARD_BYTES = 1 << 20
GUARD_FILL = 0xA5


def hip_encoder(case: Case, cuda, weights=None):
    from rag._encoder import HipEncoder, ModelShape
    cfg = case.cfg
    w = weights if weights is not None else case_weights(case)
    shape = ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, cfg.pooling,
                       cfg.max_seq)
    return HipEncoder(shape, w, device=cuda)


def guarded_forward(enc, ids, lens, *, pooling: str, normalize: bool, return_hidden: bool = False, small_lds: bool = False):
    """One forward in a workspace of EXACTLY crs_encoder_workspace_bytes, with a poisoned guard region behind it that must
    come back untouched (the split-K slab count decides the layout: an off-by-one there writes past the end)."""
    b, s = ids.shape
    need = enc.workspace_bytes(b, s)
    buf = torch.empty(need + GUARD_BYTES, dtype=torch.uint8, device=enc.device)
    buf[need:].fill_(GUARD_FILL)
    enc.desc.pooling = 1 if pooling == "cls" else 0
    res = enc.forward(ids, lens, normalize=normalize, return_hidden=return_hidden, workspace=buf[:need], small_lds=small_lds)
    torch.cuda.synchronize()
    assert bool((buf[need:] == GUARD_FILL).all()), "the forward wrote past crs_encoder_workspace_bytes"
    if return_hidden:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy()


def check_case_on_gpu(case: Case, cuda, small_lds: bool = False, report=None):
    """Runs the case (hidden state + the four pooled outputs) and asserts max |gpu - fp64| <= 2 E_q + a on each.
    Returns {"hidden": array, ("mean", True): array, ...} for callers that compare two runs."""
    w = case_weights(case)
    inputs = case_inputs(case)
    ids, mask, lens = inputs
    ref = cached_reference(case) if case.query_batch else reference(case, w, inputs)
    enc = hip_encoder(case, cuda, w)
    got = {}
    lines, fails = [], []
    for mode in POOLED_MODES:
        if mode == POOLED_MODES[0]:
            got[mode], got["hidden"] = guarded_forward(enc, ids, lens, pooling=mode[0], normalize=mode[1], return_hidden=True,
                                                       small_lds=small_lds)
            err = float(np.abs(got["hidden"].astype(np.float64) - ref.h64)[ref.valid].max())
            assert np.isfinite(got["hidden"][ref.valid]).all()
            lines.append(("hidden", err, ref.eq_hidden, ref.bound_hidden()))
        else:
            got[mode] = guarded_forward(enc, ids, lens, pooling=mode[0], normalize=mode[1], small_lds=small_lds)
        err = float(np.abs(got[mode].astype(np.float64) - ref.pooled64[mode]).max())
        lines.append((f"{mode[0]}{'-norm' if mode[1] else '-raw'}", err, ref.eq_pooled[mode], ref.bound_pooled(mode)))
    for what, err, eq, bound in lines:
        msg = f"{case.name}{' small_lds' if small_lds else ''} {what}: max|gpu-fp64| {err:.3e}  E_q {eq:.3e}  ratio {err / eq:.3f}  bound {bound:.3e}"
        print(msg)
        if report is not None:
            report.append(msg)
        if not err <= bound:
            fails.append(msg)
    assert not fails, "\n".join(fails)
    # the assertions test_encoder_gpu.py makes on pooled output, kept as they are
    out, refn = got[("mean", True)], ref.pooled64[("mean", True)]
    cos = (out * refn).sum(1) / (np.linalg.norm(out, axis=1) * np.linalg.norm(refn, axis=1))
    assert (1.0 - cos).max() < 2e-4
    assert np.abs(out - refn).max() < 3e-3
    assert np.allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5)
    return got


def fused_qkv_attention_applies(case: Case) -> bool:
    """qkv_attn_supported and the token limit of make_enc_plan (csrc/enc_plan.cpp), restated: the one kernel the
    CRS_ENC_SMALL_LDS flag replaces by kernels of another accumulation order."""
    h, hd = case.cfg.hidden, case.cfg.head_dim
    if h > 384 or h % 128 or hd not in (32, 64) or case.seq not in (16, 32, 64) or case.tokens > 4096:
        return False
    lds = (64 + 3 * hd) * h * 2 + (2 * 64 * (hd + 8) + hd * 72) * 2 + 4 * 16 * 72 * 2
    return lds <= 160 * 1024


def check_small_lds_on_gpu(case: Case, cuda):
    """CRS_ENC_SMALL_LDS (include/crs_encoder.h): the same bound against fp64, and the distance to the default forward.
    The flag does two things.  It stages the panel GEMMs' K range in 128-column pieces: the MFMAs of a workgroup still
    run in the same order over the same K range into the same accumulators, so this changes no bit.  And it replaces the
    fused QKV + attention kernel by the QKV GEMM and an attention kernel of enc_attn.hip, whose softmax works in base 2
    and whose products run in another order: where the fused kernel would have run, the two forwards agree as two
    realisations of one numerics model do -- each within E_q of the model, hence within 2 E_q (+ a) of each other.
    Measured on an MI355X: bit-equal in all 32 cases outside the fused kernel, 0.13-1.25 E_q in the 17 inside."""
    small = check_case_on_gpu(case, cuda, small_lds=True)
    dflt = check_case_on_gpu(case, cuda)
    ref = cached_reference(case)
    d = float(np.abs(small["hidden"].astype(np.float64) - dflt["hidden"])[ref.valid].max())
    print(f"{case.name} small_lds vs default hidden: max diff {d:.3e} ({d / ref.eq_hidden:.3f} E_q), "
          f"bit-equal {np.array_equal(small['hidden'][ref.valid], dflt['hidden'][ref.valid])}")
    if not fused_qkv_attention_applies(case):
        assert np.array_equal(small["hidden"][ref.valid], dflt["hidden"][ref.valid])
        for mode in POOLED_MODES:
            assert np.array_equal(small[mode], dflt[mode])
        return
    assert d <= ref.bound_hidden()
    for mode in POOLED_MODES:
        assert np.abs(small[mode].astype(np.float64) - dflt[mode]).max() <= ref.bound_pooled(mode)
