"""Shared by tools/make_bertscore_golden.py (which writes tests/golden/bertscore.npz with transformers.BertModel /
RobertaModel in fp64) and the BERTScore tests: the cases, their seeded weights under the package's internal (BertModel)
tensor names, the token ids of both sides, and an fp64 restatement of the matching step."""
import os
from dataclasses import dataclass

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bertscore.npz")

# |P|, |R|, |F| of BertScorer.score_device against the fp64 golden.  The error comes from the encoder's fp16 GEMM operands
# (hidden states within 3e-2 absolute: tests/test_encoder_layer_gpu.py); the matching kernel's own error is below 2e-4
# (tests/test_bertscore_gpu.py).  Provable ceiling per case: 2 * 3e-2 * sqrt(H) / min|h| (e2e_ceiling below).
# The committed value is 4 x the largest error of the first GPU run (the margin of the cross-encoder test: padded widths
# select different attention forms).  Measured on an MI355X, max over the pairs of a case, |P| / |R| / |F| error:
#   tiny_4  4.6e-06 / 9.0e-06 / 6.7e-06      mid_3   1.46e-05 / 1.77e-05 / 1.60e-05     base_2  7.9e-06 / 9.2e-06 / 8.6e-06
#   rob_3   1.48e-05 / 1.40e-05 / 1.46e-05   wide_1  1.9e-06 / 1.4e-06 / 1.7e-06
# largest 1.773e-05 (mid_3, R) -> 4 x = 7.1e-05, a thousandth of the 0.060 ceiling.  The 200-pair batch of synthetic:tiny
# differed from the per-pair calls by 0.
E2E_TOL = 7.1e-5


@dataclass(frozen=True)
class BsCfg:
    name: str
    kind: str             # "bert" or "roberta"
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int          # rows of the position table
    ln_eps: float = 1e-12
    pad_id: int = 0
    cls_id: int = 1
    sep_id: int = 2
    pos_offset: int = 0   # first position id (RoBERTa: pad_id + 1)
    type_rows: int = 2


TINY = BsCfg("tiny", "bert", 1000, 64, 2, 4, 256, 64)
MID = BsCfg("mid", "bert", 2000, 384, 2, 12, 1536, 256)
BASE = BsCfg("base", "bert", 2000, 768, 2, 12, 3072, 512)
ROB = BsCfg("rob", "roberta", 1000, 128, 2, 4, 512, 66, ln_eps=1e-5, pad_id=1, cls_id=0, sep_id=2, pos_offset=2, type_rows=1)
WIDE = BsCfg("wide", "bert", 1000, 1024, 1, 16, 4096, 512)

# (key, config, seed, pairs, candidate width, reference width)
CASES = [("tiny_4", TINY, 201, 4, 24, 17), ("mid_3", MID, 202, 3, 80, 33), ("base_2", BASE, 203, 2, 150, 130),
         ("rob_3", ROB, 204, 3, 40, 21), ("wide_1", WIDE, 205, 1, 512, 512)]
LAYER_CHECK = ("mid_3", "base_2")         # cases whose layer-L and layer-(L - 1) scores are far apart (tiny's are not)


def weight_names(cfg: BsCfg):
    h, f = cfg.hidden, cfg.ffn
    out = [("embeddings.word_embeddings.weight", (cfg.vocab_size, h)), ("embeddings.position_embeddings.weight", (cfg.max_pos, h)),
           ("embeddings.token_type_embeddings.weight", (cfg.type_rows, h)),
           ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        out += [(p + "attention.self.query.weight", (h, h)), (p + "attention.self.query.bias", (h,)),
                (p + "attention.self.key.weight", (h, h)), (p + "attention.self.key.bias", (h,)),
                (p + "attention.self.value.weight", (h, h)), (p + "attention.self.value.bias", (h,)),
                (p + "attention.output.dense.weight", (h, h)), (p + "attention.output.dense.bias", (h,)),
                (p + "attention.output.LayerNorm.weight", (h,)), (p + "attention.output.LayerNorm.bias", (h,)),
                (p + "intermediate.dense.weight", (f, h)), (p + "intermediate.dense.bias", (f,)),
                (p + "output.dense.weight", (h, f)), (p + "output.dense.bias", (h,)),
                (p + "output.LayerNorm.weight", (h,)), (p + "output.LayerNorm.bias", (h,))]
    return out


def make_weights(cfg: BsCfg, seed: int):
    """One PCG64 stream per tensor: matrices ~N(0, 0.05), biases ~N(0, 0.02), LayerNorm gains 1 + N(0, 0.05)."""
    w = {}
    for idx, (name, shape) in enumerate(weight_names(cfg)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if name.endswith("LayerNorm.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith(".bias"):
            a = 0.02 * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = 0.05 * rng.standard_normal(shape, dtype=np.float32)
        w[name] = a.astype(np.float32)
    return w


def synth_pairs(cfg: BsCfg, pairs: int, seq_a: int, seq_b: int, seed: int):
    """cls ... sep, right-padded, ragged lengths (row 0 is full).  Half of a reference's tokens are drawn from its candidate,
    in another order, so the row and column maxima are neither trivial nor equal.
    -> (ids_a int32 [n, seq_a], mask_a int32, ids_b int32 [n, seq_b], mask_b int32)."""
    rng = np.random.default_rng(seed)

    def lens_of(seq):
        lens = np.full(pairs, seq, dtype=np.int64)
        if pairs > 1:
            lens[1:] = rng.integers(max(4, seq // 3), seq, size=pairs - 1)
        return lens

    la, lb = lens_of(seq_a), lens_of(seq_b)
    ids_a = np.full((pairs, seq_a), cfg.pad_id, dtype=np.int64)
    ids_b = np.full((pairs, seq_b), cfg.pad_id, dtype=np.int64)
    for p in range(pairs):
        body_a = rng.integers(4, cfg.vocab_size, size=la[p] - 2)
        body_b = rng.integers(4, cfg.vocab_size, size=lb[p] - 2)
        take = rng.random(lb[p] - 2) < 0.5
        body_b[take] = rng.choice(body_a, size=int(take.sum()))
        ids_a[p, :la[p]] = np.concatenate([[cfg.cls_id], body_a, [cfg.sep_id]])
        ids_b[p, :lb[p]] = np.concatenate([[cfg.cls_id], body_b, [cfg.sep_id]])
    mask_a = (np.arange(seq_a)[None, :] < la[:, None]).astype(np.int32)
    mask_b = (np.arange(seq_b)[None, :] < lb[:, None]).astype(np.int32)
    return ids_a.astype(np.int32), mask_a, ids_b.astype(np.int32), mask_b


def token_weights(mask: np.ndarray) -> np.ndarray:
    """The package's weights without idf: 1 on every real token, 0 on the two special tokens (first and last real one)."""
    w = mask.astype(np.float64).copy()
    lens = mask.sum(1)
    w[:, 0] = 0.0
    w[np.arange(mask.shape[0]), lens - 1] = 0.0
    return w


def match_ref(a, len_a, b, len_b, w_a=None, w_b=None):
    """Plain fp64 restatement of the matching step: normalise, matrix product, maxima over the real tokens, weighted means.
    a [n, Sa, H], b [n, Sb, H] (any float dtype), lens int [n], weights [n, S] or None (1 on real tokens) -> fp64 [n, 3].
    A zero row has cosine 0 to everything; a weight sum of 0 gives 0; F is 0 when P + R is 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.zeros((a.shape[0], 3))
    for p in range(a.shape[0]):
        la, lb = int(len_a[p]), int(len_b[p])
        if la == 0 or lb == 0:
            continue
        x, y = a[p, :la], b[p, :lb]
        nx, ny = np.linalg.norm(x, axis=1, keepdims=True), np.linalg.norm(y, axis=1, keepdims=True)
        x = np.divide(x, nx, out=np.zeros_like(x), where=nx > 0)
        y = np.divide(y, ny, out=np.zeros_like(y), where=ny > 0)
        sim = x @ y.T
        wa = np.ones(la) if w_a is None else np.asarray(w_a[p, :la], dtype=np.float64)
        wb = np.ones(lb) if w_b is None else np.asarray(w_b[p, :lb], dtype=np.float64)
        P = (wa * sim.max(1)).sum() / wa.sum() if wa.sum() > 0 else 0.0
        R = (wb * sim.max(0)).sum() / wb.sum() if wb.sum() > 0 else 0.0
        out[p] = P, R, (2 * P * R / (P + R) if P + R != 0 else 0.0)
    return out


def model_shape(cfg: BsCfg, layers: int = None):
    from rag._encoder import ModelShape
    return ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers if layers is None else layers, cfg.heads, cfg.ffn, cfg.max_pos,
                      cfg.ln_eps, "mean", min(512, cfg.max_pos - cfg.pos_offset), pos_offset=cfg.pos_offset)


def e2e_ceiling(hidden: int, min_norm: float) -> float:
    """A hidden state off by at most 3e-2 per element moves by at most 3e-2 sqrt(H) in norm, a unit vector by that over |h|,
    a cosine of two such vectors by twice that; maxima and weighted means move by no more than their arguments."""
    return 2 * 3e-2 * np.sqrt(hidden) / min_norm
