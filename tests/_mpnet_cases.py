"""Shared by tools/make_mpnet_golden.py (which writes tests/golden/encoder_mpnet.npz with transformers.MPNetModel in fp64)
and the MPNet tests: the cases, their seeded weights under the package's internal (BertModel) tensor names, token ids."""
import os
from dataclasses import dataclass

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_mpnet.npz")
REL_BIAS = "encoder.relative_attention_bias.weight"
PAD_ID, CLS_ID, SEP_ID = 1, 0, 2          # <pad>, <s>, </s>
BUCKETS, POS_OFFSET = 32, 2
HIDDEN_ROWS_CAP = 64                       # hidden states kept per case (a committed file stays under 1 MiB)


@dataclass(frozen=True)
class MPNetCfg:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int          # rows of the position table (positions 2 .. max_pos - 1 are used)
    max_seq: int
    ln_eps: float = 1e-5


TINY = MPNetCfg("tiny", 1000, 64, 2, 4, 256, 66, 64)               # head_dim 16 (synthetic:tiny-mpnet's shape)
MID = MPNetCfg("mid", 2000, 384, 2, 12, 1536, 258, 256)            # head_dim 32
BASE = MPNetCfg("base", 2000, 768, 2, 12, 3072, 514, 384)          # head_dim 64: two layers of all-mpnet-base-v2, small vocabulary

# (key, config, seed, batch, seq): 3 x 80 spans two key blocks with a ragged tail; >= 130 tokens reach the logarithmic
# buckets and the clamp at distance 128; 384 is all-mpnet-base-v2's own limit
CASES = [("tiny_4x24", TINY, 101, 4, 24), ("tiny_3x5", TINY, 102, 3, 5),
         ("mid_3x80", MID, 103, 3, 80), ("mid_2x150", MID, 104, 2, 150),
         ("base_2x16", BASE, 105, 2, 16), ("base_1x150", BASE, 106, 1, 150), ("base_2x384", BASE, 107, 2, 384)]


def weight_names(cfg: MPNetCfg):
    h, f = cfg.hidden, cfg.ffn
    out = [("embeddings.word_embeddings.weight", (cfg.vocab_size, h)), ("embeddings.position_embeddings.weight", (cfg.max_pos, h)),
           ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,)), (REL_BIAS, (BUCKETS, cfg.heads))]
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


def make_weights(cfg: MPNetCfg, seed: int):
    """One PCG64 stream per tensor: matrices ~N(0, 0.05), biases ~N(0, 0.02), LayerNorm gains 1 + N(0, 0.05), the relative
    bias table ~N(0, 0.5) (O(1) like a trained one, and asymmetric in +-offset: a transposed index shows).  No token types:
    a zero row stands in."""
    w = {}
    for idx, (name, shape) in enumerate(weight_names(cfg)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if name.endswith("LayerNorm.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith(".bias"):
            a = 0.02 * rng.standard_normal(shape, dtype=np.float32)
        elif name == REL_BIAS:
            a = 0.5 * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = 0.05 * rng.standard_normal(shape, dtype=np.float32)
        w[name] = a.astype(np.float32)
    w["embeddings.token_type_embeddings.weight"] = np.zeros((1, cfg.hidden), dtype=np.float32)
    return w


def synth_tokens(cfg: MPNetCfg, batch: int, seq: int, seed: int):
    """<s> ... </s>, right-padded with <pad>, ragged lengths (row 0 is full) -> (ids int32 [B, S], mask int32 [B, S])."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(4, cfg.vocab_size, size=(batch, seq), dtype=np.int64)
    lens = np.full(batch, seq, dtype=np.int64)
    if batch > 1:
        lens[1:] = rng.integers(max(2, seq // 3), seq, size=batch - 1)
    mask = np.arange(seq)[None, :] < lens[:, None]
    ids[:, 0] = CLS_ID
    ids[np.arange(batch), lens - 1] = SEP_ID
    ids[~mask] = PAD_ID
    return ids.astype(np.int32), mask.astype(np.int32)


def hidden_rows(mask: np.ndarray) -> np.ndarray:
    """Flat indices (into [B * S]) of the real tokens whose hidden states the golden file keeps: all of them in a small
    case, else the first and last two of every sequence plus an even spread."""
    real = np.flatnonzero(mask.reshape(-1))
    if real.size <= HIDDEN_ROWS_CAP:
        return real
    B, S = mask.shape
    lens = mask.sum(1)
    ends = [b * S + j for b in range(B) for j in (0, 1, lens[b] - 2, lens[b] - 1)]
    spread = real[np.linspace(0, real.size - 1, HIDDEN_ROWS_CAP - len(ends)).astype(np.int64)]
    return np.unique(np.concatenate([np.asarray(ends, dtype=np.int64), spread]))


def model_shape(cfg: MPNetCfg, pooling: str = "mean"):
    from rag._encoder import ModelShape
    return ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, pooling, cfg.max_seq,
                      rel_buckets=BUCKETS, pos_offset=POS_OFFSET)


def encode_ref(ids, mask, w, cfg: MPNetCfg, rel_table):
    """fp64 restatement of the forward the library runs for an MPNet shape: internal tensor names, position rows from
    POS_OFFSET on, rel_table [heads, 2 * span - 1] (rag._encoder.relative_bias_table) added to the scores at
    (key - query) + span - 1.  -> final hidden states [B, S, H] (numpy fp64)."""
    import math
    import torch
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in w.items()}
    ids_t, m = torch.from_numpy(np.asarray(ids)).long(), torch.from_numpy(np.asarray(mask)).double()
    B, S = ids_t.shape
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh

    def ln(x, name):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + cfg.ln_eps) * W[name + ".weight"] + W[name + ".bias"]

    x = ln(W["embeddings.word_embeddings.weight"][ids_t] + W["embeddings.position_embeddings.weight"][POS_OFFSET:POS_OFFSET + S][None]
           + W["embeddings.token_type_embeddings.weight"][0], "embeddings.LayerNorm")
    t = torch.from_numpy(np.asarray(rel_table)).double()
    span = (t.shape[1] + 1) // 2
    off = torch.arange(S)[None, :] - torch.arange(S)[:, None] + span - 1          # [query, key]
    bias = t[:, off]                                                              # [heads, S, S]
    neg = (1.0 - m)[:, None, None, :] * -1e30
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        lin = lambda v, name: v @ W[p + name + ".weight"].T + W[p + name + ".bias"]
        q, k, v = (lin(x, "attention.self." + n).view(B, S, nh, hd).transpose(1, 2) for n in ("query", "key", "value"))
        a = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(hd) + bias[None] + neg, dim=-1)
        ctx = (a @ v).transpose(1, 2).reshape(B, S, H)
        x = ln(lin(ctx, "attention.output.dense") + x, p + "attention.output.LayerNorm")
        hmid = lin(x, "intermediate.dense")
        x = ln(lin(0.5 * hmid * (1.0 + torch.erf(hmid / math.sqrt(2.0))), "output.dense") + x, p + "output.LayerNorm")
    return x.numpy()
