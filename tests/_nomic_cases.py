"""Shared by tools/make_nomic_golden.py (which writes tests/golden/encoder_nomic.npz with transformers.NomicBertModel in fp64)
and the nomic-embed-text tests: the cases, their seeded weights under NomicBertModel's tensor names (the package's internal
names for this family), token ids, and the fp64 restatement of the forward."""
import json
import os
from dataclasses import dataclass

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_nomic.npz")
PAD_ID, CLS_ID, SEP_ID = 0, 101, 102          # BERT's uncased WordPiece vocabulary
THETA = 1000.0
HIDDEN_ROWS_CAP = 32                           # hidden states kept per case, as fp64 (a committed file stays under 1 MiB)


@dataclass(frozen=True)
class NomicCfg:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int
    max_seq: int
    ln_eps: float = 1e-12


TINY = NomicCfg("tiny", 1000, 64, 2, 4, 256, 128, 128)              # head_dim 16 (synthetic:tiny-nomic's shape)
MID = NomicCfg("mid", 2000, 384, 2, 12, 1536, 512, 256)             # head_dim 32
BASE = NomicCfg("base", 2000, 768, 2, 12, 3072, 2048, 1024)         # head_dim 64: two layers of nomic-embed-text, small vocabulary

# (key, config, seed, batch, seq): 3 x 80 spans two key blocks with a ragged tail; 2 x 600 has positions past BERT's 512 (and
# takes the blocked attention kernel: the whole-sequence kernels stop at 512)
CASES = [("tiny_4x24", TINY, 201, 4, 24), ("tiny_3x5", TINY, 202, 3, 5),
         ("mid_3x80", MID, 203, 3, 80), ("mid_2x150", MID, 204, 2, 150),
         ("base_2x16", BASE, 205, 2, 16), ("base_1x150", BASE, 206, 1, 150), ("base_2x600", BASE, 207, 2, 600)]


def weight_names(cfg: NomicCfg):
    h, f = cfg.hidden, cfg.ffn
    out = [("embeddings.word_embeddings.weight", (cfg.vocab_size, h)), ("embeddings.token_type_embeddings.weight", (2, h)),
           ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
    for i in range(cfg.layers):
        p = f"layers.{i}."
        out += [(p + "self_attn.q_proj.weight", (h, h)), (p + "self_attn.k_proj.weight", (h, h)),
                (p + "self_attn.v_proj.weight", (h, h)), (p + "self_attn.o_proj.weight", (h, h)),
                (p + "post_attention_layernorm.weight", (h,)), (p + "post_attention_layernorm.bias", (h,)),
                (p + "mlp.gate_proj.weight", (f, h)), (p + "mlp.up_proj.weight", (f, h)), (p + "mlp.down_proj.weight", (h, f)),
                (p + "post_mlp_layernorm.weight", (h,)), (p + "post_mlp_layernorm.bias", (h,))]
    return out


def make_weights(cfg: NomicCfg, seed: int):
    """One PCG64 stream per tensor: matrices ~N(0, 0.05), LayerNorm biases ~N(0, 0.02), gains 1 + N(0, 0.05).  No projection
    biases, as the published checkpoints."""
    w = {}
    for idx, (name, shape) in enumerate(weight_names(cfg)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if name.endswith("norm.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith(".bias"):
            a = 0.02 * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = 0.05 * rng.standard_normal(shape, dtype=np.float32)
        w[name] = a.astype(np.float32)
    return w


def synth_tokens(cfg: NomicCfg, batch: int, seq: int, seed: int):
    """[CLS] ... [SEP], right-padded with [PAD], ragged lengths (row 0 is full) -> (ids int32 [B, S], mask int32 [B, S])."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(103, cfg.vocab_size, size=(batch, seq), dtype=np.int64)
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


def model_shape(cfg: NomicCfg, pooling: str = "mean"):
    from rag._encoder import ModelShape
    return ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, pooling, cfg.max_seq,
                      rotary_theta=THETA, gated=True)


def rope_cos_sin(positions: int, hd: int, theta: float = THETA):
    """fp64 (cos, sin), each [positions, hd / 2]: the angles pos * theta^(-2 j / hd)."""
    inv = np.float64(theta) ** (-2.0 * np.arange(hd // 2, dtype=np.float64) / hd)
    ang = np.arange(positions, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang), np.sin(ang)


def rope_cos_sin_fp32(positions: int, hd: int, theta: float = THETA):
    """(cos, sin) as transformers' NomicBertRotaryEmbedding computes them whatever the model's dtype: the inverse frequencies,
    the angles and their cosines / sines in fp32 (the golden file was made with these; at position 600 an fp32 angle is off by
    up to 4e-5 from the exact one)."""
    import torch
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))
    ang = (inv[:, None] @ torch.arange(positions, dtype=torch.float)[None, :]).T
    return ang.cos().numpy(), ang.sin().numpy()


def encode_ref(ids, mask, w, cfg: NomicCfg, cos_sin=None):
    """fp64 restatement of the forward the library runs for a nomic shape (and of transformers.NomicBertModel):
        x     = LayerNorm(word[ids] + type[0])                              no position table
        q,k,v = x Wq^T, x Wk^T, x Wv^T                                      biases only where w carries them
        q,k   = t cos + rotate_half(t) sin per head, rotate_half(t) = (-t[hd/2:], t[:hd/2])
        x     = LayerNorm(x + softmax(q k^T / sqrt(hd) + padding mask) v Wo^T)
        x     = LayerNorm(x + (silu(x Wgate^T) * (x Wup^T)) Wdown^T)
    cos_sin: (cos, sin) [>= S, hd / 2] in place of the exact fp64 values (the identity (1, 0) switches the rotation off).
    -> final hidden states [B, S, H] (numpy fp64)."""
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

    def lin(v, name):
        y = v @ W[name + ".weight"].T
        return y + W[name + ".bias"] if name + ".bias" in W else y

    cos, sin = cos_sin if cos_sin is not None else rope_cos_sin(S, hd)
    cos = torch.from_numpy(np.asarray(cos, dtype=np.float64)[:S]).repeat(1, 2)[None, None]      # [1, 1, S, hd]
    sin = torch.from_numpy(np.asarray(sin, dtype=np.float64)[:S]).repeat(1, 2)[None, None]

    def rot(t):
        return t * cos + torch.cat([-t[..., hd // 2:], t[..., :hd // 2]], dim=-1) * sin

    x = ln(W["embeddings.word_embeddings.weight"][ids_t] + W["embeddings.token_type_embeddings.weight"][0], "embeddings.LayerNorm")
    neg = (1.0 - m)[:, None, None, :] * -1e30
    for i in range(cfg.layers):
        p = f"layers.{i}."
        q, k, v = (lin(x, p + f"self_attn.{n}_proj").view(B, S, nh, hd).transpose(1, 2) for n in "qkv")
        a = torch.softmax(rot(q) @ rot(k).transpose(-1, -2) / math.sqrt(hd) + neg, dim=-1)
        ctx = (a @ v).transpose(1, 2).reshape(B, S, H)
        x = ln(lin(ctx, p + "self_attn.o_proj") + x, p + "post_attention_layernorm")
        g = lin(x, p + "mlp.gate_proj")
        x = ln(lin(g * torch.sigmoid(g) * lin(x, p + "mlp.up_proj"), p + "mlp.down_proj") + x, p + "post_mlp_layernorm")
    return x.numpy()


def write_nomic_dir(path, dialect, *, hidden=64, layers=2, heads=4, ffn=128, max_pos=256, max_seq=48, seed=0, cfg_over=None, biases=False):
    """A tiny model_type "nomic_bert" directory: 'hub' (the published checkpoint's tensor and config names) or 'hf' (as
    transformers 5.x saves NomicBertModel).  Returns the weights under NomicBertModel's names."""
    from safetensors.numpy import save_file
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    from _modeldir import make_vocab
    vocab = make_vocab()
    rng = np.random.default_rng(seed)
    h, f = hidden, ffn
    shapes = {"embeddings.word_embeddings.weight": (len(vocab), h), "embeddings.token_type_embeddings.weight": (2, h),
              "embeddings.LayerNorm.weight": (h,), "embeddings.LayerNorm.bias": (h,)}
    for i in range(layers):
        p = f"layers.{i}."
        for n in "qkvo":
            shapes[p + f"self_attn.{n}_proj.weight"] = (h, h)
            if biases:
                shapes[p + f"self_attn.{n}_proj.bias"] = (h,)
        shapes.update({p + "mlp.gate_proj.weight": (f, h), p + "mlp.up_proj.weight": (f, h), p + "mlp.down_proj.weight": (h, f),
                       p + "post_attention_layernorm.weight": (h,), p + "post_attention_layernorm.bias": (h,),
                       p + "post_mlp_layernorm.weight": (h,), p + "post_mlp_layernorm.bias": (h,)})
        if biases:
            shapes.update({p + "mlp.gate_proj.bias": (f,), p + "mlp.up_proj.bias": (f,), p + "mlp.down_proj.bias": (h,)})
    w = {k: (0.08 * rng.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    if dialect == "hub":
        cfg = {"architectures": ["NomicBertModel"], "model_type": "nomic_bert", "vocab_size": len(vocab), "n_embd": h, "n_head": heads,
               "n_layer": layers, "n_inner": f, "n_positions": max_pos, "rotary_emb_base": 1000, "rotary_emb_fraction": 1.0,
               "rotary_emb_interleaved": False, "activation_function": "swiglu", "qkv_proj_bias": biases, "mlp_fc1_bias": biases,
               "mlp_fc2_bias": biases, "prenorm": False, "layer_norm_epsilon": 1e-12, "type_vocab_size": 2}
        disk = {}
        for k, v in w.items():
            k = k.replace("embeddings.LayerNorm.", "emb_ln.")
            if k.startswith("layers."):
                k = "encoder." + k
            for old, new in ((".self_attn.o_proj.", ".attn.out_proj."), (".mlp.up_proj.", ".mlp.fc11."), (".mlp.gate_proj.", ".mlp.fc12."),
                             (".mlp.down_proj.", ".mlp.fc2."), (".post_attention_layernorm.", ".norm1."), (".post_mlp_layernorm.", ".norm2.")):
                k = k.replace(old, new)
            disk[k] = v
        for i in range(layers):
            for kind in (("weight", "bias") if biases else ("weight",)):
                parts = [disk.pop(f"encoder.layers.{i}.self_attn.{n}_proj.{kind}") for n in "qkv"]
                disk[f"encoder.layers.{i}.attn.Wqkv.{kind}"] = np.concatenate(parts)
    else:
        cfg = {"architectures": ["NomicBertModel"], "model_type": "nomic_bert", "vocab_size": len(vocab), "hidden_size": h,
               "num_attention_heads": heads, "num_hidden_layers": layers, "intermediate_size": f, "max_position_embeddings": max_pos,
               "hidden_act": "silu", "layer_norm_eps": 1e-12, "type_vocab_size": 2, "head_dim": h // heads, "pad_token_id": 0,
               "rope_parameters": {"rope_theta": 1000.0, "rope_type": "default"}}
        disk = dict(w)
    cfg.update(cfg_over or {})
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    json.dump({"max_seq_length": max_seq, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    json.dump({"do_lower_case": True, "tokenizer_class": "BertTokenizer", "cls_token": "[CLS]", "sep_token": "[SEP]"},
              open(os.path.join(path, "tokenizer_config.json"), "w"))
    json.dump({"word_embedding_dimension": h, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
               "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    with open(os.path.join(path, "vocab.txt"), "w", encoding="utf-8") as fh:
        fh.write("\n".join(vocab) + "\n")
    save_file({k: np.ascontiguousarray(v) for k, v in disk.items()}, os.path.join(path, "model.safetensors"))
    return w, vocab
