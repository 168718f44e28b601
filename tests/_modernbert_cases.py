"""Shared by tools/make_modernbert_golden.py (which writes tests/golden/encoder_modernbert.npz with transformers.ModernBertModel in
fp64, eager attention) and the ModernBERT tests: the cases, their seeded weights under ModernBertModel's tensor names (the package's
internal names for this family), token ids, the fp64 restatement of the forward in numpy, and a writer of tiny model directories."""
import json
import math
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "encoder_modernbert.npz")
TOKENIZER_JSON = os.path.join(HERE, "golden", "modernbert_tokenizer.json")
TOKENIZER_CASES = os.path.join(HERE, "golden", "modernbert_tokenizer_cases.json")
PAD_ID, CLS_ID, SEP_ID = 0, 1, 2
GLOBAL_THETA, LOCAL_THETA = 160000.0, 10000.0


@dataclass(frozen=True)
class MbCfg:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int
    max_seq: int
    local_attention: int = 16      # window = 8: bites at the sizes below
    global_every: int = 3
    norm_eps: float = 1e-5

    @property
    def window(self):
        return self.local_attention // 2


CFG_A = MbCfg("a", 300, 64, 4, 4, 128, 256, 160)       # head_dim 16; layers 0 and 3 full, 1 and 2 sliding
CFG_B = MbCfg("b", 300, 128, 3, 2, 192, 256, 160)      # head_dim 64; layer 0 full, 1 and 2 sliding

# (key, config, seed, lens, seq).  Length 5 leaves padding rows without any allowed key (q >= 5 + 8); seq 144 is three query blocks,
# and rows 73 .. 127 of query block 1 find key block 0 wholly outside their window
CASES = [("a_48", CFG_A, 301, (48, 5, 30), 48), ("a_144", CFG_A, 302, (144, 73, 5), 144),
         ("b_48", CFG_B, 303, (48, 5, 30), 48), ("b_144", CFG_B, 304, (144, 73, 5), 144)]


def weight_names(cfg: MbCfg, biases: bool = False):
    h, f = cfg.hidden, cfg.ffn
    out = [("embeddings.tok_embeddings.weight", (cfg.vocab_size, h)), ("embeddings.norm.weight", (h,))]
    if biases:
        out.append(("embeddings.norm.bias", (h,)))
    for i in range(cfg.layers):
        p = f"layers.{i}."
        if i:
            out.append((p + "attn_norm.weight", (h,)))
            if biases:
                out.append((p + "attn_norm.bias", (h,)))
        out += [(p + "attn.Wqkv.weight", (3 * h, h)), (p + "attn.Wo.weight", (h, h)), (p + "mlp_norm.weight", (h,)),
                (p + "mlp.Wi.weight", (2 * f, h)), (p + "mlp.Wo.weight", (h, f))]
        if biases:
            out += [(p + "attn.Wqkv.bias", (3 * h,)), (p + "attn.Wo.bias", (h,)), (p + "mlp_norm.bias", (h,)),
                    (p + "mlp.Wi.bias", (2 * f,)), (p + "mlp.Wo.bias", (h,))]
    out.append(("final_norm.weight", (h,)))
    if biases:
        out.append(("final_norm.bias", (h,)))
    return out


def make_weights(cfg: MbCfg, seed: int, biases: bool = False):
    """One PCG64 stream per tensor: gains 1 + N(0, 0.05), biases N(0, 0.02), matrices N(0, 0.08) -- except the query / key rows of
    Wqkv, N(0, 1.5 / hidden): on normalised inputs the scores q . k / sqrt(hd) then have a standard deviation near 1.5, so that the
    softmax is not flat and a key inside or outside the window moves the output."""
    w, h = {}, cfg.hidden
    for idx, (name, shape) in enumerate(weight_names(cfg, biases)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if name.endswith("norm.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith(".bias"):
            a = 0.02 * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = 0.08 * rng.standard_normal(shape, dtype=np.float32)
            if name.endswith("attn.Wqkv.weight"):
                a[: 2 * h] = math.sqrt(1.5 / h) * rng.standard_normal((2 * h, h), dtype=np.float32)
        w[name] = a.astype(np.float32)
    return w


def synth_tokens(cfg: MbCfg, lens, seq: int, seed: int):
    """[CLS] ... [SEP], right-padded with [PAD] -> (ids int32 [B, S], mask int32 [B, S])."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    ids = rng.integers(3, cfg.vocab_size, size=(len(lens), seq), dtype=np.int64)
    mask = np.arange(seq)[None, :] < lens[:, None]
    ids[:, 0] = CLS_ID
    ids[np.arange(len(lens)), lens - 1] = SEP_ID
    ids[~mask] = PAD_ID
    return ids.astype(np.int32), mask.astype(np.int32)


def model_shape(cfg: MbCfg, pooling: str = "mean"):
    from rag._encoder import ModelShape
    return ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.norm_eps, pooling, cfg.max_seq,
                      rotary_theta=GLOBAL_THETA, local_theta=LOCAL_THETA, prenorm=True, gelu_gated=True, window=cfg.window,
                      global_every=cfg.global_every)


def rope_cos_sin(positions: int, hd: int, theta: float):
    """fp64 (cos, sin), each [positions, hd / 2]: the angles pos * theta^(-2 j / hd)."""
    inv = np.float64(theta) ** (-2.0 * np.arange(hd // 2, dtype=np.float64) / hd)
    ang = np.arange(positions, dtype=np.float64)[:, None] * inv[None, :]
    return np.cos(ang), np.sin(ang)


def rope_cos_sin_fp32(positions: int, hd: int, theta: float):
    """(cos, sin) as transformers' rotary embedding computes them whatever the model's dtype: inverse frequencies, angles, cosines
    and sines in fp32 (the golden file was made with these)."""
    import torch
    inv = 1.0 / (theta ** (torch.arange(0, hd, 2, dtype=torch.float) / hd))
    ang = (inv[:, None] @ torch.arange(positions, dtype=torch.float)[None, :]).T
    return ang.cos().numpy().astype(np.float64), ang.sin().numpy().astype(np.float64)


def window_mask(seq: int, window: int):
    """[query, key] True where the key is allowed: |i - j| <= window, both ends included."""
    i = np.arange(seq)
    return np.abs(i[:, None] - i[None, :]) <= window


def erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def gelu(x):
    return 0.5 * x * (1.0 + erf(x / math.sqrt(2.0)))


def encode_ref(ids, mask, w, cfg: MbCfg, fp32_angles: bool = False, window_rule=None, act=gelu):
    """fp64 numpy restatement of the forward the library runs for a ModernBERT shape (and of transformers.ModernBertModel):
        r     = LN(tok[ids])                                              no position table, no token types
        per layer i:  x = r (i = 0) or LN_attn(r);  q, k, v = x Wqkv^T;  q, k rotated with the layer type's theta
                      allowed(query, key) = key is real and (layer is full: i % global_every == 0, or |query - key| <= window)
                      r = r + softmax(q k^T / sqrt(hd) over the allowed keys) v Wo^T
                      input, gate = (LN_mlp(r) Wi^T).chunk(2);  r = r + (gelu(input) * gate) Wo^T
        hidden = LN_final(r)
    Norms have a bias only where w carries one; so do the projections.  window_rule(seq, window) -> bool [query, key] replaces
    window_mask (planted faults); act replaces the GELU.  -> [B, S, H] fp64; rows of padding queries hold whatever the allowed
    real keys give them (zeros where a sliding layer allows none: their context is defined as 0 there)."""
    W = {k: np.asarray(v, dtype=np.float64) for k, v in w.items()}
    ids, real = np.asarray(ids), np.asarray(mask).astype(bool)
    B, S = ids.shape
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh

    def ln(x, name):
        mu = x.mean(-1, keepdims=True)
        var = ((x - mu) ** 2).mean(-1, keepdims=True)
        y = (x - mu) / np.sqrt(var + cfg.norm_eps) * W[name + ".weight"]
        return y + W[name + ".bias"] if name + ".bias" in W else y

    def lin(v, name):
        y = v @ W[name + ".weight"].T
        return y + W[name + ".bias"] if name + ".bias" in W else y

    tables = {}
    for kind, theta in (("full", GLOBAL_THETA), ("local", LOCAL_THETA)):
        cos, sin = (rope_cos_sin_fp32 if fp32_angles else rope_cos_sin)(S, hd, theta)
        tables[kind] = (np.concatenate([cos, cos], axis=1)[None, None], np.concatenate([sin, sin], axis=1)[None, None])

    def rot(t, kind):
        cos, sin = tables[kind]
        return t * cos + np.concatenate([-t[..., hd // 2:], t[..., :hd // 2]], axis=-1) * sin

    local = (window_rule or window_mask)(S, cfg.window)
    r = ln(W["embeddings.tok_embeddings.weight"][ids], "embeddings.norm")
    for i in range(cfg.layers):
        p = f"layers.{i}."
        full = i % cfg.global_every == 0
        x = ln(r, p + "attn_norm") if p + "attn_norm.weight" in W else r
        qkv = lin(x, p + "attn.Wqkv").reshape(B, S, 3, nh, hd).transpose(2, 0, 3, 1, 4)      # [3, B, nh, S, hd]
        kind = "full" if full else "local"
        q, k, v = rot(qkv[0], kind), rot(qkv[1], kind), qkv[2]
        allowed = real[:, None, None, :] & (np.ones((S, S), dtype=bool) if full else local)[None, None]
        s = np.where(allowed, q @ k.transpose(0, 1, 3, 2) / math.sqrt(hd), -np.inf)
        mx = s.max(-1, keepdims=True)
        e = np.where(allowed, np.exp(s - np.where(np.isfinite(mx), mx, 0.0)), 0.0)
        den = e.sum(-1, keepdims=True)
        a = e / np.where(den > 0, den, 1.0)                  # a query without any allowed key: a zero row
        ctx = (a @ v).transpose(0, 2, 1, 3).reshape(B, S, H)
        r = r + lin(ctx, p + "attn.Wo")
        inp, gate = np.split(lin(ln(r, p + "mlp_norm"), p + "mlp.Wi"), 2, axis=-1)
        r = r + lin(act(inp) * gate, p + "mlp.Wo")
    return ln(r, "final_norm")


def pooled(hidden, mask):
    """(mean-pooled, CLS-pooled), both L2-normalised, fp64 [B, H]"""
    m = np.asarray(mask, dtype=np.float64)
    mean = (hidden * m[..., None]).sum(1) / m.sum(1, keepdims=True)
    cls = hidden[:, 0]
    return mean / np.linalg.norm(mean, axis=1, keepdims=True), cls / np.linalg.norm(cls, axis=1, keepdims=True)


def hf_config_dict(cfg: MbCfg, **over):
    """config.json of a ModernBertModel of this shape, as transformers 5.x writes the keys this package reads"""
    d = {"architectures": ["ModernBertModel"], "model_type": "modernbert", "vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden,
         "num_attention_heads": cfg.heads, "num_hidden_layers": cfg.layers, "intermediate_size": cfg.ffn,
         "max_position_embeddings": cfg.max_pos, "hidden_activation": "gelu", "norm_eps": cfg.norm_eps, "norm_bias": False,
         "attention_bias": False, "mlp_bias": False, "local_attention": cfg.local_attention,
         "layer_types": ["full_attention" if i % cfg.global_every == 0 else "sliding_attention" for i in range(cfg.layers)],
         "rope_parameters": {"full_attention": {"rope_type": "default", "rope_theta": GLOBAL_THETA},
                             "sliding_attention": {"rope_type": "default", "rope_theta": LOCAL_THETA}},
         "pad_token_id": PAD_ID, "cls_token_id": CLS_ID, "sep_token_id": SEP_ID}
    d.update(over)
    return d


def write_modernbert_dir(path, cfg: MbCfg, weights, *, prefix: str = "", cfg_over=None, drop_keys=(), max_seq=None, pooling="mean",
                         tokenizer_json: str = TOKENIZER_JSON):
    """A model_type "modernbert" sentence-transformers directory: config.json, model.safetensors (tensor names with `prefix` in
    front: "" or "model."), the committed byte-level BPE tokenizer.json, sentence_bert_config.json and 1_Pooling/config.json."""
    import shutil

    from safetensors.numpy import save_file
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    c = hf_config_dict(cfg, **(cfg_over or {}))
    for k in drop_keys:
        c.pop(k, None)
    json.dump(c, open(os.path.join(path, "config.json"), "w"))
    json.dump({"max_seq_length": max_seq or cfg.max_seq, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    json.dump({"word_embedding_dimension": cfg.hidden, "pooling_mode_cls_token": pooling == "cls", "pooling_mode_mean_tokens": pooling == "mean",
               "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    shutil.copy(tokenizer_json, os.path.join(path, "tokenizer.json"))
    save_file({prefix + k: np.ascontiguousarray(v) for k, v in weights.items()}, os.path.join(path, "model.safetensors"))
    return path
