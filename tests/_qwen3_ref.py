"""Qwen3 test helper: the two tiny model configurations of tests/golden/encoder_qwen3.npz with their seeded weights (shared with
tools/make_qwen3_golden.py), a model directory writer, and plain fp64 references with DERIVED bounds for the three new kernels.
numpy only.  u = 2^-24; every fp32 operation is charged 2u relative, as in tests/_attn_ref.py and tests/_row_ref.py.

causal_ref_and_bound   tests/_attn_ref.py's bound restated for the grouped layout and the causal mask.  Query head h reads key / value
                       head h // G, and row q attends the keys j < lim(q) = min(q + 1, len).  The terms are those of ref_and_bound --
                       P rounded to fp16 (2^-10 P, + 2^-25 per subnormal weight), the score term eps_j, fp32 accumulation 2u (66 nb) P
                       and the row sum 2u (18 + 2 nb + 3) |o| per 64-key block, the output's fp16 rounding -- with nb = ceil(lim / 64),
                       the blocks THIS row walks, and the 32-deep products charged as 64 additions per block like the 16-deep ones.
qk_norm_rope           n = x r g, r = 1 / sqrt(mean(x^2) + eps); out = n_lo cos - n_hi sin (and the mirror).  Inputs are fp16 values
                       (exact in fp32).  fp32 terms: the sum of squares of hd terms 2u (log2(hd) + 2) relative on ss (products + tree),
                       the division, addition, sqrt and reciprocal 8u on r (a relative error e on ss gives e / 2 on r) -> er = u (log2(hd)
                       + 6); n: two multiplications more, en = er + 4u; the rotation: |n_lo cos| (en + 2u) + |n_hi sin| (en + 2u) + 2u
                       |out| for the subtraction; the table entries are fp32 roundings of the fp64 angles' cos / sin: u each, inside.
                       Then ONE fp16 rounding: half an fp16 ulp of (|ref| + the above) + 2^-24.
rmsnorm                layernorm_ref_and_bound's restatement without mean and bias: r = (sum of slabs) + residual in fp32, 2u per
                       addition on the partial sums; ss over H terms 2u (log2(64) + H / 64 + 2); rstd as above; x = r rstd g: 4u more;
                       a perturbation dr of the row moves x by |dr| rstd |g| (1 + x^2 / H-ish second term bounded by the same) -- charged
                       2 |dr| rstd |g|; x16: half an fp16 ulp on top; n32: the fp32 terms alone."""
import json
import math
import os
import shutil

import numpy as np

import _attn_ref as ar

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "encoder_qwen3.npz")
TOKENIZER_JSON = os.path.join(HERE, "golden", "modernbert_tokenizer.json")     # a small byte-level BPE file: [CLS] $A [SEP]
U = 2.0 ** -24
LENS, SEQ = (1, 63, 64, 65, 130), 130
CFGS = {      # the two tiny models: (head_dim 128, 2 query heads on 1 key / value head) and (head_dim 64, 2 on 2)
    "g2": dict(vocab=300, hidden=128, layers=2, heads=2, kv_heads=1, head_dim=128, ffn=256, max_pos=256, eps=1e-6, theta=1e6, seed=71),
    "g1": dict(vocab=300, hidden=128, layers=2, heads=2, kv_heads=2, head_dim=64, ffn=256, max_pos=256, eps=1e-6, theta=1e6, seed=72),
}


def shape(cfg):
    from rag._encoder import ModelShape
    return ModelShape(cfg["vocab"], cfg["hidden"], cfg["layers"], cfg["heads"], cfg["ffn"], cfg["max_pos"], cfg["eps"], "last", cfg["max_pos"],
                      rotary_theta=cfg["theta"], gated=True, causal=True, kv_heads=cfg["kv_heads"], head_dim=cfg["head_dim"])


def make_weights(cfg):
    """rag.embedding.synthetic_weights of the shape (Qwen3Model's names), matrices ~ 0.08 N(0, 1)"""
    from rag.embedding import synthetic_weights
    return synthetic_weights(shape(cfg), cfg["seed"], scale=0.08)


def weights_digest(w):
    import hashlib
    d = hashlib.sha256()
    for k in sorted(w):
        d.update(k.encode() + np.ascontiguousarray(w[k]).tobytes())
    return d.hexdigest()


def synth_ids(cfg):
    """int32 [len(LENS), SEQ] right-padded with id 0, real ids in [3, vocab)"""
    rng = np.random.default_rng(cfg["seed"] + 1000)
    ids = rng.integers(3, cfg["vocab"], size=(len(LENS), SEQ)).astype(np.int32)
    ids[np.arange(SEQ)[None, :] >= np.asarray(LENS)[:, None]] = 0
    return ids


def hf_config(cfg):
    return {"architectures": ["Qwen3Model"], "model_type": "qwen3", "vocab_size": cfg["vocab"], "hidden_size": cfg["hidden"],
            "num_hidden_layers": cfg["layers"], "num_attention_heads": cfg["heads"], "num_key_value_heads": cfg["kv_heads"],
            "head_dim": cfg["head_dim"], "intermediate_size": cfg["ffn"], "max_position_embeddings": cfg["max_pos"],
            "rms_norm_eps": cfg["eps"], "rope_theta": cfg["theta"], "hidden_act": "silu", "attention_bias": False,
            "use_sliding_window": False, "tie_word_embeddings": False}


def write_model_dir(path, cfg, weights, overrides=None, st_layout=True, prefix="model."):
    """A model_type qwen3 directory: the layout files of tests/_modeldir.write_model_dir, with its BERT config.json and weights replaced
    by Qwen3's (names under `prefix`, plus an lm_head the loader must ignore), the BPE tokenizer.json fixture, and 1_Pooling saying
    pooling_mode_lasttoken (st_layout) or absent (a bare Qwen3Model)."""
    import _modeldir
    from safetensors.numpy import save_file
    _modeldir.write_model_dir(path, modules_json=st_layout, max_seq=cfg["max_pos"])
    json.dump({**hf_config(cfg), **(overrides or {})}, open(os.path.join(path, "config.json"), "w"))
    save_file({**{prefix + k: v for k, v in weights.items()}, "lm_head.weight": np.zeros((4, cfg["hidden"]), dtype=np.float32)},
              os.path.join(path, "model.safetensors"))
    shutil.copy(TOKENIZER_JSON, os.path.join(path, "tokenizer.json"))
    pool = os.path.join(path, "1_Pooling", "config.json")
    if st_layout:
        json.dump({"word_embedding_dimension": cfg["hidden"], "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": False,
                   "pooling_mode_lasttoken": True}, open(pool, "w"))
    else:
        os.remove(pool)
    return path


# ---- causal grouped-query attention -------------------------------------------------------------------------------------------------
def grouped_inputs(batch, seq, heads, kv_heads, hd, lens, seed):
    """fp16 [batch * seq, (heads + 2 kv_heads) hd] from tests/_attn_ref.make_inputs (poisoned padding, peaked scores): its Q block and
    the first kv_heads heads of its K and V blocks."""
    full = ar.make_inputs(batch, seq, heads, hd, lens, seed, peaked=True)
    h = heads * hd
    return np.ascontiguousarray(np.concatenate([full[:, :h], full[:, h:h + kv_heads * hd], full[:, 2 * h:2 * h + kv_heads * hd]], axis=1))


def causal_ref_and_bound(qkv, lens, batch, seq, heads, kv_heads, hd, fault=None):
    """(ref, bound) fp64 [batch * seq, heads * hd]; rows q >= len hold the attention over the real keys (the kernel's, unread).
    fault: 'leak_future' admits key q + 1, 'drop_diagonal' drops key q (planted in the REFERENCE: the bound must reject them)."""
    x = np.asarray(qkv, dtype=np.float64).reshape(batch, seq, heads + 2 * kv_heads, hd)
    g = heads // kv_heads
    n = ar.clamp_lens(lens, seq)
    ref = np.empty((batch, seq, heads, hd))
    bound = np.empty_like(ref)
    rs = 1.0 / math.sqrt(hd)
    qi = np.arange(seq)
    for b in range(batch):
        ln = int(n[b])
        lim = np.minimum(qi + 1, ln)
        if fault == "leak_future":
            lim = np.minimum(qi + 2, ln)
        nb = ((np.minimum(qi + 1, ln) + 63) // 64)[:, None]
        live = np.arange(ln)[None, :] < lim[:, None]
        if fault == "drop_diagonal":
            live &= ~((np.arange(ln)[None, :] == qi[:, None]) & (qi[:, None] > 0))
        for h in range(heads):
            qq, kk, vv = x[b, :, h], x[b, :ln, heads + h // g], x[b, :ln, heads + kv_heads + h // g]
            d = qq @ kk.T * rs
            a = np.abs(qq) @ np.abs(kk).T * rs
            s = np.where(live, d, -np.inf)
            mx = s.max(axis=1, keepdims=True)
            p = np.exp(s - mx)
            l = p.sum(axis=1, keepdims=True)
            w = p / l
            o = w @ vv
            pabs = w @ np.abs(vv)
            eps = np.where(live, U * (2 * hd * a + 6 * np.abs(d) + 2 * np.abs(d) + 4 * np.abs(np.where(live, s - mx, 0.0)) + 4), 0.0)
            weps = w * eps
            e = 2.0 ** -10 * pabs + 2.0 ** -25 * ((live & (p < 2.0 ** -14)) @ np.abs(vv)) / l
            e += np.exp(2 * eps.max(axis=1, keepdims=True)) * (weps @ np.abs(vv) + np.abs(o) * weps.sum(axis=1, keepdims=True))
            e += 2 * U * (66 * nb) * pabs + 2 * U * (18 + 2 * nb + 3) * np.abs(o)
            ref[b, :, h] = o
            bound[b, :, h] = e + 2.0 ** -11 * (np.abs(o) + e) + 2.0 ** -24
    return ref.reshape(batch * seq, heads * hd), bound.reshape(batch * seq, heads * hd)


# ---- qk_norm_rope --------------------------------------------------------------------------------------------------------------------
def qk_norm_rope_ref_and_bound(qkv, table, g_q, g_k, eps, seq, heads, kv_heads, hd):
    """(ref, bound) fp64 over the Q and K blocks [T, (heads + kv_heads) hd] of qkv fp16 [T, (heads + 2 kv_heads) hd]; table fp32
    [positions, hd] (cos | sin), token t at position t % seq"""
    t = qkv.shape[0]
    nh, half = heads + kv_heads, hd // 2
    x = np.asarray(qkv, dtype=np.float64)[:, :nh * hd].reshape(t, nh, hd)
    gain = np.stack([np.asarray(g_q if h < heads else g_k, dtype=np.float64) for h in range(nh)])[None]
    tab = np.asarray(table, dtype=np.float64)[np.arange(t) % seq]
    cs, sn = tab[:, None, :half], tab[:, None, half:]
    r = 1.0 / np.sqrt((x * x).mean(axis=2, keepdims=True) + eps)
    nrm = x * r * gain
    lo, hi = nrm[..., :half], nrm[..., half:]
    ref = np.concatenate([lo * cs - hi * sn, hi * cs + lo * sn], axis=2)
    en = U * (math.log2(hd) + 6) + 4 * U
    mag = np.concatenate([np.abs(lo * cs) + np.abs(hi * sn), np.abs(hi * cs) + np.abs(lo * sn)], axis=2)
    f32 = mag * (en + 2 * U) + 2 * U * np.abs(ref)
    bound = f32 + ar.half_ulp16(np.abs(ref) + f32) + 2.0 ** -24
    return ref.reshape(t, nh * hd), bound.reshape(t, nh * hd)


# ---- add_rmsnorm ---------------------------------------------------------------------------------------------------------------------
def rmsnorm_ref_and_bound(y, residual, g, eps):
    """y fp32 [ns, T, H], residual fp32 [T, H] or None, g fp32 [H] -> dict r / x16 / n32 -> (ref, bound) in fp64"""
    y64 = np.asarray(y, dtype=np.float64)
    ns, _, hidden = y64.shape
    r = y64.sum(axis=0) + (0.0 if residual is None else np.asarray(residual, dtype=np.float64))
    mag = np.abs(y64).sum(axis=0) + (0.0 if residual is None else np.abs(np.asarray(residual, dtype=np.float64)))
    dr = 2 * U * ns * mag                                          # ns additions, each on a partial sum below mag
    gg = np.abs(np.asarray(g, dtype=np.float64))[None, :]
    rstd = 1.0 / np.sqrt((r * r).mean(axis=1, keepdims=True) + eps)
    x = r * rstd * np.asarray(g, dtype=np.float64)[None, :]
    e_ss = 2 * U * (6 + hidden / 64 + 2)                            # per-lane chain of H / 64 terms, six cross-lane steps, products
    e_rstd = e_ss / 2 + 8 * U + (2 * np.abs(r) * dr).sum(axis=1, keepdims=True) / (r * r).sum(axis=1, keepdims=True).clip(1e-300) / 2
    e_x = np.abs(x) * (e_rstd + 4 * U) + 2 * dr * rstd * gg
    return {"r": (r, dr + 2.0 ** -149), "n32": (x, e_x + 2.0 ** -126), "x16": (x, e_x + ar.half_ulp16(np.abs(x) + e_x) + 2.0 ** -24)}
