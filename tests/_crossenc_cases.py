"""Shared by tools/make_crossenc_golden.py (which writes tests/golden/crossenc.npz with transformers'
BertForSequenceClassification in fp64) and the cross-encoder tests: the cases, their seeded weights under the package's internal
(BertModel) tensor names plus pooler.dense.* / classifier.*, the token / type-id generator, an fp64 restatement of the pair
forward and of the head, and a writer of cross-encoder model directories."""
import json
import math
import os
from dataclasses import dataclass

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crossenc.npz")
PAD_ID, CLS_ID, SEP_ID = 0, 1, 2
HIDDEN_ROWS_CAP = 64                       # hidden states kept per case (a committed file stays under 1 MiB)
HEAD = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")
TYPE_EMB = "embeddings.token_type_embeddings.weight"
# classifier weights ~N(0, 0.05), wider in the cases (by seed) whose logits would otherwise move too little when the type ids
# are zeroed (the short pairs of the tiny cases): see ZEROED_TYPES_GAP
CLS_SCALE = {201: 0.2, 202: 0.4}

# Largest |logit - fp64 golden| per case.  NOT yet measured on an MI355X (no device was available when this was written): these
# are the figures of the fp16-rounding model below (pair_forward_ref(..., emulate_fp16=True): fp64 arithmetic, a round trip through
# fp16 at every point where the kernels store or consume fp16), i.e. the error the number formats alone give; the device adds the
# fp32 summation order.  The bound of the parity test is four times the largest (room for kernel-selection changes that reorder
# fp16 sums).  To replace them by measurements: run tests/test_crossenc_gpu.py with -s (it prints the device's figure per case and
# selection), write the per-case maxima here and into profiles/crossenc_parity.txt, re-run tools/make_crossenc_golden.py.
# The pair head is now bounded on its own: tests/test_row_kernels_gpu.py runs pair_head_kernel<1> and <2> alone (crs_pair_head_f32)
# against fp64 under the derived bound of tests/_row_ref.py; the end-to-end tolerance below stays as it is.
MODELLED_LOGIT_ERR = {"tiny_4x24": 2.2e-4, "tiny_3x5": 2.0e-4, "mid_3x80": 4.3e-4, "base_2x150": 5.0e-4, "base_1x512": 8.3e-4}
LOGIT_TOL = 4 * max(MODELLED_LOGIT_ERR.values())
# the generator asserts, per case: zeroing the type ids moves the fp64 logits (largest change over the rows) by more than this, so a
# kernel that ignores them fails the parity test
ZEROED_TYPES_GAP = 10 * LOGIT_TOL


@dataclass(frozen=True)
class CeCfg:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int
    ln_eps: float = 1e-12


TINY = CeCfg("tiny", 1000, 64, 2, 4, 256, 64)                # head_dim 16 (synthetic:tiny-ce's shape)
MID = CeCfg("mid", 2000, 384, 2, 12, 1536, 128)              # head_dim 32: two layers of ms-marco-MiniLM's shape, small vocabulary
BASE = CeCfg("base", 2000, 768, 2, 12, 3072, 512)            # head_dim 64

# (key, config, seed, batch, seq)
CASES = [("tiny_4x24", TINY, 201, 4, 24), ("tiny_3x5", TINY, 202, 3, 5), ("mid_3x80", MID, 203, 3, 80),
         ("base_2x150", BASE, 204, 2, 150), ("base_1x512", BASE, 205, 1, 512)]


def case(key):
    return next(c for c in CASES if c[0] == key)


def weight_names(cfg: CeCfg):
    h, f = cfg.hidden, cfg.ffn
    out = [("embeddings.word_embeddings.weight", (cfg.vocab_size, h)), ("embeddings.position_embeddings.weight", (cfg.max_pos, h)),
           (TYPE_EMB, (2, h)), ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
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
    out += [(HEAD[0], (h, h)), (HEAD[1], (h,)), (HEAD[2], (1, h)), (HEAD[3], (1,))]
    return out


def make_weights(cfg: CeCfg, seed: int):
    """One PCG64 stream per tensor: matrices (the two token-type rows, the pooler) ~N(0, 0.05), the classifier ~N(0, CLS_SCALE.get(seed, 0.05)),
    biases ~N(0, 0.02), LayerNorm gains 1 + N(0, 0.05)."""
    w = {}
    for idx, (name, shape) in enumerate(weight_names(cfg)):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if name.endswith("LayerNorm.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(shape, dtype=np.float32)
        elif name.endswith(".bias"):
            a = 0.02 * rng.standard_normal(shape, dtype=np.float32)
        elif name == HEAD[2]:
            a = CLS_SCALE.get(seed, 0.05) * rng.standard_normal(shape, dtype=np.float32)
        else:
            a = 0.05 * rng.standard_normal(shape, dtype=np.float32)
        w[name] = a.astype(np.float32)
    return w


def synth_pairs(cfg: CeCfg, batch: int, seq: int, seed: int):
    """[CLS] a [SEP] b [SEP] rows, right-padded, ragged lengths (row 0 is full) with the segment boundary at a different place
    in every row; from four rows on, the last row is a single sentence [CLS] a [SEP] (all type 0).  At seq 5 every row is the
    shortest legal pair.  -> (ids, type_ids, mask), int32 [B, S]."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(3, cfg.vocab_size, size=(batch, seq), dtype=np.int64)
    types = np.zeros((batch, seq), dtype=np.int64)
    lens = np.full(batch, seq, dtype=np.int64)
    if batch > 1 and seq > 5:
        lens[1:] = rng.integers(max(5, seq // 3), seq, size=batch - 1)
    for b in range(batch):
        n = int(lens[b])
        ids[b, 0], ids[b, n - 1], ids[b, n:] = CLS_ID, SEP_ID, PAD_ID
        if batch >= 4 and b == batch - 1:
            continue                                          # single sentence: all type 0
        n_a = 1 + (b * 7 + int(rng.integers(0, n - 4 + 1))) % (n - 4) if n > 5 else 1      # 1 <= n_a <= n - 4
        ids[b, 1 + n_a] = SEP_ID
        types[b, 2 + n_a:n] = 1
    mask = np.arange(seq)[None, :] < lens[:, None]
    return ids.astype(np.int32), types.astype(np.int32), mask.astype(np.int32)


def hidden_rows(mask: np.ndarray) -> np.ndarray:
    """Flat indices (into [B * S]) of the real tokens whose hidden states the golden file keeps: all of them in a small
    case, else the first and last two of every sequence ([CLS] among them) plus an even spread."""
    real = np.flatnonzero(mask.reshape(-1))
    if real.size <= HIDDEN_ROWS_CAP:
        return real
    B, S = mask.shape
    lens = mask.sum(1)
    ends = [b * S + j for b in range(B) for j in (0, 1, lens[b] - 2, lens[b] - 1)]
    spread = real[np.linspace(0, real.size - 1, HIDDEN_ROWS_CAP - len(ends)).astype(np.int64)]
    return np.unique(np.concatenate([np.asarray(ends, dtype=np.int64), spread]))


def model_shape(cfg: CeCfg):
    from rag._encoder import ModelShape
    return ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, "cls", cfg.max_pos)


def head_ref(h_cls, w):
    """fp64 head on [B, H] first-token states -> (pooled [B, H], logits [B])."""
    h = np.asarray(h_cls, dtype=np.float64)
    pooled = np.tanh(h @ w[HEAD[0]].astype(np.float64).T + w[HEAD[1]].astype(np.float64))
    return pooled, pooled @ w[HEAD[2]].astype(np.float64).reshape(-1) + float(w[HEAD[3]].reshape(-1)[0])


def pair_forward_ref(ids, types, mask, w, cfg: CeCfg, emulate_fp16: bool = False):
    """fp64 restatement of the pair forward: embeddings (word + type[t]) + position -> LayerNorm, the post-LN BERT layers,
    then head_ref on token 0.  -> (hidden [B, S, H], pooled [B, H], logits [B]), numpy fp64.  emulate_fp16: the same arithmetic with
    a round trip through fp16 wherever the HIP encoder stores or consumes fp16 (the rounding points of oracle/encoder_ref.py: GEMM
    weights, the LayerNorm's fp16 copy, Q | K | V, the softmax numerators, the attention output, the GELU output) -- a model of
    the device's error from the number formats alone."""
    import torch
    r16 = (lambda t: t.float().half().double()) if emulate_fp16 else (lambda t: t)
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).double() for k, v in w.items()}
    ids_t, ty_t = torch.from_numpy(np.asarray(ids)).long(), torch.from_numpy(np.asarray(types)).long()
    m = torch.from_numpy(np.asarray(mask)).double()
    B, S = ids_t.shape
    H, nh = cfg.hidden, cfg.heads
    hd = H // nh

    def ln(x, name):
        mu = x.mean(-1, keepdim=True)
        var = ((x - mu) ** 2).mean(-1, keepdim=True)
        return (x - mu) / torch.sqrt(var + cfg.ln_eps) * W[name + ".weight"] + W[name + ".bias"]

    x = ln((W["embeddings.word_embeddings.weight"][ids_t] + W[TYPE_EMB][ty_t]) + W["embeddings.position_embeddings.weight"][:S][None],
           "embeddings.LayerNorm")
    neg = (1.0 - m)[:, None, None, :] * -1e30
    for i in range(cfg.layers):
        p = f"encoder.layer.{i}."
        lin = lambda v, name: v @ r16(W[p + name + ".weight"]).T + W[p + name + ".bias"]
        x16 = r16(x)
        q, k, v = (r16(lin(x16, "attention.self." + n)).view(B, S, nh, hd).transpose(1, 2) for n in ("query", "key", "value"))
        sc = q @ k.transpose(-1, -2) / math.sqrt(hd) + neg
        e = torch.exp(sc - sc.amax(-1, keepdim=True))
        ctx = r16(((r16(e) @ v) / e.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, S, H))
        x = ln(lin(ctx, "attention.output.dense") + x, p + "attention.output.LayerNorm")
        hmid = lin(r16(x), "intermediate.dense")
        x = ln(lin(r16(0.5 * hmid * (1.0 + torch.erf(hmid / math.sqrt(2.0)))), "output.dense") + x, p + "output.LayerNorm")
    hidden = x.numpy()
    pooled, logits = head_ref(hidden[:, 0], w)
    return hidden, pooled, logits


def write_crossenc_dir(path, *, labels=1, pooler=True, classifier=True, activation_fn=None, model_type="bert", seed=0):
    """A BertForSequenceClassification directory: the sentence-encoder directory of tests/_modeldir.py (vocab.txt, tokenizer
    files, bert.* tensors) with a cross-encoder's config.json and model.safetensors (bert.pooler.dense.*, classifier.*).
    Returns the weights under the internal names."""
    from safetensors.numpy import save_file
    from _modeldir import write_model_dir
    weights, cfg = write_model_dir(path, seed=seed)
    h = cfg["hidden_size"]
    cfg.update({"architectures": ["BertForSequenceClassification"], "model_type": model_type, "num_labels": labels,
                "id2label": {str(i): f"LABEL_{i}" for i in range(labels)}})
    if activation_fn is not None:
        cfg["sbert_ce_default_activation_function"] = activation_fn
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    rng = np.random.default_rng(seed + 1)
    if pooler:
        weights[HEAD[0]] = (0.08 * rng.standard_normal((h, h))).astype(np.float32)
        weights[HEAD[1]] = (0.02 * rng.standard_normal((h,))).astype(np.float32)
    disk = {"bert." + k: v for k, v in weights.items()}
    if classifier:
        weights[HEAD[2]] = disk[HEAD[2]] = (0.2 * rng.standard_normal((labels, h))).astype(np.float32)
        weights[HEAD[3]] = disk[HEAD[3]] = (0.02 * rng.standard_normal((labels,))).astype(np.float32)
    save_file(disk, os.path.join(path, "model.safetensors"))
    return weights
