"""Shared by tools/make_xlmr_golden.py (which writes tests/golden/encoder_xlmr.npz and crossenc_xlmr.npz with transformers'
XLMRobertaModel / XLMRobertaForSequenceClassification in fp64) and the XLM-RoBERTa tests: the cases, their seeded weights under
the package's internal (BertModel) tensor names, token ids, and a writer of checkpoint directories."""
import json
import os
import shutil
from dataclasses import dataclass

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_xlmr.npz")
CE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "crossenc_xlmr.npz")
CLS_ID, PAD_ID, SEP_ID, UNK_ID = 0, 1, 2, 3          # <s>, <pad>, </s>, <unk>
POS_OFFSET = 2
HIDDEN_ROWS_CAP = 64                       # hidden states kept per case (a committed file stays under 1 MiB)
HEAD = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")
# internal head names -> XLMRobertaForSequenceClassification's
TO_CHECKPOINT_HEAD = {"pooler.dense.weight": "classifier.dense.weight", "pooler.dense.bias": "classifier.dense.bias",
                      "classifier.weight": "classifier.out_proj.weight", "classifier.bias": "classifier.out_proj.bias"}


@dataclass(frozen=True)
class XlmrCfg:
    name: str
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int          # rows of the position table (positions 2 .. max_pos - 1 are used)
    max_seq: int
    ln_eps: float = 1e-5


TINY = XlmrCfg("tiny", 1000, 64, 2, 4, 256, 66, 64)                 # synthetic:tiny-xlmr's shape
MID = XlmrCfg("mid", 2000, 384, 2, 12, 1536, 130, 128)              # two layers of multilingual-MiniLM's shape, small vocabulary
TOP = XlmrCfg("top", 250002, 64, 1, 4, 256, 66, 64)                 # XLM-R's vocabulary size: ids at the top of the table

# (key, config, seed, batch, seq).  tiny_1x64: one row of max_seq tokens, so the table's last row, max_pos - 1, is read
CASES = [("tiny_4x24", TINY, 401, 4, 24), ("tiny_1x64", TINY, 402, 1, 64), ("mid_3x80", MID, 403, 3, 80), ("top_2x16", TOP, 404, 2, 16)]
CE_CASES = [("tiny_4x24", TINY, 411, 4, 24), ("mid_3x80", MID, 412, 3, 80)]


def weight_names(cfg: XlmrCfg):
    h, f = cfg.hidden, cfg.ffn
    out = [("embeddings.word_embeddings.weight", (cfg.vocab_size, h)), ("embeddings.position_embeddings.weight", (cfg.max_pos, h)),
           ("embeddings.token_type_embeddings.weight", (1, h)),
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


def make_weights(cfg: XlmrCfg, seed: int):
    """One PCG64 stream per tensor: matrices (the one token-type row among them) ~N(0, 0.05), biases ~N(0, 0.02), LayerNorm gains
    1 + N(0, 0.05).  XLMRobertaModel's own tensor names are the internal ones."""
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


def make_ce_weights(cfg: XlmrCfg, seed: int):
    """make_weights plus the classification head under the internal names (pooler.dense.*, classifier.*): dense ~N(0, 0.05),
    out_proj ~N(0, 0.2), biases ~N(0, 0.02)."""
    w = make_weights(cfg, seed)
    h = cfg.hidden
    for idx, (name, shape, scale) in enumerate(((HEAD[0], (h, h), 0.05), (HEAD[1], (h,), 0.02), (HEAD[2], (1, h), 0.2), (HEAD[3], (1,), 0.02))):
        rng = np.random.Generator(np.random.PCG64([seed, 100000 + idx]))
        w[name] = (scale * rng.standard_normal(shape, dtype=np.float32)).astype(np.float32)
    return w


def checkpoint_names(w):
    """Internal names -> an XLMRobertaForSequenceClassification (or, without a head, XLMRobertaModel under `roberta.`) state dict."""
    return {TO_CHECKPOINT_HEAD.get(k, "roberta." + k): v for k, v in w.items()}


def synth_tokens(cfg: XlmrCfg, batch: int, seq: int, seed: int):
    """<s> ... </s>, right-padded with <pad>, ragged lengths (row 0 is full) -> (ids int32 [B, S], mask int32 [B, S]).  Half of
    the ids come from the last 64 rows of the vocabulary."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(4, cfg.vocab_size, size=(batch, seq), dtype=np.int64)
    top = rng.integers(cfg.vocab_size - 64, cfg.vocab_size, size=(batch, seq), dtype=np.int64)
    ids = np.where(rng.random((batch, seq)) < 0.5, top, ids)
    ids[0, 1] = cfg.vocab_size - 1
    lens = np.full(batch, seq, dtype=np.int64)
    if batch > 1:
        lens[1:] = rng.integers(max(3, seq // 3), seq, size=batch - 1)
    mask = np.arange(seq)[None, :] < lens[:, None]
    ids[:, 0] = CLS_ID
    ids[np.arange(batch), lens - 1] = SEP_ID
    ids[~mask] = PAD_ID
    return ids.astype(np.int32), mask.astype(np.int32)


def synth_pairs(cfg: XlmrCfg, batch: int, seq: int, seed: int):
    """<s> a </s></s> b </s> rows, right-padded, ragged (row 0 is full), the boundary at a different place in every row."""
    ids, mask = synth_tokens(cfg, batch, seq, seed)
    lens = mask.sum(1)
    rng = np.random.default_rng(seed + 7)
    for r in range(batch):
        cut = int(rng.integers(2, lens[r] - 3))
        ids[r, cut] = ids[r, cut + 1] = SEP_ID
    return ids, mask


def hidden_rows(mask: np.ndarray) -> np.ndarray:
    real = np.flatnonzero(mask.reshape(-1))
    if real.size <= HIDDEN_ROWS_CAP:
        return real
    B, S = mask.shape
    lens = mask.sum(1)
    ends = [b * S + j for b in range(B) for j in (0, 1, lens[b] - 2, lens[b] - 1)]
    spread = real[np.linspace(0, real.size - 1, HIDDEN_ROWS_CAP - len(ends)).astype(np.int64)]
    return np.unique(np.concatenate([np.asarray(ends, dtype=np.int64), spread]))


def model_shape(cfg: XlmrCfg, pooling: str = "mean"):
    from rag._encoder import ModelShape
    return ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, pooling, cfg.max_seq,
                      pos_offset=POS_OFFSET)


def write_xlmr_dir(path, tokenizer_json, *, cfg: XlmrCfg = TINY, seed: int = 0, head: bool = False, labels: int = 1,
                   model_type: str = "xlm-roberta", pooling: str = "mean", normalize: bool = True, vocab_size: int = None):
    """A sentence-transformers (head False) or sequence-classification (head True) XLM-RoBERTa directory around the tokenizer.json
    fixture: config.json, model.safetensors (roberta.* and classifier.dense / classifier.out_proj), tokenizer files, and for an
    embedding model modules.json + 1_Pooling.  `vocab_size` shrinks the word table to the fixture's vocabulary."""
    from dataclasses import replace
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    if vocab_size:
        cfg = replace(cfg, vocab_size=vocab_size)
    w = make_ce_weights(cfg, seed) if head else make_weights(cfg, seed)
    if head and labels != 1:
        w[HEAD[2]] = np.repeat(w[HEAD[2]], labels, axis=0)
        w[HEAD[3]] = np.repeat(w[HEAD[3]], labels, axis=0)
    save_file({k: np.ascontiguousarray(v) for k, v in checkpoint_names(w).items()}, os.path.join(path, "model.safetensors"))
    config = {"model_type": model_type, "vocab_size": cfg.vocab_size, "hidden_size": cfg.hidden, "num_hidden_layers": cfg.layers,
              "num_attention_heads": cfg.heads, "intermediate_size": cfg.ffn, "max_position_embeddings": cfg.max_pos,
              "layer_norm_eps": cfg.ln_eps, "type_vocab_size": 1, "pad_token_id": PAD_ID, "bos_token_id": CLS_ID, "eos_token_id": SEP_ID,
              "hidden_act": "gelu"}
    if head:
        config["architectures"] = ["XLMRobertaForSequenceClassification"]
        config["num_labels"] = labels
        config["id2label"] = {str(i): f"LABEL_{i}" for i in range(labels)}
        config["sbert_ce_default_activation_function"] = "torch.nn.modules.linear.Identity"
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(config, fh)
    shutil.copyfile(tokenizer_json, os.path.join(path, "tokenizer.json"))
    with open(os.path.join(path, "special_tokens_map.json"), "w") as fh:
        json.dump({"cls_token": "<s>", "sep_token": "</s>", "pad_token": "<pad>", "unk_token": "<unk>", "bos_token": "<s>", "eos_token": "</s>"}, fh)
    if not head:
        with open(os.path.join(path, "modules.json"), "w") as fh:
            mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                    {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]
            if normalize:
                mods.append({"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"})
            json.dump(mods, fh)
        with open(os.path.join(path, "sentence_bert_config.json"), "w") as fh:
            json.dump({"max_seq_length": cfg.max_seq, "do_lower_case": False}, fh)
        os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
        with open(os.path.join(path, "1_Pooling", "config.json"), "w") as fh:
            json.dump({"word_embedding_dimension": cfg.hidden, "pooling_mode_cls_token": pooling == "cls",
                       "pooling_mode_mean_tokens": pooling == "mean", "pooling_mode_max_tokens": False}, fh)
    return cfg
