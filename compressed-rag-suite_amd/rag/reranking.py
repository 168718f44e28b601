"""Cross-encoder re-ranking on the MI355X.

What users of a retrieve-then-read pipeline mean by ``rerank: true``: a BERT sequence classifier reads
``[CLS] query [SEP] chunk [SEP]`` and emits one relevance logit (``cross-encoder/ms-marco-MiniLM-L-6-v2`` and its L-12 /
TinyBERT siblings; sentence-transformers' ``CrossEncoder.predict``).  Here: host WordPiece pair encoding
(rag/tokenizer.py ``join_pair``) -> ``crs_encoder_score_pairs`` (the hand-written encoder's layer stack with per-token type
ids, then the pooler + classifier head kernel; csrc/enc_misc.hip, csrc/enc_pair.hip).  No CPU path.

Config keys: ``model_name`` / ``model_path``, ``batch_size`` (pairs per launch, default 128), ``max_seq_length``,
``activation`` (``'auto' | 'identity' | 'sigmoid'``), ``device``, ``synthetic_seed``.

Model resolution, offline by construction, as ``EmbeddingModel``: a LOCAL directory (config.json with ``model_type: bert`` and
one label, model.safetensors with ``bert.*`` + ``bert.pooler.dense.*`` + ``classifier.*``, vocab.txt or tokenizer.json); else
``$CRS_MODEL_DIR/<basename of model_name>``; else ``synthetic:tiny-ce`` / ``synthetic:minilm-ce``: seeded random weights with a
hash tokeniser (plumbing and benchmarks only -- the scores are then meaningless as relevance).  Anything else raises.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from rag import _native as nat
from rag.tokenizer import HashTokenizer, join_pair, pad_batch

logger = logging.getLogger(__name__)

_KNOWN_CE = {
    "tiny-ce": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=64, pooling="cls", max_seq=64),
    # cross-encoder/ms-marco-MiniLM-L-6-v2 (public model card / config.json)
    "minilm-ce": dict(vocab_size=30522, hidden=384, layers=6, heads=12, ffn=1536, max_pos=512, pooling="cls", max_seq=512),
    # tiny-ce as an XLM-RoBERTa classifier: position ids from 2, pairs <s> a </s></s> b </s> with every type id 0
    "tiny-xlmr-ce": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=66, pooling="cls", max_seq=64, ln_eps=1e-5,
                         pos_offset=2),
}
_HEAD = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")
# XLMRobertaForSequenceClassification's head -> the internal names (classifier.dense first: classifier.out_proj shares its prefix)
_XLMR_HEAD_NAMES = {"classifier.dense.": "pooler.dense.", "classifier.out_proj.": "classifier."}


def synthetic_ce_weights(shape, seed: int = 0) -> Dict[str, np.ndarray]:
    """rag.embedding.synthetic_weights (two token-type rows) plus a seeded pooler and a one-label classifier, one PCG64
    stream per tensor; the encoder's tensors are the ones an embedding model of this shape and seed gets."""
    from rag.embedding import synthetic_weights
    w = synthetic_weights(shape, seed)
    h = shape.hidden
    for idx, (name, shp, scale) in enumerate(((_HEAD[0], (h, h), 0.05), (_HEAD[1], (h,), 0.02), (_HEAD[2], (1, h), 0.2),
                                              (_HEAD[3], (1,), 0.02))):
        rng = np.random.Generator(np.random.PCG64([seed, 100000 + idx]))
        w[name] = (scale * rng.standard_normal(shp, dtype=np.float32)).astype(np.float32)
    return w


def resolve_activation(setting: str, cfg: dict) -> str:
    """'identity' or 'sigmoid'.  'auto' follows sentence-transformers' CrossEncoder: config.json's
    sbert_ce_default_activation_function (a class path: one ending in 'Identity' gives logits, one ending in 'Sigmoid' the
    sigmoid); an absent key gives the sigmoid, its default for one label."""
    if setting in ("identity", "sigmoid"):
        return setting
    if setting != "auto":
        raise ValueError(f"activation must be 'auto', 'identity' or 'sigmoid', got {setting!r}")
    name = (cfg or {}).get("sbert_ce_default_activation_function")
    if not name:
        return "sigmoid"
    tail = str(name).rsplit(".", 1)[-1]
    if tail.endswith("Identity"):
        return "identity"
    if tail.endswith("Sigmoid"):
        return "sigmoid"
    raise NotImplementedError(f"cross-encoder activation '{name}' is not supported (Identity and Sigmoid are)")


def load_cross_encoder_dir(path: str):
    """(ModelShape, weights dict under BertModel names + pooler.dense.* + classifier.*, tokenizer, config dict) from a
    BertForSequenceClassification directory, as CrossEncoder(path) reads it."""
    from safetensors.numpy import load_file
    from rag._encoder import ModelShape
    from rag.tokenizer import tokenizer_from_model_dir
    with open(os.path.join(path, "config.json")) as fh:
        cfg = json.load(fh)
    model_type = cfg.get("model_type", "bert")
    if model_type not in ("bert", "xlm-roberta"):
        raise NotImplementedError(f"cross-encoder model_type '{model_type}' is not supported (bert and xlm-roberta are: RoBERTa "
                                  f"cross-encoders need a byte-level BPE tokenizer, MPNet ones have no token types)")
    labels = cfg.get("num_labels")
    if labels is None:
        labels = len(cfg["id2label"]) if "id2label" in cfg else 2          # transformers' default is two labels
    if int(labels) != 1:
        raise NotImplementedError(f"cross-encoder with {labels} labels is not supported (one relevance label is)")
    raw = load_file(os.path.join(path, "model.safetensors"))
    pos_offset = 0
    if model_type == "xlm-roberta":
        # RobertaClassificationHead (classifier.dense -> tanh -> classifier.out_proj on <s>) is the pooler + classifier head
        # under other names; such checkpoints ship no roberta.pooler and need none
        weights = {}
        for k, v in raw.items():
            for old, new in _XLMR_HEAD_NAMES.items():
                if k.startswith(old):
                    k = new + k[len(old):]
                    break
            else:
                k = k[8:] if k.startswith("roberta.") else k
            weights[k] = np.asarray(v, dtype=np.float32)
        pos_offset = int(cfg.get("pad_token_id", 1)) + 1
    else:
        weights = {(k[5:] if k.startswith("bert.") else k): np.asarray(v, dtype=np.float32) for k, v in raw.items()}
    missing = [n for n in _HEAD if n not in weights]
    if missing:
        raise NotImplementedError(f"{path}: not a BERT or XLM-RoBERTa sequence classifier, {', '.join(missing)} missing "
                                  f"(a cross-encoder needs bert.pooler.dense.* and classifier.*, or classifier.dense.* and "
                                  f"classifier.out_proj.*)")
    if weights["classifier.weight"].shape[0] != 1:
        raise NotImplementedError(f"cross-encoder with {weights['classifier.weight'].shape[0]} labels is not supported (one relevance label is)")
    max_pos = cfg["max_position_embeddings"]
    shape = ModelShape(cfg["vocab_size"], cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"],
                       cfg["intermediate_size"], max_pos, cfg.get("layer_norm_eps", 1e-12 if model_type == "bert" else 1e-5), "cls",
                       max_pos - pos_offset, pos_offset=pos_offset)
    return shape, weights, tokenizer_from_model_dir(path), cfg


class CrossEncoderReranker:
    """Scores (query, text) pairs with a BERT cross-encoder on the GPU."""

    TOKEN_CACHE_CAP = 65536           # texts; the cache is dropped whole when it passes this

    def __init__(self, config):
        if isinstance(config, str):
            config = {"model_name": config}
        self.model_name = config.get("model_name") or config.get("model_path") or ""
        self.batch_size = int(config.get("batch_size", 128))
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        shape, weights, self.tokenizer, cfg = self._resolve(config)
        if config.get("max_seq_length"):
            from dataclasses import replace
            shape = replace(shape, max_seq=min(int(config["max_seq_length"]), shape.max_pos - shape.pos_offset))
        if shape.max_seq < 5:
            raise ValueError("max_seq_length must be >= 5 for sentence pairs")
        self.activation = resolve_activation(config.get("activation", "auto"), cfg)
        self.shape = shape
        self._weights, self._device_pref = weights, config.get("device")
        self._model = None
        # special tokens of a pair: 3 in [CLS] a [SEP] b [SEP], 4 in XLM-RoBERTa's <s> a </s></s> b </s>
        self._pair_seps, self._pair_typed = getattr(self.tokenizer, "pair_seps", 1), getattr(self.tokenizer, "pair_typed", True)
        self._tokens: Dict[str, Tuple[List[int], int]] = {}   # text -> (its first max_seq - specials token ids, its full token count)

    def _resolve(self, config: dict):
        from rag._encoder import ModelShape
        name = self.model_name
        model_dir = os.environ.get("CRS_MODEL_DIR")
        for cand in (config.get("model_path"), name, os.path.join(model_dir, os.path.basename(name)) if model_dir and name else None):
            if cand and os.path.isdir(cand) and os.path.exists(os.path.join(cand, "model.safetensors")):
                logger.info(f"Loading local cross-encoder {cand}")
                return load_cross_encoder_dir(cand)
        if name.startswith("synthetic:") and name.split(":", 1)[1].lower() in _KNOWN_CE:
            key = name.split(":", 1)[1].lower()
            logger.warning(f"Using SYNTHETIC weights for cross-encoder '{key}' (no checkpoint available offline)")
            shape = ModelShape(**{"ln_eps": 1e-12, **_KNOWN_CE[key]})
            # a random model has no trained activation: logits, as the ms-marco checkpoints are configured
            cfg = {"sbert_ce_default_activation_function": "torch.nn.modules.linear.Identity"}
            tok = (HashTokenizer(shape.vocab_size, special=(0, 2, 1), pair_seps=2, pair_typed=False) if shape.pos_offset
                   else HashTokenizer(shape.vocab_size))
            return shape, synthetic_ce_weights(shape, int(config.get("synthetic_seed", 0))), tok, cfg
        raise FileNotFoundError(
            f"No local cross-encoder for '{name}': pass a BertForSequenceClassification directory as model_name/model_path, "
            f"set CRS_MODEL_DIR, or use 'synthetic:tiny-ce' / 'synthetic:minilm-ce' / 'synthetic:tiny-xlmr-ce' (models cannot be "
            f"downloaded here)")

    @property
    def model(self):
        """The HipEncoder with the pair head, uploaded on first use (construction needs no GPU)."""
        if self._model is None:
            from rag._encoder import HipEncoder
            nat.require_gpu()
            self._model = HipEncoder(self.shape, self._weights, device=self._device_pref if str(self._device_pref or "").startswith("cuda") else None)
            self._weights = None
        return self._model

    # ---- tokenisation ----------------------------------------------------------------------------------------------------------
    def _body(self, text: str) -> Tuple[List[int], int]:
        got = self._tokens.get(text)
        if got is None:
            if len(self._tokens) >= self.TOKEN_CACHE_CAP:
                self._tokens.clear()
            ids = self.tokenizer.encode_body(str(text).strip())
            got = self._tokens[text] = (ids[: self.shape.max_seq - 2 - self._pair_seps], len(ids))
        return got

    def tokenize_pairs(self, pairs: Sequence[Tuple[str, str]]):
        """-> (list of id lists, list of type-id lists): [CLS] a [SEP] b [SEP] per pair, truncated 'longest_first' to max_seq."""
        tok, out_ids, out_types = self.tokenizer, [], []
        for a, b in pairs:
            (ia, na), (ib, nb) = self._body(a), self._body(b)
            ids, types = join_pair(ia, ib, tok.cls_id, tok.sep_id, self.shape.max_seq, na, nb, seps=self._pair_seps, typed=self._pair_typed)
            out_ids.append(ids)
            out_types.append(types)
        return out_ids, out_types

    # ---- scoring ---------------------------------------------------------------------------------------------------------------
    def predict_device(self, pairs: Sequence[Tuple[str, str]]):
        """Scores as a cuda fp32 tensor [n] in input order: pairs sorted longest first, one score_pairs call per batch_size of
        them (padded to the batch's longest, type ids padded with 0), scattered back."""
        import torch
        model = self.model
        n = len(pairs)
        out = torch.empty((n,), dtype=torch.float32, device=model.device)
        if n == 0:
            return out
        ids, types = self.tokenize_pairs(pairs)
        # longest first, equal lengths by their ids: the batches depend on the set of pairs, not on the order they came in
        order = sorted(range(n), key=lambda i: (-len(ids[i]), ids[i]))
        pad = getattr(self.tokenizer, "pad_id", 0)
        for lo in range(0, n, self.batch_size):
            sel = order[lo: lo + self.batch_size]
            b_ids, lens = pad_batch([ids[i] for i in sel], pad)
            b_types, _ = pad_batch([types[i] for i in sel], 0)
            scores = model.score_pairs(b_ids, b_types, lens, activation=self.activation)
            out[torch.as_tensor(sel, device=out.device)] = scores
        return out

    def predict(self, pairs: Sequence[Tuple[str, str]]) -> np.ndarray:
        """np.float32 [n]: one relevance score per (query, text) pair, in input order."""
        return self.predict_device(pairs).cpu().numpy()
