"""Learned sparse retrieval (SPLADE) on the MI355X.

A learned sparse encoder is a ``BertForMaskedLM`` checkpoint: its output for a text is one non-negative weight per vocabulary id,
``w_v = max_i log(1 + relu(logit_iv))`` over the text's real tokens, and the relevance of a document to a query is the dot product
of the two sparse vectors.  Here: the hand-written encoder's final hidden states (``HipEncoder.forward(..., return_hidden=True)``)
-> ``crs_mlm_sparse_pool`` (csrc/mlm_pool.hip: the MLM head whose vocabulary projection max-pools in its epilogue, so the
[tokens, V] logits never exist) -> ``crs_sparse_compact`` (csrc/sparse_compact.hip: the dense row to at most ``max_terms``
(id, weight) pairs in id order, on the device) -> the store's sparse index (rag/indexing.py, ``VectorStore.sparse_index``) ->
``crs_sparse_topk`` (csrc/sparse_scan.hip).  No CPU path.

Config keys: ``model_name`` / ``model_path``, ``batch_size`` (texts per encoder forward, default 64), ``max_seq`` (default: the
model's), ``tokenize`` ('host' | 'device', as rag.embedding), ``device``, ``synthetic_seed``, ``bias_shift`` (synthetic models only).

Model resolution, offline by construction, as ``LateInteractionReranker``: a LOCAL BertForMaskedLM directory whose
model.safetensors holds ``bert.*``, ``cls.predictions.transform.dense.{weight,bias}``,
``cls.predictions.transform.LayerNorm.{weight,bias}``, ``cls.predictions.bias`` (or ``cls.predictions.decoder.bias``) and
``cls.predictions.decoder.weight`` (tied to ``bert.embeddings.word_embeddings.weight`` when absent); else
``$CRS_MODEL_DIR/<basename of model_name>``; else ``synthetic:tiny-splade`` (hidden 64, 2 layers, 1000 ids) /
``synthetic:splade-base`` (the bge-base shape, 30522 ids): seeded random weights with a hash tokeniser and a tied decoder (plumbing
and benchmarks only).  Random MLM logits are positive about half the time, nothing like a trained model's, so the synthetic decoder
bias is shifted down by ``bias_shift`` standard deviations of a logit (default 3.0): a text then activates a few to a few dozen
ids (tests/test_sparse_cpu.py checks that on the fp64 reference).  DistilBERT-named checkpoints (``vocab_transform`` ...) and
bge-m3's sparse head are not read: a directory without the tensors above raises NotImplementedError naming the missing ones.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from rag import _native as nat
from rag.tokenizer import HashTokenizer, pad_batch

logger = logging.getLogger(__name__)

T_DENSE_W, T_DENSE_B = "cls.predictions.transform.dense.weight", "cls.predictions.transform.dense.bias"
T_LN_W, T_LN_B = "cls.predictions.transform.LayerNorm.weight", "cls.predictions.transform.LayerNorm.bias"
DEC_W, DEC_B = "cls.predictions.decoder.weight", "cls.predictions.bias"
DEC_B_ALT = "cls.predictions.decoder.bias"
WORD_EMB = "embeddings.word_embeddings.weight"
HEAD = (T_DENSE_W, T_DENSE_B, T_LN_W, T_LN_B, DEC_W, DEC_B)

_KNOWN_SPARSE = {
    "tiny-splade": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=64, pooling="cls", max_seq=64),
    # the bge-base-en-v1.5 shape (public config.json) under a tied MLM head
    "splade-base": dict(vocab_size=30522, hidden=768, layers=12, heads=12, ffn=3072, max_pos=512, pooling="cls", max_seq=512),
}


def synthetic_sparse_weights(shape, seed: int = 0, bias_shift: float = 3.0) -> Dict[str, np.ndarray]:
    """rag.embedding.synthetic_weights plus a seeded MLM head (its own PCG64 streams): transform dense ~ N(0, 1 / H), LayerNorm
    near identity, the decoder tied to the word embeddings (scale 0.05), and a decoder bias of N(0, 0.02) shifted down by
    ``bias_shift`` standard deviations of a logit (sqrt(H) x 0.05: the transform's output has unit variance per element)."""
    from rag.embedding import synthetic_weights
    w = synthetic_weights(shape, seed)
    h = shape.hidden
    rng = [np.random.Generator(np.random.PCG64([seed, 300000 + i])) for i in range(5)]
    w[T_DENSE_W] = (rng[0].standard_normal((h, h), dtype=np.float32) / np.sqrt(h)).astype(np.float32)
    w[T_DENSE_B] = (0.02 * rng[1].standard_normal(h, dtype=np.float32)).astype(np.float32)
    w[T_LN_W] = (1.0 + 0.05 * rng[2].standard_normal(h, dtype=np.float32)).astype(np.float32)
    w[T_LN_B] = (0.02 * rng[3].standard_normal(h, dtype=np.float32)).astype(np.float32)
    w[DEC_W] = w[WORD_EMB]
    w[DEC_B] = (0.02 * rng[4].standard_normal(shape.vocab_size, dtype=np.float32) - float(bias_shift) * np.sqrt(h) * 0.05).astype(np.float32)
    return w


def map_mlm_tensors(raw: Dict[str, np.ndarray], where: str = "checkpoint") -> Dict[str, np.ndarray]:
    """A BertForMaskedLM state dict under the internal names: ``bert.`` stripped, the head's six tensors under HEAD's names
    (``cls.predictions.decoder.bias`` read as ``cls.predictions.bias``; a missing decoder weight tied to the word embeddings).
    NotImplementedError naming what is missing."""
    out = {(k[5:] if k.startswith("bert.") else k): np.asarray(v, dtype=np.float32) for k, v in raw.items()}
    if DEC_B not in out and DEC_B_ALT in out:
        out[DEC_B] = out[DEC_B_ALT]
    out.pop(DEC_B_ALT, None)
    if DEC_W not in out and WORD_EMB in out:
        out[DEC_W] = out[WORD_EMB]                     # tie_word_embeddings: safetensors keeps one copy
    missing = [n for n in HEAD + (WORD_EMB,) if n not in out]
    if missing:
        raise NotImplementedError(f"{where}: not a BertForMaskedLM checkpoint, missing {', '.join(missing)} (a learned sparse encoder "
                                  f"needs bert.* and the cls.predictions.* head; DistilBERT-named checkpoints and bge-m3's sparse "
                                  f"head are not read)")
    return out


def load_sparse_dir(path: str):
    """(ModelShape, weights dict under the internal names, tokenizer, config dict) from a BertForMaskedLM checkpoint directory:
    config.json (model_type bert), model.safetensors, vocab.txt or tokenizer.json."""
    from safetensors.numpy import load_file
    from rag._encoder import ModelShape
    from rag.tokenizer import tokenizer_from_model_dir
    with open(os.path.join(path, "config.json")) as fh:
        cfg = json.load(fh)
    if cfg.get("model_type", "bert") != "bert":
        raise NotImplementedError(f"sparse-encoder model_type '{cfg.get('model_type')}' is not supported (bert is)")
    weights = map_mlm_tensors(load_file(os.path.join(path, "model.safetensors")), path)
    h, v = cfg["hidden_size"], cfg["vocab_size"]
    want = {T_DENSE_W: (h, h), T_DENSE_B: (h,), T_LN_W: (h,), T_LN_B: (h,), DEC_W: (v, h), DEC_B: (v,)}
    for name, shp in want.items():
        if tuple(weights[name].shape) != shp:
            raise ValueError(f"{path}: {name} must be {shp}, got {tuple(weights[name].shape)}")
    if cfg.get("hidden_act", "gelu") != "gelu":
        raise NotImplementedError(f"{path}: hidden_act '{cfg.get('hidden_act')}' is not supported (the head's transform is erf-GELU)")
    max_pos = cfg["max_position_embeddings"]
    shape = ModelShape(v, h, cfg["num_hidden_layers"], cfg["num_attention_heads"], cfg["intermediate_size"], max_pos,
                       cfg.get("layer_norm_eps", 1e-12), "cls", max_pos)
    return shape, weights, tokenizer_from_model_dir(path), cfg


class SparseEncoder:
    """Encodes texts into bounded sparse vectors over the model's vocabulary, on the GPU."""

    def __init__(self, config):
        if isinstance(config, str):
            config = {"model_name": config}
        self.model_name = config.get("model_name") or config.get("model_path") or ""
        self.batch_size = int(config.get("batch_size", 64))
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.tokenize_mode = config.get("tokenize", "host")
        if self.tokenize_mode not in ("host", "device"):
            raise ValueError(f"tokenize must be 'host' or 'device', got {self.tokenize_mode!r}")
        shape, weights, self.tokenizer, _cfg = self._resolve(config)
        nat.mlm_pool_plan(1, 1, shape.hidden, shape.vocab_size)                   # NativeError for a shape the head kernel lacks
        limit = min(shape.max_seq, shape.max_pos - shape.pos_offset)
        self.max_seq = min(int(config.get("max_seq", limit)), limit)
        if self.max_seq < 3:
            raise ValueError("max_seq must be >= 3")
        self.shape = shape
        self.vocab_size = shape.vocab_size
        tok = self.tokenizer
        self.skip_ids = sorted({int(i) for i in (getattr(tok, "cls_id", None), getattr(tok, "sep_id", None), getattr(tok, "pad_id", None))
                                if i is not None and 0 <= int(i) < shape.vocab_size})
        self._device_tokenizer = None
        if self.tokenize_mode == "device":
            from rag._unigram import tokenizer_spec
            tokenizer_spec(self.tokenizer)             # NotImplementedError for a tokenizer the kernel does not restate
        self._weights, self._device_pref = weights, config.get("device")
        self._model = self._head = None
        self._mlm_ws = None
        self.forwards = 0                              # encoder forwards run (the tests count them)
        self.texts_encoded = 0                         # texts those forwards held

    def _resolve(self, config: dict):
        from rag._encoder import ModelShape
        name = self.model_name
        model_dir = os.environ.get("CRS_MODEL_DIR")
        for cand in (config.get("model_path"), name, os.path.join(model_dir, os.path.basename(name)) if model_dir and name else None):
            if cand and os.path.isdir(cand) and os.path.exists(os.path.join(cand, "model.safetensors")):
                logger.info(f"Loading local sparse encoder {cand}")
                return load_sparse_dir(cand)
        if name.startswith("synthetic:") and name.split(":", 1)[1].lower() in _KNOWN_SPARSE:
            key = name.split(":", 1)[1].lower()
            logger.warning(f"Using SYNTHETIC weights for sparse encoder '{key}' (no checkpoint available offline)")
            shape = ModelShape(**{"ln_eps": 1e-12, **_KNOWN_SPARSE[key]})
            weights = synthetic_sparse_weights(shape, int(config.get("synthetic_seed", 0)), float(config.get("bias_shift", 3.0)))
            return shape, weights, HashTokenizer(shape.vocab_size), {}
        raise FileNotFoundError(
            f"No local sparse encoder for '{name}': pass a BertForMaskedLM checkpoint directory (bert.* + cls.predictions.*) as "
            f"model_name/model_path, set CRS_MODEL_DIR, or use 'synthetic:tiny-splade' / 'synthetic:splade-base' (models cannot be "
            f"downloaded here)")

    @property
    def model(self):
        """The HipEncoder, uploaded on first use together with the head's tensors (construction needs no GPU)."""
        if self._model is None:
            import torch
            from rag._encoder import HipEncoder
            nat.require_gpu()
            w = self._weights
            self._model = HipEncoder(self.shape, {k: v for k, v in w.items() if k not in HEAD},
                                     device=self._device_pref if str(self._device_pref or "").startswith("cuda") else None)
            dev = self._model.device

            def up(name, half=False):
                t = torch.from_numpy(np.ascontiguousarray(w[name], dtype=np.float32)).to(dev)
                return t.to(torch.float16).contiguous() if half else t

            self._head = dict(w_t=up(T_DENSE_W, True), b_t=up(T_DENSE_B), gamma=up(T_LN_W), beta=up(T_LN_B), w_d=up(DEC_W, True),
                              bias=up(DEC_B), skip=torch.tensor(self.skip_ids, dtype=torch.int32, device=dev) if self.skip_ids else None)
            self._weights = None
        return self._model

    @property
    def device(self):
        return self.model.device

    # ---- tokenisation ----------------------------------------------------------------------------------------------------------
    def tokenize(self, texts: Sequence[str]) -> List[List[int]]:
        """[CLS] ids [SEP] per text, cut to max_seq (the encoder's own rule: rag.embedding.EmbeddingModel.tokenize)."""
        texts = [str(t).strip() for t in texts]
        if hasattr(self.tokenizer, "encode_batch"):
            return self.tokenizer.encode_batch(texts, self.max_seq)
        return [self.tokenizer.encode(t, self.max_seq) for t in texts]

    def _tokenize_device(self, texts, timings=None):
        """(ids cuda int32 [n, max_seq], lens host int32 [n]) from the device tokeniser: rag.embedding.tokenize_on_device."""
        from rag._unigram import device_tokenizer
        from rag.embedding import tokenize_on_device
        dev = self.model.device
        if self._device_tokenizer is None:
            self._device_tokenizer = device_tokenizer(self.tokenizer, dev)
        return tokenize_on_device(self._device_tokenizer, self.tokenizer, dev, list(texts), self.max_seq, self.tokenize, timings=timings)

    # ---- encoding --------------------------------------------------------------------------------------------------------------
    def _width(self, longest: int) -> int:
        for step in (16, 32, 64):
            if longest <= step <= self.max_seq:
                return step
        return longest

    def _head_batch(self, ids, lens, dense):
        """One encoder forward and the head: ids int32 [b, width] (numpy or cuda), lens int32 [b] -> dense[:b] cuda fp32 [b, V]."""
        import torch
        model, hd = self.model, self._head
        b, width = int(ids.shape[0]), int(ids.shape[1])
        _, hidden = model.forward(ids, lens, normalize=False, return_hidden=True)
        lens_d = lens if isinstance(lens, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(model.device)
        need = nat.mlm_workspace_bytes(b, width, self.shape.hidden, self.vocab_size)
        if self._mlm_ws is None or self._mlm_ws.numel() < need:
            self._mlm_ws = torch.empty(need, dtype=torch.uint8, device=model.device)
        nat.mlm_sparse_pool(hidden, lens_d.to(torch.int32), hd["w_t"], hd["b_t"], hd["gamma"], hd["beta"], self.shape.ln_eps, hd["w_d"],
                            hd["bias"], self.shape.max_pos - self.shape.pos_offset, self._mlm_ws, dense[:b])
        self.forwards += 1
        self.texts_encoded += b
        return b, width

    def encode_device(self, texts: Sequence[str], max_terms: int):
        """(ids cuda int32 [n, max_terms], weights cuda fp32 [n, max_terms], counts cuda int32 [n]) in INPUT order: per text its
        at most max_terms largest positive weights (ties by lower id) in ascending id order, the special tokens [CLS] / [SEP] /
        [PAD] always dropped, unused slots (-1, 0).  Processed longest first in batches of batch_size, each padded to its longest
        (16 / 32 / 64 when it fits).  No host synchronisation beyond what tokenisation needs."""
        import torch
        if not isinstance(max_terms, (int, np.integer)) or isinstance(max_terms, bool) or not 1 <= max_terms <= nat.SPARSE_MAX_TERMS:
            raise ValueError(f"max_terms must be an integer in 1..{nat.SPARSE_MAX_TERMS}, got {max_terms!r}")
        texts = list(texts)
        n, cap = len(texts), int(max_terms)
        model = self.model
        dev = model.device
        out = (torch.full((n, cap), -1, dtype=torch.int32, device=dev), torch.zeros((n, cap), dtype=torch.float32, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev))
        if n == 0:
            return out
        with torch.cuda.device(dev):
            if self.tokenize_mode == "device":
                ids_all, lens_h = self._tokenize_device(texts)
                lens_all = torch.from_numpy(lens_h).to(dev)
                order = sorted(range(n), key=lambda i: -len(texts[i]))
            else:
                token_ids = self.tokenize(texts)
                lens_h = np.asarray([len(t) for t in token_ids], dtype=np.int32)
                order = sorted(range(n), key=lambda i: (-len(token_ids[i]), i))
            dense = torch.empty((min(n, self.batch_size), self.vocab_size), dtype=torch.float32, device=dev)
            pad = getattr(self.tokenizer, "pad_id", 0)
            for lo in range(0, n, self.batch_size):
                sel = order[lo: lo + self.batch_size]
                sel_t = torch.as_tensor(sel, device=dev)
                if self.tokenize_mode == "device":
                    width = self._width(int(lens_h[sel].max()))
                    ids, lens = ids_all[sel_t, :width].contiguous(), lens_all[sel_t]
                else:
                    ids, lens = pad_batch([token_ids[i] for i in sel], pad, short_steps=tuple(s for s in (16, 32, 64) if s <= self.max_seq))
                b, width = self._head_batch(ids, lens, dense)
                got = nat.sparse_compact(dense[:b], self.vocab_size, cap, self._head["skip"])
                for dst, src in zip(out, got):
                    dst[sel_t] = src
        return out

    def encode_docs_device(self, texts: Sequence[str], max_terms: int = 256):
        """encode_device for documents: up to 256 terms a text by default."""
        return self.encode_device(texts, max_terms)

    def encode_queries_device(self, texts: Sequence[str], max_terms: int = 64):
        """encode_device for queries: up to 64 terms by default, so that 64 queries always fit one crs_sparse_topk launch
        (64 x 64 = CRS_BM25_MAX_PAIRS)."""
        return self.encode_device(texts, max_terms)

    def head_tensors(self) -> Dict[str, "object"]:
        """The head's device tensors (w_t, b_t, gamma, beta, w_d, bias, skip), for parity tests and benches."""
        self.model
        return dict(self._head)
