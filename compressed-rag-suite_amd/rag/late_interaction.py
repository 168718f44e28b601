"""Late-interaction (ColBERT) re-ranking on the MI355X.

Between the token-overlap rule (cheap, weak) and the cross-encoder (a full forward per (query, chunk) pair): every chunk is encoded
ONCE, at index time, into one small unit vector per token; at query time only the query is encoded, and a pair's score is
``sum_i max_j <q_i, d_j>`` over the query's tokens i and the chunk's tokens j (MaxSim).  Here: the hand-written encoder's final
hidden states (``HipEncoder.forward(..., return_hidden=True)``) -> ``crs_token_project`` (csrc/token_project.hip: the ``linear``
projection, unit length, fp16, packed through a host-built slot table) -> the store's token index (rag/indexing.py,
``VectorStore.token_index``) -> ``crs_maxsim`` (csrc/maxsim.hip), one launch for every candidate list of a device batch.  No CPU
path.

Config keys: ``model_name`` / ``model_path``, ``dim`` (checked against the checkpoint; sizes a synthetic one), ``query_maxlen``
(default 32, at most 64: crs_maxsim holds the query in registers), ``doc_maxlen`` (default 180), ``query_augment`` (default false),
``mask_punctuation`` (default true), ``query_marker`` / ``doc_marker`` (a token string of the vocabulary, a token id, or ''/None for
no marker), ``batch_size`` (texts per encoder forward, default 64), ``device``, ``synthetic_seed``.

Model resolution, offline by construction, as ``CrossEncoderReranker``: a LOCAL BERT directory whose model.safetensors holds
``bert.*`` plus ``linear.weight [dim, H]`` and no bias; else ``$CRS_MODEL_DIR/<basename of model_name>``; else
``synthetic:tiny-colbert`` (hidden 64, 2 layers, dim 32) / ``synthetic:colbert-minilm`` (the MiniLM shape, dim 128): seeded random
weights with a hash tokeniser (plumbing and benchmarks only -- the scores are then meaningless as relevance).  A directory without
``linear.weight`` raises NotImplementedError naming the tensor.  ASSUMPTION: ``bert.*`` + ``linear.weight`` without a bias is the
layout of the ``colbert-ir/colbertv2.0`` checkpoint as its public model card describes it; no such checkpoint was at hand when this
was written, so the loader is tested on directories written by tests/_late_cases.py only.

Token layout: a query is ``[CLS] [Q] q... [SEP]``, a document ``[CLS] [D] d... [SEP]``; the markers default to the vocabulary's
``[unused0]`` / ``[unused1]`` and to none when the vocabulary lacks them (the hash tokeniser has no vocabulary); token type ids are
0; both are truncated to their maxlen (the body is cut, [SEP] stays).

``query_augment: true`` pads the query to ``query_maxlen`` with ``[MASK]`` and ATTENDS to the padding -- ColBERT's
``attend_to_mask_tokens`` variant.  ColBERT's default variant (padding not attended, yet scored) is out of scope: this encoder masks
attention by prefix length, so a position is either inside the sequence (attended and scored) or outside it (neither).

``mask_punctuation``: document tokens whose id is what the tokeniser gives a single ``string.punctuation`` character are dropped
from the index (ColBERT's skiplist); they still take part in the forward.  [CLS], [D] and [SEP] are kept, as in ColBERT.
"""
from __future__ import annotations

import json
import logging
import os
import string
from typing import Dict, List, Optional, Sequence

import numpy as np

from rag import _native as nat
from rag.tokenizer import HashTokenizer, pad_batch

logger = logging.getLogger(__name__)

LINEAR = "linear.weight"
MAX_QUERY = nat.MAXSIM_MAX_QUERY
_KNOWN_LI = {
    "tiny-colbert": (dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=256, pooling="cls", max_seq=256), 32),
    # the all-MiniLM-L6 shape (public config.json) under a 128-dimensional ColBERT head
    "colbert-minilm": (dict(vocab_size=30522, hidden=384, layers=6, heads=12, ffn=1536, max_pos=512, pooling="cls", max_seq=512), 128),
}


def synthetic_li_weights(shape, dim: int, seed: int = 0) -> Dict[str, np.ndarray]:
    """rag.embedding.synthetic_weights plus a seeded ``linear.weight [dim, H]`` (its own PCG64 stream)."""
    from rag.embedding import synthetic_weights
    w = synthetic_weights(shape, seed)
    rng = np.random.Generator(np.random.PCG64([seed, 200000]))
    w[LINEAR] = (rng.standard_normal((dim, shape.hidden), dtype=np.float32) / np.sqrt(shape.hidden)).astype(np.float32)
    return w


def load_late_interaction_dir(path: str):
    """(ModelShape, weights dict under BertModel names + linear.weight, tokenizer, config dict) from a ColBERT checkpoint
    directory: config.json (model_type bert), model.safetensors with ``bert.*`` and ``linear.weight``, vocab.txt or tokenizer.json."""
    from safetensors.numpy import load_file
    from rag._encoder import ModelShape
    from rag.tokenizer import tokenizer_from_model_dir
    with open(os.path.join(path, "config.json")) as fh:
        cfg = json.load(fh)
    if cfg.get("model_type", "bert") != "bert":
        raise NotImplementedError(f"late-interaction model_type '{cfg.get('model_type')}' is not supported (bert is)")
    raw = load_file(os.path.join(path, "model.safetensors"))
    weights = {(k[5:] if k.startswith("bert.") else k): np.asarray(v, dtype=np.float32) for k, v in raw.items()}
    if LINEAR not in weights:
        raise NotImplementedError(f"{path}: not a ColBERT checkpoint, {LINEAR} missing (a late-interaction model needs bert.* and "
                                  f"{LINEAR} [dim, hidden]; bge-m3's colbert_linear.pt and PyLate's 1_Dense layouts are not read)")
    if weights[LINEAR].ndim != 2 or weights[LINEAR].shape[1] != cfg["hidden_size"]:
        raise ValueError(f"{path}: {LINEAR} must be [dim, {cfg['hidden_size']}], got {weights[LINEAR].shape}")
    max_pos = cfg["max_position_embeddings"]
    shape = ModelShape(cfg["vocab_size"], cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"],
                       cfg["intermediate_size"], max_pos, cfg.get("layer_norm_eps", 1e-12), "cls", max_pos)
    return shape, weights, tokenizer_from_model_dir(path), cfg


def token_id_of(tokenizer, piece) -> Optional[int]:
    """The id of a vocabulary piece (None when the tokeniser has no vocabulary or lacks it); an int is taken as the id itself."""
    if piece is None or piece == "":
        return None
    if isinstance(piece, (int, np.integer)) and not isinstance(piece, bool):
        return int(piece)
    vocab = getattr(tokenizer, "vocab", None)
    if isinstance(vocab, dict):
        return vocab.get(piece)
    inner = getattr(tokenizer, "_tok", None)
    if inner is not None and hasattr(inner, "token_to_id"):
        return inner.token_to_id(piece)
    return None


class LateInteractionReranker:
    """Encodes queries and documents into per-token vectors and scores (query, store row) pairs by MaxSim on the GPU."""

    def __init__(self, config):
        if isinstance(config, str):
            config = {"model_name": config}
        self.model_name = config.get("model_name") or config.get("model_path") or ""
        self.batch_size = int(config.get("batch_size", 64))
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.query_maxlen = int(config.get("query_maxlen", 32))
        if not 3 <= self.query_maxlen <= MAX_QUERY:
            raise ValueError(f"query_maxlen must be in 3..{MAX_QUERY} (crs_maxsim holds the query in registers), got {self.query_maxlen}")
        shape, weights, self.tokenizer, _cfg = self._resolve(config)
        self.dim = int(weights[LINEAR].shape[0])
        if config.get("dim") is not None and int(config["dim"]) != self.dim:
            raise ValueError(f"dim {config['dim']} does not match the checkpoint's {LINEAR} [{self.dim}, {shape.hidden}]")
        if not 1 <= self.dim <= 128:
            raise ValueError(f"dim must be in 1..128, got {self.dim}")
        self.dimp = nat.token_dim_padded(self.dim)
        limit = min(shape.max_seq, shape.max_pos - shape.pos_offset)
        self.doc_maxlen = min(int(config.get("doc_maxlen", 180)), limit)
        if self.doc_maxlen < 3 or self.query_maxlen > limit:
            raise ValueError(f"doc_maxlen must be >= 3 and query_maxlen <= {limit} (the model's positions)")
        self.query_augment = bool(config.get("query_augment", False))
        self.mask_punctuation = bool(config.get("mask_punctuation", True))
        tok = self.tokenizer
        self.query_marker = token_id_of(tok, config["query_marker"] if "query_marker" in config else "[unused0]")
        self.doc_marker = token_id_of(tok, config["doc_marker"] if "doc_marker" in config else "[unused1]")
        self.mask_id = token_id_of(tok, config.get("mask_token", "[MASK]"))
        if self.mask_id is None:          # no vocabulary: BERT's id beside BERT's [CLS] / [SEP], else the padding id
            self.mask_id = 103 if getattr(tok, "cls_id", None) == 101 else int(getattr(tok, "pad_id", 0))
        self.skip_ids = self._punctuation_ids() if self.mask_punctuation else frozenset()
        self.shape = shape
        self._weights, self._device_pref = weights, config.get("device")
        self._model = self._w16 = None
        self.doc_forwards = 0             # encoder forwards run for documents (the tests count them)
        self.docs_encoded = 0             # documents those forwards held

    def _resolve(self, config: dict):
        from rag._encoder import ModelShape
        name = self.model_name
        model_dir = os.environ.get("CRS_MODEL_DIR")
        for cand in (config.get("model_path"), name, os.path.join(model_dir, os.path.basename(name)) if model_dir and name else None):
            if cand and os.path.isdir(cand) and os.path.exists(os.path.join(cand, "model.safetensors")):
                logger.info(f"Loading local late-interaction model {cand}")
                return load_late_interaction_dir(cand)
        if name.startswith("synthetic:") and name.split(":", 1)[1].lower() in _KNOWN_LI:
            key = name.split(":", 1)[1].lower()
            logger.warning(f"Using SYNTHETIC weights for late-interaction model '{key}' (no checkpoint available offline)")
            known, dim = _KNOWN_LI[key]
            shape = ModelShape(**{"ln_eps": 1e-12, **known})
            dim = int(config.get("dim") or dim)
            return shape, synthetic_li_weights(shape, dim, int(config.get("synthetic_seed", 0))), HashTokenizer(shape.vocab_size), {}
        raise FileNotFoundError(
            f"No local late-interaction model for '{name}': pass a ColBERT checkpoint directory (bert.* + {LINEAR}) as "
            f"model_name/model_path, set CRS_MODEL_DIR, or use 'synthetic:tiny-colbert' / 'synthetic:colbert-minilm' (models cannot be "
            f"downloaded here)")

    def _punctuation_ids(self) -> frozenset:
        """The ids the tokeniser gives the single characters of string.punctuation (ColBERT's skiplist), the unknown id left out."""
        tok = self.tokenizer
        out = set()
        for ch in string.punctuation:
            ids = tok.encode_body(ch)
            if len(ids) == 1:
                out.add(int(ids[0]))
        unk = getattr(tok, "unk_id", None)
        if unk is None:                   # the `tokenizers`-backed classes keep the unknown token inside their model
            inner = getattr(getattr(tok, "_tok", None), "model", None)
            unk = next((i for i in (token_id_of(tok, t) for t in (getattr(inner, "unk_token", None), "[UNK]", "<unk>")) if i is not None), None)
        out.discard(unk)
        return frozenset(out)

    @property
    def model(self):
        """The HipEncoder, uploaded on first use together with the fp16 projection (construction needs no GPU)."""
        if self._model is None:
            import torch
            from rag._encoder import HipEncoder
            nat.require_gpu()
            w = {k: v for k, v in self._weights.items() if k != LINEAR}
            self._model = HipEncoder(self.shape, w, device=self._device_pref if str(self._device_pref or "").startswith("cuda") else None)
            self._w16 = torch.from_numpy(np.ascontiguousarray(self._weights[LINEAR], dtype=np.float32)).to(self._model.device).to(torch.float16).contiguous()
            self._weights = None
        return self._model

    @property
    def device(self):
        return self.model.device

    # ---- tokenisation ----------------------------------------------------------------------------------------------------------
    def _frame(self, body: Sequence[int], marker: Optional[int], maxlen: int) -> List[int]:
        tok = self.tokenizer
        head = [tok.cls_id] + ([marker] if marker is not None else [])
        return head + list(body[: maxlen - len(head) - 1]) + [tok.sep_id]

    def tokenize_queries(self, texts: Sequence[str]) -> List[List[int]]:
        """[CLS] [Q] q... [SEP] per query, cut to query_maxlen; with query_augment padded to query_maxlen with [MASK]."""
        out = []
        for t in texts:
            ids = self._frame(self.tokenizer.encode_body(str(t).strip()), self.query_marker, self.query_maxlen)
            if self.query_augment:
                ids = ids + [self.mask_id] * (self.query_maxlen - len(ids))
            out.append(ids)
        return out

    def tokenize_docs(self, texts: Sequence[str]) -> List[List[int]]:
        """[CLS] [D] d... [SEP] per document, cut to doc_maxlen.  Nothing is cached: a caller that needs the ids twice (the store's
        size guard, then the encoding) passes them on (doc_token_counts / encode_docs_device take `ids`)."""
        return [self._frame(self.tokenizer.encode_body(str(t).strip()), self.doc_marker, self.doc_maxlen) for t in texts]

    def keep_mask(self, ids: Sequence[int]) -> np.ndarray:
        """bool [len(ids)]: the document tokens that enter the index (all but the punctuation ids of the skiplist)."""
        if not self.skip_ids:
            return np.ones(len(ids), dtype=bool)
        return np.fromiter((i not in self.skip_ids for i in ids), dtype=bool, count=len(ids))

    def doc_token_counts(self, texts: Sequence[str], ids: Optional[Sequence[Sequence[int]]] = None) -> np.ndarray:
        """int64 [n]: index tokens of each document, from the host tokenisation alone (the store's size guard); `ids`: the
        documents' token ids when the caller already has them (tokenize_docs)."""
        ids = self.tokenize_docs(texts) if ids is None else ids
        return np.asarray([int(self.keep_mask(t).sum()) for t in ids], dtype=np.int64)

    @staticmethod
    def dst_table(keeps: Sequence[np.ndarray], width: int, first_slots: Sequence[int]) -> np.ndarray:
        """int64 [len(keeps), width]: output slot of every position of a padded batch -- document b's kept tokens get
        first_slots[b], first_slots[b] + 1, ... in token order; dropped tokens and padding get -1."""
        dst = np.full((len(keeps), width), -1, dtype=np.int64)
        for b, (keep, first) in enumerate(zip(keeps, first_slots)):
            at = np.flatnonzero(keep)
            dst[b, at] = int(first) + np.arange(at.size)
        return dst

    # ---- encoding --------------------------------------------------------------------------------------------------------------
    def _project(self, ids: np.ndarray, lens: np.ndarray, dst: np.ndarray, out16):
        import torch
        model = self.model
        _, hidden = model.forward(ids, lens, normalize=False, return_hidden=True)
        if dst.size and int(dst.max()) >= out16.shape[0]:
            raise ValueError("slot table leaves the output array")
        nat.token_project(hidden.view(-1, self.shape.hidden), self._w16, None, torch.from_numpy(dst.reshape(-1)).to(model.device), out16)

    def encode_queries_device(self, texts: Sequence[str]):
        """(q16 cuda fp16 [n, lq_max, dimp], q_len cuda int32 [n]): lq_max the longest query of the call; rows at and past q_len
        are zeros.  One encoder forward per batch_size queries."""
        import torch
        model = self.model
        ids = self.tokenize_queries(texts)
        n = len(ids)
        lq_max = max((len(t) for t in ids), default=1)
        q16 = torch.zeros((n, lq_max, self.dimp), dtype=torch.float16, device=model.device)
        lens_all = np.asarray([len(t) for t in ids], dtype=np.int32)
        pad = getattr(self.tokenizer, "pad_id", 0)
        flat = q16.view(n * lq_max, self.dimp)
        for lo in range(0, n, self.batch_size):
            b_ids, lens = pad_batch(ids[lo: lo + self.batch_size], pad)
            keeps = [np.ones(int(l), dtype=bool) for l in lens]
            dst = self.dst_table(keeps, b_ids.shape[1], [(lo + b) * lq_max for b in range(len(keeps))])
            self._project(b_ids, lens, dst, flat)
        return q16, torch.from_numpy(lens_all).to(model.device)

    def encode_docs_device(self, texts: Sequence[str], ids: Optional[Sequence[Sequence[int]]] = None, out=None, first_slot: int = 0):
        """(tok16 cuda fp16 [T, dimp], counts cuda int32 [n]): the documents' index tokens one after the other in INPUT order.
        Processed longest first (equal lengths by their ids) in batches of batch_size, each batch padded to its longest, and
        scattered back through the host-built slot table.  `ids`: the documents' token ids when the caller already has them.
        `out` (cuda fp16 [>= first_slot + T, dimp]): write the T rows there from row first_slot on instead of into a new array
        (the store's token index: no temporary copy of the new rows); the returned tok16 is then that slice of `out`."""
        import torch
        model = self.model
        ids = self.tokenize_docs(texts) if ids is None else ids
        n = len(ids)
        keeps = [self.keep_mask(t) for t in ids]
        counts = np.asarray([int(k.sum()) for k in keeps], dtype=np.int64)
        first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=first[1:])
        first += int(first_slot)
        total = int(first[-1])
        if out is None:
            out = torch.zeros((total, self.dimp), dtype=torch.float16, device=model.device)
        elif out.dtype != torch.float16 or out.dim() != 2 or out.shape[1] != self.dimp or out.shape[0] < total or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous fp16 [>= {total}, {self.dimp}] array")
        order = sorted(range(n), key=lambda i: (-len(ids[i]), ids[i]))
        pad = getattr(self.tokenizer, "pad_id", 0)
        for lo in range(0, n, self.batch_size):
            sel = order[lo: lo + self.batch_size]
            b_ids, lens = pad_batch([ids[i] for i in sel], pad)
            dst = self.dst_table([keeps[i] for i in sel], b_ids.shape[1], [first[i] for i in sel])
            self._project(b_ids, lens, dst, out)
            self.doc_forwards += 1
            self.docs_encoded += len(sel)
        return out[int(first_slot):total], torch.from_numpy(counts.astype(np.int32)).to(model.device)

    # ---- scoring ---------------------------------------------------------------------------------------------------------------
    def score_rows(self, queries: Sequence[str], rows, store):
        """cuda fp32 [nq, m_max]: the MaxSim score of each query against each of its candidate sidecar rows (int64 [nq, m_max], a
        negative row = empty slot, scored -inf) over the store's token index, in ONE crs_maxsim launch."""
        import torch
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.ndim != 2 or rows.shape[0] != len(queries) or rows.shape[1] < 1:
            raise ValueError("rows must be int64 [len(queries), m_max >= 1]")
        index = store.token_index(self)
        dev = index.device
        with torch.cuda.device(dev):
            q16, q_len = self.encode_queries_device(queries)
            return nat.maxsim(q16, q_len, index.tok16, index.n_tokens, index.offsets_dev, index.n_rows, torch.from_numpy(rows).to(dev))
