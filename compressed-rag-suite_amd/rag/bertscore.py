"""BERTScore on the MI355X: the reference's answer-quality metric (evaluation/retrieval/rag_metrics.py:58-67,179-207 calls
``bert_score.score(predictions, references, lang=..., model_type=...)``) without the ``bert_score`` package.

What the package does per (candidate, reference) pair -- encode both sentences with a BERT-family model, keep the hidden
states of layer L, take the cosine of every token pair, the row and column maxima, and two weighted means -- is here:
``HipEncoder`` built with only the first L layers of the checkpoint (the package's ``model.encoder.layer[:num_layers]``; the
pooled output is ignored) and one launch of ``crs_token_match`` (csrc/token_match.hip) per batch of pairs.  fp32 matching
arithmetic, as in the package; no CPU fallback.

``score(cands, refs, lang='en', model_type=None, ...)`` is usable as ``RAGMetrics.bert_score_fn``; ``BertScorer(config)`` is the
object behind it (``score_device`` / ``score`` / ``mean_scores``).

Models, offline by construction: ``model_path`` / ``model_name`` name a plain HuggingFace directory (config.json,
model.safetensors, tokenizer files), else ``$CRS_MODEL_DIR/<basename of model_name>`` is tried, as ``EmbeddingModel`` does;
``synthetic:tiny`` / ``synthetic:minilm`` give seeded weights with a hash tokeniser (plumbing only).  ``model_type`` ``bert``
and ``roberta`` are loaded (``load_hf_dir``); RoBERTa is BERT's layer stack with position ids from ``pad_token_id + 1`` and a
one-row token-type table.

``MODEL_LAYERS`` holds the layer the ``bert_score`` package publishes for each model (its ``model2layers`` table, tuned on
WMT16 to-English Pearson correlation) for the four models the reference's tables need; any other model must pass
``num_layers``.

Weights follow the package: without idf every real token weighs 1 and the two special tokens 0 (they stay match targets);
``idf=<reference sentences>`` weighs a token by log((N + 1) / (df + 1)), log(N + 1) when unseen, 0 for the specials.  A pair
with an empty sentence scores P = R = F = 0.

One deviation: the package multiplies the similarities of padded positions by 0, so in a padded batch a token whose best
real cosine is negative scores 0 there, depending on its batch mates.  Here padding is excluded outright, so a pair's score
does not depend on its batch.  ``rescale_with_baseline`` raises NotImplementedError: the baseline files are not shipped.

Parity with the ``bert_score`` package itself is UNPINNED: the package is not installed where this was built or tested.
The tests pin the matching kernel against fp64 numpy and the whole scorer against ``transformers`` BertModel / RobertaModel
hidden states in fp64 with a plain restatement of the formulas above (tests/golden/bertscore.npz).
"""
from __future__ import annotations

import json
import logging
import math
import os
from collections import Counter
from dataclasses import replace
from typing import Dict, List, Optional, Sequence

import numpy as np

from rag import _native as nat

logger = logging.getLogger(__name__)

# model -> the hidden-state layer bert_score uses by default (bert_score/utils.py model2layers)
MODEL_LAYERS = {"bert-base-uncased": 9, "bert-large-uncased": 18, "roberta-base": 10, "roberta-large": 17}
LANG_MODELS = {"en": "roberta-large"}          # bert_score's lang2model, the entry the reference's default reaches
MAX_SEQ = 512                                   # crs_token_match's longest side
_SYNTHETIC = ("tiny", "minilm")


class _JsonTokenizer:
    """A `tokenizers.Tokenizer` behind the encode / encode_batch interface of rag.tokenizer (single sentences with the
    model's special tokens, truncated to max_len tokens in all)."""

    def __init__(self, tok, cls_id: int, sep_id: int, pad_id: int):
        self._tok, self.cls_id, self.sep_id, self.pad_id = tok, cls_id, sep_id, pad_id
        self._max_len = None
        tok.no_padding()

    def _limit(self, max_len: int):
        if self._max_len != max_len:
            self._tok.enable_truncation(max_length=max_len)
            self._max_len = max_len

    def encode(self, text: str, max_len: int) -> List[int]:
        self._limit(max_len)
        return self._tok.encode(text).ids

    def encode_batch(self, texts: Sequence[str], max_len: int) -> List[List[int]]:
        self._limit(max_len)
        return [e.ids for e in self._tok.encode_batch(list(texts))]


def _roberta_tokenizer(path: str, cfg: dict):
    """tokenizer.json as shipped, else vocab.json + merges.txt as a byte-level BPE with RobertaProcessing -- what
    transformers.RobertaTokenizerFast builds from the same files."""
    try:
        from tokenizers import AddedToken, Tokenizer, decoders, pre_tokenizers, processors
        from tokenizers.models import BPE
    except ImportError as e:
        raise NotImplementedError("a RoBERTa tokenizer needs the `tokenizers` library, which is not importable") from e
    names = {"cls": "<s>", "sep": "</s>", "pad": "<pad>", "unk": "<unk>", "mask": "<mask>"}
    sm = os.path.join(path, "special_tokens_map.json")
    if os.path.exists(sm):
        with open(sm, encoding="utf-8") as fh:
            m = json.load(fh)
        for key in names:
            v = m.get(key + "_token")
            v = v.get("content") if isinstance(v, dict) else v
            if isinstance(v, str):
                names[key] = v
    tj = os.path.join(path, "tokenizer.json")
    if os.path.exists(tj):
        tok = Tokenizer.from_file(tj)
    else:
        vj, mt = os.path.join(path, "vocab.json"), os.path.join(path, "merges.txt")
        if not (os.path.exists(vj) and os.path.exists(mt)):
            raise FileNotFoundError(f"{path}: no tokenizer.json and no vocab.json + merges.txt")
        tok = Tokenizer(BPE.from_file(vj, mt, continuing_subword_prefix="", end_of_word_suffix="", fuse_unk=False))
        tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
        tok.decoder = decoders.ByteLevel()
        specials = [AddedToken(names[k], normalized=False, special=True) for k in ("cls", "pad", "sep", "unk", "mask")]
        tok.add_special_tokens([t for t in specials if tok.token_to_id(t.content) is not None])
        tok.post_processor = processors.RobertaProcessing(sep=(names["sep"], tok.token_to_id(names["sep"])),
                                                          cls=(names["cls"], tok.token_to_id(names["cls"])),
                                                          trim_offsets=True, add_prefix_space=False)
    cls_id, sep_id = tok.token_to_id(names["cls"]), tok.token_to_id(names["sep"])
    if cls_id is None or sep_id is None:
        raise ValueError(f"{path}: the tokenizer has no {names['cls']} / {names['sep']}")
    pad_id = tok.token_to_id(names["pad"])
    return _JsonTokenizer(tok, cls_id, sep_id, pad_id if pad_id is not None else int(cfg.get("pad_token_id", 1)))


def load_hf_dir(path: str):
    """(ModelShape with the checkpoint's full layer count, weights under the internal BertModel names, tokenizer) from a plain
    HuggingFace directory: config.json, model.safetensors and tokenizer files.  model_type `bert`: tensor prefix `bert.` or
    none, WordPiece from tokenizer.json or vocab.txt (rag.tokenizer.tokenizer_from_model_dir).  `roberta`: prefix `roberta.`
    or none, position ids from pad_token_id + 1, the one-row token-type table, layer_norm_eps from the config, byte-level
    BPE through the `tokenizers` library.  Anything else raises NotImplementedError."""
    from rag._encoder import ModelShape
    with open(os.path.join(path, "config.json")) as fh:
        cfg = json.load(fh)
    model_type = cfg.get("model_type", "bert")
    if model_type not in ("bert", "roberta"):
        raise NotImplementedError(f"model_type '{model_type}' is not supported by BertScorer (bert and roberta are)")
    pos_offset = int(cfg.get("pad_token_id", 1)) + 1 if model_type == "roberta" else 0
    max_pos = int(cfg["max_position_embeddings"])
    shape = ModelShape(cfg["vocab_size"], cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"],
                       cfg["intermediate_size"], max_pos, float(cfg.get("layer_norm_eps", 1e-5 if model_type == "roberta" else 1e-12)),
                       "mean", min(MAX_SEQ, max_pos - pos_offset), pos_offset=pos_offset)
    if model_type == "roberta":
        tokenizer = _roberta_tokenizer(path, cfg)
    else:
        from rag.tokenizer import tokenizer_from_model_dir
        tokenizer = tokenizer_from_model_dir(path)
    from safetensors.numpy import load_file
    raw = load_file(os.path.join(path, "model.safetensors"))
    prefix = model_type + "."
    weights = {(k[len(prefix):] if k.startswith(prefix) else k): v for k, v in raw.items()}
    return shape, weights, tokenizer


def idf_weights(token_lists: Sequence[Sequence[int]], specials: Sequence[int]):
    """The package's idf table from the tokenised reference sentences: id -> log((N + 1) / (df + 1)), with df the number of
    sentences holding the id; the special tokens weigh 0.  -> (dict, default for unseen ids = log(N + 1))."""
    n = len(token_lists)
    df = Counter()
    for ids in token_lists:
        df.update(set(ids))
    table = {t: math.log((n + 1) / (c + 1)) for t, c in df.items()}
    for s in specials:
        table[s] = 0.0
    return table, math.log(n + 1)


def sentence_weights(ids: Sequence[int], idf=None) -> List[float]:
    """Weights of one tokenised sentence (special tokens first and last): 1 per token, or its idf value with `idf` = the pair
    idf_weights returns; 0 on the two special tokens."""
    if idf is None:
        w = [1.0] * len(ids)
    else:
        table, default = idf
        w = [table.get(t, default) for t in ids]
    if w:
        w[0] = 0.0
        w[-1] = 0.0
    return w


class BertScorer:
    """BERTScore P / R / F1 of (candidate, reference) pairs on the GPU.  Config keys: model_name / model_path, num_layers,
    batch_size (64), idf (False, or the list of reference sentences the idf table is built from), max_seq_length, device."""

    def __init__(self, config: Optional[dict] = None, *, shape=None, weights=None, tokenizer=None):
        config = dict(config or {})
        if config.get("rescale_with_baseline"):
            raise NotImplementedError("rescale_with_baseline needs bert_score's baseline files, which are not shipped here")
        self.model_name = config.get("model_name") or LANG_MODELS["en"]
        self.batch_size = max(1, int(config.get("batch_size", 64)))
        if shape is None:
            shape, weights, tokenizer = self._resolve(config)
        key = os.path.basename(os.path.normpath(self.model_name))
        num_layers = config.get("num_layers")
        if num_layers is None:
            if key not in MODEL_LAYERS:
                raise ValueError(f"no published BERTScore layer for '{self.model_name}': pass num_layers (known: {sorted(MODEL_LAYERS)})")
            num_layers = MODEL_LAYERS[key]
        num_layers = int(num_layers)
        if not 1 <= num_layers <= shape.layers:
            raise ValueError(f"num_layers must be in 1..{shape.layers} for '{self.model_name}', got {num_layers}")
        self.num_layers = num_layers
        max_seq = min(MAX_SEQ, shape.max_pos - shape.pos_offset)
        if config.get("max_seq_length"):
            max_seq = min(max_seq, int(config["max_seq_length"]))
        if max_seq < 2:
            raise ValueError("max_seq_length must leave room for the two special tokens")
        self.shape = replace(shape, layers=num_layers, max_seq=max_seq)
        self.tokenizer = tokenizer
        self._idf = None
        idf = config.get("idf")
        if idf is not None and idf is not False:
            if isinstance(idf, (str, bytes)) or idf is True or not hasattr(idf, "__len__"):
                raise ValueError("idf must be False or the list of reference sentences to build the table from")
            self._idf = idf_weights(self.tokenize(list(idf)), (tokenizer.cls_id, tokenizer.sep_id))
        # only layers < num_layers are read from `weights`; a pooler / classifier head is not this model's business
        from rag._encoder import HEAD_NAMES, HipEncoder
        nat.require_gpu()
        device = config.get("device") or "cuda"
        if not str(device).startswith("cuda"):
            logger.warning(f"device '{device}' requested; this build only runs on the GPU ('cuda')")
            device = "cuda"
        self.model = HipEncoder(self.shape, {k: v for k, v in weights.items() if k not in HEAD_NAMES}, device=device)
        self.device = self.model.device

    def _resolve(self, config: dict):
        name = self.model_name
        model_dir = os.environ.get("CRS_MODEL_DIR")
        for cand in (config.get("model_path"), name, os.path.join(model_dir, os.path.basename(name)) if model_dir else None):
            if cand and os.path.isdir(cand) and os.path.exists(os.path.join(cand, "model.safetensors")):
                logger.info(f"Loading local checkpoint {cand}")
                return load_hf_dir(cand)
        if name.startswith("synthetic:") and name.split(":", 1)[1].lower() in _SYNTHETIC:
            from rag._encoder import ModelShape
            from rag.embedding import _ALIASES, _KNOWN, synthetic_weights
            from rag.tokenizer import HashTokenizer
            key = name.split(":", 1)[1].lower()
            logger.warning(f"Using SYNTHETIC weights for architecture '{key}' (no checkpoint available offline)")
            shape = ModelShape(**{"ln_eps": 1e-12, **_KNOWN[_ALIASES.get(key, key)]})
            return shape, synthetic_weights(shape, int(config.get("synthetic_seed", 0))), HashTokenizer(shape.vocab_size)
        raise FileNotFoundError(
            f"No local checkpoint for '{name}': pass a HuggingFace directory as model_name/model_path, "
            f"set CRS_MODEL_DIR, or use 'synthetic:tiny' (models cannot be downloaded here)")

    # ---- host side -----------------------------------------------------------------------------
    def tokenize(self, texts: Sequence[str]) -> List[List[int]]:
        """-> id lists with the model's two special tokens, truncated to max_seq; text is stripped first, as the package does."""
        texts = [str(t).strip() for t in texts]
        if hasattr(self.tokenizer, "encode_batch"):
            return self.tokenizer.encode_batch(texts, self.shape.max_seq)
        return [self.tokenizer.encode(t, self.shape.max_seq) for t in texts]

    def token_weights(self, ids: Sequence[int]) -> List[float]:
        """Weights of one tokenised sentence (sentence_weights with this scorer's idf table)."""
        return sentence_weights(ids, self._idf)

    # ---- device side ---------------------------------------------------------------------------
    def score_ids_device(self, ids_a, len_a, ids_b, len_b, w_a=None, w_b=None):
        """One batch from token ids: ids int32 [n, seq] (right padded), lens int32 [n], weights fp32 [n, seq] or None (1 on
        real tokens, 0 on the first and last one) -> cuda fp32 [n, 3].  A pair with a side of two tokens or fewer (an
        empty sentence) scores 0."""
        import torch
        ids_a, ids_b = np.ascontiguousarray(ids_a, dtype=np.int32), np.ascontiguousarray(ids_b, dtype=np.int32)
        len_a, len_b = np.ascontiguousarray(len_a, dtype=np.int32), np.ascontiguousarray(len_b, dtype=np.int32)
        n = ids_a.shape[0]
        if n == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self.device)

        def default_w(lens, seq):
            w = (np.arange(seq)[None, :] < lens[:, None]).astype(np.float32)
            w[:, 0] = 0.0
            w[np.arange(n), np.maximum(lens, 1) - 1] = 0.0
            return w

        w_a = default_w(len_a, ids_a.shape[1]) if w_a is None else np.ascontiguousarray(w_a, dtype=np.float32)
        w_b = default_w(len_b, ids_b.shape[1]) if w_b is None else np.ascontiguousarray(w_b, dtype=np.float32)
        _, ha = self.model.forward(ids_a, np.maximum(len_a, 1), normalize=False, return_hidden=True)
        _, hb = self.model.forward(ids_b, np.maximum(len_b, 1), normalize=False, return_hidden=True)
        empty = (len_a <= 2) | (len_b <= 2)
        dev = lambda a: torch.from_numpy(a).to(self.device)
        return nat.token_match(ha, dev(np.where(empty, 0, len_a).astype(np.int32)), hb, dev(np.where(empty, 0, len_b).astype(np.int32)),
                               dev(w_a), dev(w_b))

    def score_device(self, cands: Sequence[str], refs: Sequence[str]):
        """P, R, F1 of each (candidate, reference) pair as a cuda fp32 tensor [n, 3], in input order."""
        import torch
        from rag.tokenizer import pad_batch
        if isinstance(cands, str) or isinstance(refs, str):
            raise TypeError("cands and refs are lists of sentences")
        if len(cands) != len(refs):
            raise ValueError(f"{len(cands)} candidates but {len(refs)} references (one reference per candidate)")
        n = len(cands)
        out = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        ta, tb = self.tokenize(cands), self.tokenize(refs)
        order = sorted(range(n), key=lambda i: -(len(ta[i]) + len(tb[i])))      # longest first: least padding per batch
        steps = tuple(st for st in (16, 32, 64) if st <= self.shape.max_seq)
        pad_id = getattr(self.tokenizer, "pad_id", 0)

        def padded(rows):
            ids, lens = pad_batch(rows, pad_id, short_steps=steps)
            w = np.zeros(ids.shape, dtype=np.float32)
            for r, row in enumerate(rows):
                w[r, :len(row)] = self.token_weights(row)
            return ids, lens, w

        for lo in range(0, n, self.batch_size):
            sel = order[lo: lo + self.batch_size]
            ids_a, len_a, w_a = padded([ta[i] for i in sel])
            ids_b, len_b, w_b = padded([tb[i] for i in sel])
            res = self.score_ids_device(ids_a, len_a, ids_b, len_b, w_a, w_b)
            if len(sel) == n and sel == list(range(n)):
                return res
            out[torch.as_tensor(sel, device=self.device)] = res
        return out

    def score(self, cands: Sequence[str], refs: Sequence[str]):
        """(P, R, F1), each numpy fp32 [n]."""
        res = self.score_device(cands, refs).cpu().numpy()
        return res[:, 0].copy(), res[:, 1].copy(), res[:, 2].copy()

    def mean_scores(self, cands: Sequence[str], refs: Sequence[str]) -> Optional[Dict[str, float]]:
        """{'precision', 'recall', 'f1'}: the dict RAGMetrics.bertscore returns (rag_metrics.py:200-204); None for empty input."""
        if len(cands) == 0:
            return None
        p, r, f = self.score(cands, refs)
        return {"precision": float(p.mean()), "recall": float(r.mean()), "f1": float(f.mean())}


_SCORERS: Dict[tuple, BertScorer] = {}


def score(cands, refs, lang="en", verbose=False, model_type=None, num_layers=None, idf=False, batch_size=64, **kw):
    """Drop-in for ``bert_score.score`` as the reference calls it: -> (P, R, F1), three CPU torch tensors [n].
    ``model_type=None`` means the model of ``lang`` ('en': roberta-large), resolved through ``model_path`` (keyword) /
    ``CRS_MODEL_DIR``.  ``idf=True`` builds the table from ``refs``; a list of sentences is used as given.  Scorers without
    idf are kept per (model, layer) for the next call."""
    import torch
    if kw.get("rescale_with_baseline"):
        raise NotImplementedError("rescale_with_baseline needs bert_score's baseline files, which are not shipped here")
    if kw.get("all_layers"):
        raise NotImplementedError("all_layers is not supported")
    if model_type is None:
        if lang not in LANG_MODELS:
            raise ValueError(f"no default model for lang '{lang}': pass model_type")
        model_type = LANG_MODELS[lang]
    config = {"model_name": model_type, "model_path": kw.get("model_path"), "num_layers": num_layers, "batch_size": batch_size,
              "device": kw.get("device"), "max_seq_length": kw.get("max_seq_length"), "synthetic_seed": kw.get("synthetic_seed", 0)}
    if idf is not False and idf is not None:
        scorer = BertScorer({**config, "idf": list(refs) if idf is True else idf})
    else:
        key = (model_type, kw.get("model_path"), num_layers, kw.get("max_seq_length"), kw.get("synthetic_seed", 0))
        scorer = _SCORERS.get(key)
        if scorer is None:
            scorer = _SCORERS[key] = BertScorer(config)
        scorer.batch_size = max(1, int(batch_size))
    res = scorer.score_device(cands, refs).cpu()
    return res[:, 0].clone(), res[:, 1].clone(), res[:, 2].clone()
