"""Text embedding generation on the MI355X.

Drop-in for the reference's ``EmbeddingModel`` (/root/reference/rag/embedding.py:14-91): same
config keys (``model_name``, ``device``, ``batch_size``, ``normalize``), same methods and return
types (``embed`` -> float32 numpy [n, d]; a single string gives [1, d]).  Underneath, what
sentence-transformers did (tokenise -> BertModel -> pooling -> normalise) is: host WordPiece ->
``crs_encoder_forward`` (hand-written HIP: MFMA GEMMs, fused attention, fp32 LayerNorm / pooling).

Model resolution, offline by construction (the reference fetches by hub name, which cannot work
here): ``model_path`` (additive key) or ``model_name`` may be a LOCAL sentence-transformers
directory (config.json, model.safetensors, vocab.txt, optional sentence_bert_config.json and
1_Pooling/config.json); else ``$CRS_MODEL_DIR/<basename of model_name>`` is tried; else, when
``model_name`` is ``synthetic:<minilm|bge|tiny|mpnet|tiny-mpnet|tiny-xlmr|multilingual-minilm|multilingual-e5-base|tiny-nomic|nomic-embed-text|tiny-modernbert|modernbert-base>`` or ``CRS_ALLOW_SYNTHETIC_WEIGHTS=1`` is set,
seeded random weights of the named architecture are used with a hash tokeniser (plumbing and
benchmarks only -- embeddings are then meaningless as language).  Anything else raises.

Task prefixes (additive keys ``query_prefix`` / ``document_prefix``, default ""): models trained with them (nomic-embed-text:
"search_query: " / "search_document: "; E5: "query: " / "passage: ") get the prefix prepended to every text of that kind before
tokenisation; ``embed`` / ``embed_device`` / ``tokenize`` / ``tokenize_device`` take ``kind=None | 'query' | 'document'`` and the
chunk methods are 'document'.  Nothing is read from config_sentence_transformers.json.
"""
from __future__ import annotations

import json
import logging
import os
from typing import Dict, List, Optional, Union

import numpy as np

from rag.chunking import Chunk
from rag import _native as nat
from rag.tokenizer import HashTokenizer, WordPieceTokenizer, make_wordpiece_tokenizer, pad_batch

logger = logging.getLogger(__name__)

# architectures this build knows by name (public model cards; SURVEY.md section 2.3 shapes)
_KNOWN = {
    "all-minilm-l6-v2": dict(vocab_size=30522, hidden=384, layers=6, heads=12, ffn=1536, max_pos=512,
                             pooling="mean", max_seq=256),
    "bge-base-en-v1.5": dict(vocab_size=30522, hidden=768, layers=12, heads=12, ffn=3072, max_pos=512,
                             pooling="cls", max_seq=512),
    "tiny": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=64, pooling="mean", max_seq=64),
    # MPNet: BERT's layer stack + a bucketed relative-position bias in attention; position ids start at 2 (max_pos rows
    # in the table, the first two unused), no token types, <s> </s> <pad> <unk> in the WordPiece vocabulary
    "all-mpnet-base-v2": dict(vocab_size=30527, hidden=768, layers=12, heads=12, ffn=3072, max_pos=514, pooling="mean",
                              max_seq=384, ln_eps=1e-5, rel_buckets=32, pos_offset=2),
    "tiny-mpnet": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=66, pooling="mean", max_seq=64,
                       rel_buckets=32, pos_offset=2),
    # XLM-RoBERTa: BERT's layer stack, position ids from 2, one token-type row, <s> <pad> </s> <unk> in a SentencePiece Unigram
    # vocabulary.  The two real shapes (paraphrase-multilingual-MiniLM-L12-v2, intfloat/multilingual-e5-base) are quoted from
    # memory of the public config.json files: they only size synthetic weights
    "tiny-xlmr": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=66, pooling="mean", max_seq=64,
                      ln_eps=1e-5, pos_offset=2),
    "multilingual-minilm": dict(vocab_size=250037, hidden=384, layers=12, heads=12, ffn=1536, max_pos=514, pooling="mean",
                                max_seq=128, ln_eps=1e-5, pos_offset=2),
    "multilingual-e5-base": dict(vocab_size=250002, hidden=768, layers=12, heads=12, ffn=3072, max_pos=514, pooling="mean",
                                 max_seq=512, ln_eps=1e-5, pos_offset=2),
    # nomic-embed-text-v1 / v1.5: BERT's post-LayerNorm layer order and WordPiece vocabulary, rotary Q / K (base 1000) in place of a
    # position table, SwiGLU feed-forward, no biases; published with 8192 positions (trained to 2048)
    "tiny-nomic": dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=128, pooling="mean", max_seq=128,
                       rotary_theta=1000.0, gated=True),
    "nomic-embed-text": dict(vocab_size=30528, hidden=768, layers=12, heads=12, ffn=3072, max_pos=8192, pooling="mean", max_seq=512,
                             rotary_theta=1000.0, gated=True),
    # ModernBERT (nomic-ai/modernbert-embed-base, Alibaba-NLP/gte-modernbert-base, answerdotai/ModernBERT-base): pre-norm layers,
    # every third layer attends the whole sequence (rope base 160000) and the others a +-64 window (base 10000), GeGLU, no biases,
    # byte-level BPE vocabulary of 50368 ids, 8192 positions
    "tiny-modernbert": dict(vocab_size=1000, hidden=64, layers=4, heads=4, ffn=128, max_pos=256, pooling="mean", max_seq=256,
                            ln_eps=1e-5, rotary_theta=160000.0, local_theta=10000.0, prenorm=True, gelu_gated=True, window=8, global_every=3),
    "modernbert-base": dict(vocab_size=50368, hidden=768, layers=22, heads=12, ffn=1152, max_pos=8192, pooling="mean", max_seq=8192,
                            ln_eps=1e-5, rotary_theta=160000.0, local_theta=10000.0, prenorm=True, gelu_gated=True, window=64, global_every=3),
}
_ALIASES = {"minilm": "all-minilm-l6-v2", "bge": "bge-base-en-v1.5", "bge-base": "bge-base-en-v1.5", "mpnet": "all-mpnet-base-v2",
            "nomic": "nomic-embed-text", "nomic-embed-text-v1": "nomic-embed-text", "nomic-embed-text-v1.5": "nomic-embed-text",
            "modernbert": "modernbert-base", "modernbert-embed-base": "modernbert-base", "gte-modernbert-base": "modernbert-base"}
REL_BIAS = "encoder.relative_attention_bias.weight"      # [buckets, heads], shared by all layers (MPNet)


TOKENIZE_GROUP_BYTES = 64 << 20      # UTF-8 bytes of one crs_wordpiece_encode launch (and one lens / flags read-back)


def tokenize_on_device(device_tok, tokenizer, dev, texts: List[str], max_seq: int, host_tokenize, pre_lower: bool = False,
                       group_bytes: int = TOKENIZE_GROUP_BYTES, timings: Optional[dict] = None):
    """(ids cuda int32 [n, max_seq], lens as a host int32 array [n]): the device tokeniser `device_tok` (rag._unigram.device_tokenizer
    of `tokenizer`) on groups of texts bounded by group_bytes, one launch and one read-back of lens / flags per group; the texts
    the kernel flags (a code point outside its table's reach) go through host_tokenize(texts) -> id lists and their rows are
    written in.  Shared by EmbeddingModel and rag.sparse.SparseEncoder."""
    import time
    import torch
    texts = [str(t).strip() for t in texts]
    if pre_lower:
        texts = [t.lower() for t in texts]
    pad = getattr(tokenizer, "pad_id", 0)
    ids_parts, lens_parts, lo = [], [], 0
    while lo < len(texts):
        hi, size = lo, 0
        while hi < len(texts) and (hi == lo or size + len(texts[hi]) <= group_bytes // 4):   # <= 4 bytes a character
            size += len(texts[hi])
            hi += 1
        ids, lens, flags, host = device_tok.encode(texts[lo:hi], max_seq, timings)
        t0 = time.perf_counter()
        back = torch.stack((lens, flags)).cpu().numpy()
        if timings is not None:
            timings["readback_s"] = timings.get("readback_s", 0.0) + (time.perf_counter() - t0)
        lens_h = back[0].copy()
        redo = sorted(set(np.nonzero(back[1])[0].tolist()) | set(host))
        if redo:
            rows, rlen = pad_batch(host_tokenize([texts[lo + i] for i in redo]), pad)
            block = np.full((len(redo), max_seq), pad, dtype=np.int32)
            block[:, : rows.shape[1]] = rows
            ids[torch.as_tensor(redo, device=dev)] = torch.from_numpy(block).to(dev)
            lens_h[redo] = rlen
        ids_parts.append(ids)
        lens_parts.append(lens_h)
        lo = hi
    if not ids_parts:
        return torch.empty((0, max_seq), dtype=torch.int32, device=dev), np.zeros(0, dtype=np.int32)
    return (ids_parts[0] if len(ids_parts) == 1 else torch.cat(ids_parts)), np.concatenate(lens_parts)


def synthetic_weights(shape, seed: int = 0, scale: float = 0.05) -> Dict[str, np.ndarray]:
    """Seeded random checkpoint with HuggingFace BertModel tensor names (one PCG64 stream per tensor).  Shapes with
    `rel_buckets` (MPNet) also get the relative-position bias table (~N(0, 0.5): real tables are O(1)) and, having no
    token types, a zero token-type table.  Gated (nomic) shapes: NomicBertModel's names, query / key projections ~N(0, 1 / hidden)."""
    h, f = shape.hidden, shape.ffn
    if getattr(shape, "prenorm", False):    # ModernBERT under ModernBertModel's names: no position table, no token types, no biases
        names = [("embeddings.tok_embeddings.weight", (shape.vocab_size, h)), ("embeddings.norm.weight", (h,))]
        for i in range(shape.layers):
            p = f"layers.{i}."
            names += ([(p + "attn_norm.weight", (h,))] if i else []) + [
                (p + "attn.Wqkv.weight", (3 * h, h)), (p + "attn.Wo.weight", (h, h)), (p + "mlp_norm.weight", (h,)),
                (p + "mlp.Wi.weight", (2 * f, h)), (p + "mlp.Wo.weight", (h, f))]
        names.append(("final_norm.weight", (h,)))
        out = {}
        for idx, (name, shp) in enumerate(names):
            rng = np.random.Generator(np.random.PCG64([seed, idx]))
            if name.endswith("norm.weight"):
                a = 1.0 + 0.05 * rng.standard_normal(shp, dtype=np.float32)
            else:
                a = scale * rng.standard_normal(shp, dtype=np.float32)
                if name.endswith("attn.Wqkv.weight"):      # query / key rows ~N(0, 1 / h), as for the nomic shapes below
                    a[: 2 * h] = h ** -0.5 * rng.standard_normal((2 * h, h), dtype=np.float32)
            out[name] = a.astype(np.float32)
        return out
    if getattr(shape, "gated", False):      # nomic-embed-text under NomicBertModel's names: no position table, no biases
        names = [("embeddings.word_embeddings.weight", (shape.vocab_size, h)), ("embeddings.token_type_embeddings.weight", (2, h)),
                 ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
        for i in range(shape.layers):
            p = f"layers.{i}."
            names += [(p + "self_attn.q_proj.weight", (h, h)), (p + "self_attn.k_proj.weight", (h, h)),
                      (p + "self_attn.v_proj.weight", (h, h)), (p + "self_attn.o_proj.weight", (h, h)),
                      (p + "post_attention_layernorm.weight", (h,)), (p + "post_attention_layernorm.bias", (h,)),
                      (p + "mlp.gate_proj.weight", (f, h)), (p + "mlp.up_proj.weight", (f, h)), (p + "mlp.down_proj.weight", (h, f)),
                      (p + "post_mlp_layernorm.weight", (h,)), (p + "post_mlp_layernorm.bias", (h,))]
        out = {}
        for idx, (name, shp) in enumerate(names):
            rng = np.random.Generator(np.random.PCG64([seed, idx]))
            if name.endswith("norm.weight"):
                a = 1.0 + 0.05 * rng.standard_normal(shp, dtype=np.float32)
            elif name.endswith(".bias"):
                a = 0.02 * rng.standard_normal(shp, dtype=np.float32)
            elif ".q_proj." in name or ".k_proj." in name:
                # ~N(0, 1 / h): attention logits q . k / sqrt(hd) of unit variance at EVERY width.  Rotary positions act only
                # through these logits; at `scale` a 64-wide model's logits have a standard deviation of 0.16 (the 768-wide
                # one's: 1.9), its softmax is flat and the rotation could not show in any output
                a = h ** -0.5 * rng.standard_normal(shp, dtype=np.float32)
            else:
                a = scale * rng.standard_normal(shp, dtype=np.float32)
            out[name] = a.astype(np.float32)
        return out
    names = [("embeddings.word_embeddings.weight", (shape.vocab_size, h)),
             ("embeddings.position_embeddings.weight", (shape.max_pos, h)),
             ("embeddings.token_type_embeddings.weight", (2, h)),
             ("embeddings.LayerNorm.weight", (h,)), ("embeddings.LayerNorm.bias", (h,))]
    for i in range(shape.layers):
        p = f"encoder.layer.{i}."
        names += [(p + "attention.self.query.weight", (h, h)), (p + "attention.self.query.bias", (h,)),
                  (p + "attention.self.key.weight", (h, h)), (p + "attention.self.key.bias", (h,)),
                  (p + "attention.self.value.weight", (h, h)), (p + "attention.self.value.bias", (h,)),
                  (p + "attention.output.dense.weight", (h, h)), (p + "attention.output.dense.bias", (h,)),
                  (p + "attention.output.LayerNorm.weight", (h,)), (p + "attention.output.LayerNorm.bias", (h,)),
                  (p + "intermediate.dense.weight", (f, h)), (p + "intermediate.dense.bias", (f,)),
                  (p + "output.dense.weight", (h, f)), (p + "output.dense.bias", (h,)),
                  (p + "output.LayerNorm.weight", (h,)), (p + "output.LayerNorm.bias", (h,))]
    if getattr(shape, "rel_buckets", 0) > 0:      # last: the other tensors keep their streams
        names.append((REL_BIAS, (shape.rel_buckets, shape.heads)))
    out = {}
    for idx, (name, shp) in enumerate(names):
        rng = np.random.Generator(np.random.PCG64([seed, idx]))
        if name.endswith("LayerNorm.weight"):
            a = 1.0 + 0.05 * rng.standard_normal(shp, dtype=np.float32)
        elif name.endswith(".bias"):
            a = 0.02 * rng.standard_normal(shp, dtype=np.float32)
        elif name == REL_BIAS:
            a = 0.5 * rng.standard_normal(shp, dtype=np.float32)
        else:
            a = scale * rng.standard_normal(shp, dtype=np.float32)
        out[name] = a.astype(np.float32)
    if getattr(shape, "rel_buckets", 0) > 0:
        out["embeddings.token_type_embeddings.weight"][:] = 0.0
    return out


# MPNetModel's tensor names -> the internal (BertModel) ones, inside "encoder.layer.<i>."
_MPNET_LAYER_NAMES = {"attention.attn.q.": "attention.self.query.", "attention.attn.k.": "attention.self.key.",
                      "attention.attn.v.": "attention.self.value.", "attention.attn.o.": "attention.output.dense.",
                      "attention.LayerNorm.": "attention.output.LayerNorm."}


def _mpnet_weights(raw: Dict[str, np.ndarray], hidden: int) -> Dict[str, np.ndarray]:
    """An MPNet state dict (with or without the leading "mpnet.") under the internal names, plus a zero token-type row."""
    out = {}
    for k, v in raw.items():
        k = k[6:] if k.startswith("mpnet.") else k
        if k.startswith("encoder.layer."):
            head, rest = k.split(".", 3)[:3], k.split(".", 3)[3]
            for old, new in _MPNET_LAYER_NAMES.items():
                if rest.startswith(old):
                    rest = new + rest[len(old):]
                    break
            k = ".".join(head) + "." + rest
        out[k] = np.asarray(v, dtype=np.float32)
    out["embeddings.token_type_embeddings.weight"] = np.zeros((1, hidden), dtype=np.float32)
    return out


def _nomic_shape_and_weights(cfg: dict, raw: Dict[str, np.ndarray], pooling: str, max_seq):
    """(ModelShape, weights under NomicBertModel's names) of a model_type "nomic_bert" directory in either dialect: the hub
    checkpoint (config keys n_embd / n_head / ..., tensors emb_ln, encoder.layers.N.attn.Wqkv, attn.out_proj, mlp.fc11 = up,
    mlp.fc12 = gate, mlp.fc2, norm1, norm2 -- the renames of transformers' conversion mapping "nomic_bert") or one saved by
    transformers 5.x (BERT-style config keys + rope_parameters, the names kept as they are)."""
    from rag._encoder import ModelShape
    hub = "n_embd" in cfg
    if hub:
        if float(cfg.get("rotary_emb_fraction", 1.0)) != 1.0:
            raise NotImplementedError("nomic_bert: rotary_emb_fraction != 1 (partial rotation) is not supported")
        if cfg.get("rotary_emb_interleaved", False):
            raise NotImplementedError("nomic_bert: rotary_emb_interleaved (pairwise rotation) is not supported")
        if cfg.get("prenorm", False):
            raise NotImplementedError("nomic_bert: prenorm layers are not supported (post-LayerNorm is)")
        if cfg.get("rotary_emb_scale_base") is not None:
            raise NotImplementedError("nomic_bert: rotary_emb_scale_base (xPos scaling of the rotation) is not supported")
        if cfg.get("rotary_scaling_factor") not in (None, 1, 1.0):
            raise NotImplementedError("nomic_bert: rope scaling (rotary_scaling_factor) is not supported")
        act = str(cfg.get("activation_function", "swiglu")).lower()
        if act != "swiglu":
            raise NotImplementedError(f"nomic_bert: activation_function '{act}' is not supported (swiglu is)")
        hidden, heads, layers = int(cfg["n_embd"]), int(cfg["n_head"]), int(cfg["n_layer"])
        ffn = int(cfg.get("n_inner") or 4 * hidden)
        max_pos, theta = int(cfg.get("n_positions", 2048)), float(cfg.get("rotary_emb_base", 10000.0))
        eps = float(cfg.get("layer_norm_epsilon", 1e-12))
    else:
        rp = dict(cfg.get("rope_parameters") or {})
        if rp.get("rope_type", "default") != "default" or rp.get("factor") not in (None, 1, 1.0):
            raise NotImplementedError(f"nomic_bert: rope_type '{rp.get('rope_type')}' / scaling factor {rp.get('factor')} is not supported")
        if float(rp.get("partial_rotary_factor", 1.0)) != 1.0:
            raise NotImplementedError("nomic_bert: partial_rotary_factor != 1 is not supported")
        act = str(cfg.get("hidden_act", "silu")).lower()
        if act not in ("silu", "swish", "swiglu"):
            raise NotImplementedError(f"nomic_bert: hidden_act '{act}' is not supported (the silu-gated feed-forward is)")
        hidden, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
        ffn, max_pos = int(cfg["intermediate_size"]), int(cfg.get("max_position_embeddings", 2048))
        theta, eps = float(rp.get("rope_theta", cfg.get("rope_theta", 1000.0))), float(cfg.get("layer_norm_eps", 1e-12))
        if cfg.get("head_dim") not in (None, hidden // heads):
            raise NotImplementedError("nomic_bert: head_dim must be hidden_size / num_attention_heads")
    weights = {}
    renames = (("encoder.layers.", "layers."), ("emb_ln.", "embeddings.LayerNorm."), (".attn.out_proj.", ".self_attn.o_proj."),
               (".mlp.fc11.", ".mlp.up_proj."), (".mlp.fc12.", ".mlp.gate_proj."), (".mlp.fc2.", ".mlp.down_proj."),
               (".norm1.", ".post_attention_layernorm."), (".norm2.", ".post_mlp_layernorm."))
    for k, v in raw.items():
        for pre in ("model.", "bert.", "nomic_bert."):
            if k.startswith(pre):
                k = k[len(pre):]
        for old, new in renames:
            k = k.replace(old, new)
        v = np.asarray(v, dtype=np.float32)
        if ".attn.Wqkv." in k:      # [3H, H] (or [3H]) -> q, k, v, in that order
            for part, name in zip(np.split(v, 3, axis=0), "qkv"):
                weights[k.replace(".attn.Wqkv.", f".self_attn.{name}_proj.")] = np.ascontiguousarray(part)
        else:
            weights[k] = v
    shape = ModelShape(int(cfg["vocab_size"]), hidden, layers, heads, ffn, max_pos, eps, pooling, min(int(max_seq or max_pos), max_pos),
                       rotary_theta=theta, gated=True)
    return shape, weights


def _modernbert_shape_and_weights(cfg: dict, raw: Dict[str, np.ndarray], pooling: str, max_seq):
    """(ModelShape, weights under ModernBertModel's names) of a model_type "modernbert" directory; tensor names with or without
    a leading "model.".  Every option this encoder does not run is refused by name."""
    from rag._encoder import ModelShape
    for arch in cfg.get("architectures") or []:
        if arch != "ModernBertModel":
            raise NotImplementedError(f"modernbert: architecture '{arch}' (a task head) is not supported: save the bare ModernBertModel "
                                      f"(a sentence-transformers directory holds one)")
    act = str(cfg.get("hidden_activation", "gelu")).lower()
    if act != "gelu":
        raise NotImplementedError(f"modernbert: hidden_activation '{act}' is not supported (gelu is)")
    hidden, heads, layers = int(cfg["hidden_size"]), int(cfg["num_attention_heads"]), int(cfg["num_hidden_layers"])
    ffn, max_pos = int(cfg["intermediate_size"]), int(cfg.get("max_position_embeddings", 8192))
    # which layers attend the whole sequence: layer_types (transformers 5.x) or global_attn_every_n_layers
    types = cfg.get("layer_types")
    if types is not None:
        if len(types) != layers or any(t not in ("full_attention", "sliding_attention") for t in types):
            raise NotImplementedError(f"modernbert: layer_types {types} must name full_attention / sliding_attention once per layer")
        full = [i for i, t in enumerate(types) if t == "full_attention"]
        every = full[1] if len(full) > 1 else layers
        if not full or full[0] != 0 or full != list(range(0, layers, every)):
            raise NotImplementedError(f"modernbert: layer_types {types} are not periodic (full attention in layers 0, n, 2 n, ...)")
    else:
        every = int(cfg.get("global_attn_every_n_layers", 3))
        if every < 1:
            raise NotImplementedError(f"modernbert: global_attn_every_n_layers {every} is not supported")
    rp = cfg.get("rope_parameters")
    if rp:
        thetas = {}
        for kind in ("full_attention", "sliding_attention"):
            one = dict(rp.get(kind) or {}) if ("full_attention" in rp or "sliding_attention" in rp) else dict(rp)
            if one.get("rope_type", "default") != "default" or one.get("factor") not in (None, 1, 1.0):
                raise NotImplementedError(f"modernbert: rope scaling ({kind}: rope_type '{one.get('rope_type')}', factor {one.get('factor')}) is not supported")
            if "rope_theta" not in one:
                raise NotImplementedError(f"modernbert: rope_parameters has no rope_theta for {kind}")
            thetas[kind] = float(one["rope_theta"])
        g_theta, l_theta = thetas["full_attention"], thetas["sliding_attention"]
    else:
        if cfg.get("rope_scaling") not in (None, {}):
            raise NotImplementedError(f"modernbert: rope scaling ({cfg.get('rope_scaling')}) is not supported")
        g_theta = float(cfg.get("global_rope_theta", 160000.0))
        l_theta = float(cfg.get("local_rope_theta") or g_theta)
    window = int(cfg.get("local_attention", 128)) // 2
    if window < 1:
        raise NotImplementedError(f"modernbert: local_attention {cfg.get('local_attention')} leaves no window")
    weights = {(k[6:] if k.startswith("model.") else k): np.asarray(v, dtype=np.float32) for k, v in raw.items()}
    for k in weights:
        if k.split(".", 1)[0] in ("head", "decoder", "classifier"):
            raise NotImplementedError(f"modernbert: tensor '{k}' belongs to a task head (ModernBertForMaskedLM / ForSequenceClassification): not supported")
    # a bias the config announces must be in the file (the kernels run without one where it is absent, which would be silent)
    need = [("norm_bias", ["embeddings.norm.bias", "final_norm.bias"] + [f"layers.{i}.mlp_norm.bias" for i in range(layers)]
             + [f"layers.{i}.attn_norm.bias" for i in range(1, layers)]),
            ("attention_bias", [f"layers.{i}.attn.{n}.bias" for i in range(layers) for n in ("Wqkv", "Wo")]),
            ("mlp_bias", [f"layers.{i}.mlp.{n}.bias" for i in range(layers) for n in ("Wi", "Wo")])]
    for key, names in need:
        if cfg.get(key, False):
            for n in names:
                if n not in weights:
                    raise NotImplementedError(f"modernbert: config says {key} = true but the checkpoint has no '{n}'")
    shape = ModelShape(int(cfg["vocab_size"]), hidden, layers, heads, ffn, max_pos, float(cfg.get("norm_eps", 1e-5)), pooling,
                       min(int(max_seq or max_pos), max_pos), rotary_theta=g_theta, local_theta=l_theta, prenorm=True, gelu_gated=True,
                       window=window, global_every=every)
    return shape, weights


def _load_local_dir(path: str):
    """(ModelShape, weights dict, tokenizer, pre_lower, normalize_module) from a sentence-transformers directory.

    What ``SentenceTransformer(path)`` (reference rag/embedding.py:33) assembles from the same files:
    modules.json lists the pipeline (Transformer at "", Pooling at "1_Pooling", optional Normalize); the
    Transformer module reads config.json + model.safetensors + the tokenizer files and takes
    ``max_seq_length`` / ``do_lower_case`` from sentence_bert_config.json -- the latter is only an extra
    ``str.lower()`` pass BEFORE the tokenizer, whose own casing rule comes from its own files."""
    from safetensors.numpy import load_file
    from rag._encoder import ModelShape
    from rag.tokenizer import tokenizer_from_model_dir
    tr_dir, pool_dir, has_normalize = path, os.path.join(path, "1_Pooling"), False
    mj = os.path.join(path, "modules.json")
    if os.path.exists(mj):
        with open(mj) as fh:
            for mod in json.load(fh):
                kind = str(mod.get("type", "")).rsplit(".", 1)[-1]
                sub = os.path.join(path, mod.get("path", "") or "")
                if kind == "Transformer":
                    tr_dir = sub
                elif kind == "Pooling":
                    pool_dir = sub
                elif kind == "Normalize":
                    has_normalize = True
                elif kind:
                    raise NotImplementedError(f"sentence-transformers module '{mod.get('type')}' is not supported by this encoder")
    with open(os.path.join(tr_dir, "config.json")) as fh:
        cfg = json.load(fh)
    max_seq, pooling, pre_lower = cfg.get("max_position_embeddings", 512), "mean", False
    sbc_max_seq = None       # sentence_bert_config.json's own limit, for configs without max_position_embeddings (nomic_bert)
    sb = os.path.join(tr_dir, "sentence_bert_config.json")
    if os.path.exists(sb):
        with open(sb) as fh:
            sbc = json.load(fh)
        max_seq = sbc.get("max_seq_length", max_seq) or max_seq
        sbc_max_seq = sbc.get("max_seq_length") or None
        pre_lower = bool(sbc.get("do_lower_case", False))
    pc = os.path.join(pool_dir, "config.json")
    if os.path.exists(pc):
        with open(pc) as fh:
            pcfg = json.load(fh)
        modes = [m for m in ("cls_token", "mean_tokens", "max_tokens", "mean_sqrt_len_tokens", "weightedmean_tokens", "lasttoken")
                 if pcfg.get("pooling_mode_" + m)]
        if modes == ["cls_token"]:
            pooling = "cls"
        elif modes not in ([], ["mean_tokens"]):
            raise NotImplementedError(f"pooling mode(s) {modes} are not supported (mean and CLS are)")
    model_type = cfg.get("model_type", "bert")
    if model_type == "nomic_bert":
        raw = load_file(os.path.join(tr_dir, "model.safetensors"))
        shape, weights = _nomic_shape_and_weights(cfg, raw, pooling, sbc_max_seq)
        return shape, weights, tokenizer_from_model_dir(tr_dir), pre_lower, has_normalize
    if model_type == "modernbert":
        raw = load_file(os.path.join(tr_dir, "model.safetensors"))
        shape, weights = _modernbert_shape_and_weights(cfg, raw, pooling, sbc_max_seq)
        return shape, weights, tokenizer_from_model_dir(tr_dir), pre_lower, has_normalize
    if model_type not in ("bert", "mpnet", "xlm-roberta"):
        raise NotImplementedError(f"model_type '{model_type}' is not supported by this encoder (bert, mpnet and xlm-roberta are, and nomic_bert, modernbert)")
    rel_buckets = pos_offset = 0
    if model_type == "mpnet":
        rel_buckets = int(cfg.get("relative_attention_num_buckets", 32))
    if model_type in ("mpnet", "xlm-roberta"):
        pos_offset = int(cfg.get("pad_token_id", 1)) + 1       # position ids count from padding_idx + 1
    shape = ModelShape(cfg["vocab_size"], cfg["hidden_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"],
                       cfg["intermediate_size"], cfg["max_position_embeddings"],
                       cfg.get("layer_norm_eps", 1e-12 if model_type == "bert" else 1e-5),
                       pooling, min(max_seq, cfg["max_position_embeddings"] - pos_offset),
                       rel_buckets=rel_buckets, pos_offset=pos_offset)
    raw = load_file(os.path.join(tr_dir, "model.safetensors"))
    if model_type == "mpnet":
        weights = _mpnet_weights(raw, shape.hidden)
    elif model_type == "xlm-roberta":     # XLMRobertaModel's names are BertModel's; the token-type table (one row) as shipped
        weights = {(k[8:] if k.startswith("roberta.") else k): np.asarray(v, dtype=np.float32) for k, v in raw.items()}
    else:
        weights = {(k[5:] if k.startswith("bert.") else k): np.asarray(v, dtype=np.float32) for k, v in raw.items()}
    return shape, weights, tokenizer_from_model_dir(tr_dir), pre_lower, has_normalize


class EmbeddingModel:
    """Sentence encoder wrapper (BERT, MPNet, XLM-RoBERTa, nomic-embed-text and ModernBERT checkpoints) running on the GPU."""

    def __init__(self, config: dict):
        self.tokenize_mode = config.get('tokenize', 'host')     # additive key: 'device' = csrc/wordpiece.hip feeds the encoder
        if self.tokenize_mode not in ('host', 'device'):
            raise ValueError(f"rag.embedding.tokenize must be 'host' or 'device', got {self.tokenize_mode!r}")
        self.model_name = config.get('model_name', 'sentence-transformers/all-MiniLM-L6-v2')
        self.batch_size = config.get('batch_size', 32)
        self.normalize = config.get('normalize', True)
        # additive keys: the task prefix of each kind of text ("" = none)
        self.query_prefix = str(config.get('query_prefix', '') or '')
        self.document_prefix = str(config.get('document_prefix', '') or '')
        self.device = self._get_device(config.get('device', 'cuda'))
        logger.info(f"Loading embedding model: {self.model_name}")
        self._pre_lower = False      # sentence_bert_config.json do_lower_case: an extra str.lower() before the tokenizer
        self.has_normalize_module = None   # a sentence-transformers directory: whether its modules.json lists Normalize (else None)
        shape, weights, self.tokenizer = self._resolve(config)
        self._device_tokenizer = None
        if self.tokenize_mode == 'device' and shape.prenorm:
            raise NotImplementedError("rag.embedding.tokenize 'device' is not supported for ModernBERT models: their byte-level BPE "
                                      "tokeniser has no device kernel (use 'host')")
        if self.tokenize_mode == 'device':
            from rag._unigram import tokenizer_spec
            tokenizer_spec(self.tokenizer)      # NotImplementedError for a tokenizer the kernel does not restate; tables on first use
        if config.get('max_seq_length'):
            from dataclasses import replace
            shape = replace(shape, max_seq=min(int(config['max_seq_length']), shape.max_pos - shape.pos_offset))
        if config.get('pooling'):
            from dataclasses import replace
            shape = replace(shape, pooling=config['pooling'])
        from rag._encoder import HipEncoder
        self.shape = shape
        self.model = HipEncoder(shape, weights, device=self.device)
        self.dimension = shape.hidden
        logger.info(f"Model loaded on {self.device}")
        logger.info(f"Embedding dimension: {self.dimension}")

    def _get_device(self, device_preference: str) -> str:
        """Always the ROCm device (torch-ROCm reports it as 'cuda'); there is no CPU path."""
        nat.require_gpu()
        if device_preference not in ("cuda", None) and not str(device_preference).startswith("cuda"):
            logger.warning(f"device '{device_preference}' requested; this build only runs on the GPU ('cuda')")
            return "cuda"
        return device_preference or "cuda"

    def _resolve(self, config: dict):
        from rag._encoder import ModelShape
        name = self.model_name
        for cand in (config.get('model_path'), name,
                     os.path.join(os.environ.get("CRS_MODEL_DIR", ""), os.path.basename(name)) if os.environ.get("CRS_MODEL_DIR") else None):
            if cand and os.path.isdir(cand) and os.path.exists(os.path.join(cand, "model.safetensors")):
                logger.info(f"Loading local checkpoint {cand}")
                shape, weights, tok, self._pre_lower, self.has_normalize_module = _load_local_dir(cand)
                return shape, weights, tok
        key = name.split(":", 1)[1] if name.startswith("synthetic:") else os.path.basename(name)
        key = _ALIASES.get(key.lower(), key.lower())
        if key in _KNOWN and (name.startswith("synthetic:") or os.environ.get("CRS_ALLOW_SYNTHETIC_WEIGHTS") == "1"):
            logger.warning(f"Using SYNTHETIC weights for architecture '{key}' (no checkpoint available offline)")
            shape = ModelShape(**{"ln_eps": 1e-12, **_KNOWN[key]})
            seed = int(config.get('synthetic_seed', 0))
            # MPNet and XLM-RoBERTa vocabularies open with <s> <pad> </s> <unk>
            tok = HashTokenizer(shape.vocab_size, special=(0, 2, 1)) if shape.pos_offset else HashTokenizer(shape.vocab_size)
            return shape, synthetic_weights(shape, seed), tok
        raise FileNotFoundError(
            f"No local checkpoint for '{name}': pass a sentence-transformers directory as model_name/model_path, "
            f"set CRS_MODEL_DIR, or use 'synthetic:minilm' (models cannot be downloaded here)")

    # ---- encoding ------------------------------------------------------------------------------
    def _with_prefix(self, texts, kind: Optional[str]):
        """texts with the prefix of `kind` (None | 'query' | 'document') in front; the list itself where there is none."""
        if kind not in (None, 'query', 'document'):
            raise ValueError(f"kind must be None, 'query' or 'document', got {kind!r}")
        prefix = self.query_prefix if kind == 'query' else self.document_prefix if kind == 'document' else ''
        return [prefix + str(t) for t in texts] if prefix else texts

    def tokenize(self, texts: List[str], kind: Optional[str] = None):
        """-> list of id lists ([CLS] ... [SEP] or the model's own <s> ... </s>, truncated to max_seq).  Text is stripped (and lower-cased when the
        model's sentence_bert_config.json says so) first, as sentence-transformers' Transformer.tokenize does.  kind: the task
        prefix put in front of every text first ('query' / 'document'; None: none)."""
        texts = [str(t).strip() for t in self._with_prefix(texts, kind)]
        if self._pre_lower:
            texts = [t.lower() for t in texts]
        if hasattr(self.tokenizer, "encode_batch"):
            return self.tokenizer.encode_batch(texts, self.shape.max_seq)
        return [self.tokenizer.encode(t, self.shape.max_seq) for t in texts]

    TOKENIZE_GROUP_BYTES = TOKENIZE_GROUP_BYTES

    def _tokenize_device(self, texts: List[str], timings: Optional[dict] = None):
        """tokenize_on_device with this model's tokenizer, device, max_seq and casing."""
        from rag._unigram import device_tokenizer
        dev = self.model.device
        if self._device_tokenizer is None:
            self._device_tokenizer = device_tokenizer(self.tokenizer, dev)      # csrc/wordpiece.hip or csrc/unigram.hip, by type
        return tokenize_on_device(self._device_tokenizer, self.tokenizer, dev, texts, self.shape.max_seq, self.tokenize,
                                  pre_lower=self._pre_lower, group_bytes=self.TOKENIZE_GROUP_BYTES, timings=timings)

    def tokenize_device(self, texts: List[str], kind: Optional[str] = None):
        """-> (ids cuda int32 [n, max_seq]: what self.tokenize gives, right-padded with the pad id; lens cuda int32 [n]), tokenised
        by the device kernel whatever rag.embedding.tokenize says (additive).  kind: as tokenize."""
        import torch
        from rag._unigram import tokenizer_spec
        tokenizer_spec(self.tokenizer)
        ids, lens = self._tokenize_device(list(self._with_prefix(texts, kind)))
        return ids, torch.from_numpy(lens).to(ids.device)

    def _embed_device_tokens(self, texts: List[str], out):
        """embed_device with rag.embedding.tokenize 'device': the same order (longest text first), batches and widths as the
        host branch, so every batch's (ids, lens) block is the tensor pad_batch would have built; the blocks are cut on the device."""
        import torch
        n, dev = len(texts), out.device
        ids_all, lens_h = self._tokenize_device(texts)
        steps = tuple(st for st in (16, 32, 64) if st <= self.shape.max_seq)

        def width_of(lens):
            width = int(lens.max())
            for step in steps:
                if width <= step:
                    return step
            return width

        if n <= self.batch_size:
            return self.model.forward(ids_all[:, : width_of(lens_h)].contiguous(), lens_h, normalize=bool(self.normalize), out=out)
        order = sorted(range(n), key=lambda i: -len(texts[i]))
        lens_all = torch.from_numpy(lens_h).to(dev)
        cur = torch.cuda.current_stream(dev)
        lanes = [torch.cuda.Stream(device=dev) for _ in range(2)]
        lane_ws = [None, None]
        ready = torch.cuda.Event()
        ready.record(cur)              # after the tokeniser's launches and row writes, which ran on `cur`
        for b, lo in enumerate(range(0, n, self.batch_size)):
            sel = order[lo: lo + self.batch_size]
            width = width_of(lens_h[sel])
            st = lanes[b & 1]
            with torch.cuda.stream(st):
                if b < 2:
                    st.wait_event(ready)
                sel_t = torch.as_tensor(sel, device=dev)
                ids = ids_all[sel_t, :width].contiguous()
                need = self.model.workspace_bytes(len(sel), width)
                if lane_ws[b & 1] is None or lane_ws[b & 1].numel() < need:
                    lane_ws[b & 1] = torch.empty(need, dtype=torch.uint8, device=dev)
                emb = self.model.forward(ids, lens_all[sel_t], normalize=bool(self.normalize), workspace=lane_ws[b & 1])
                out[sel_t] = emb
        for st in lanes:
            out.record_stream(st)
            ids_all.record_stream(st)
            lens_all.record_stream(st)
            cur.wait_stream(st)
        return out

    def embed_device(self, texts: Union[str, List[str]], kind: Optional[str] = None):
        """Embeddings as a cuda fp32 tensor [n, d] in input order (additive, zero-copy index build).  kind: the task prefix
        put in front of every text ('query' / 'document'; None: none)."""
        import torch
        if isinstance(texts, str):
            texts = [texts]
        texts = self._with_prefix(texts, kind)
        n = len(texts)
        out = torch.empty((n, self.dimension), dtype=torch.float32, device=self.model.device)
        if n == 0:
            return out
        if self.tokenize_mode == 'device':
            return self._embed_device_tokens(list(texts), out)
        token_ids = self.tokenize(texts)
        if n <= self.batch_size:   # one batch: no length sort, no scatter (its index tensor is a blocking H2D copy per call)
            ids, lens = pad_batch(token_ids, getattr(self.tokenizer, "pad_id", 0),
                                  short_steps=tuple(st for st in (16, 32, 64) if st <= self.shape.max_seq))
            return self.model.forward(ids, lens, normalize=bool(self.normalize), out=out)
        # longest first, like SentenceTransformer.encode: least padding per batch
        order = sorted(range(n), key=lambda i: -len(texts[i]))
        # Two batches in flight on two side streams: the forward's HBM-bound phases (LayerNorm epilogues: a quarter of a
        # MiniLM layer at index-build size) of one batch run under the matrix phases of the other (+ 3-5 % tokens/s,
        # bench.py --workload enc-* --enc-inflight 2); host-side padding of the next batch overlaps too.
        cur = torch.cuda.current_stream(out.device)
        lanes = [torch.cuda.Stream(device=out.device) for _ in range(2)]
        lane_ws = [None, None]
        ready = torch.cuda.Event()
        ready.record(cur)
        for b, lo in enumerate(range(0, n, self.batch_size)):
            sel = order[lo: lo + self.batch_size]
            ids, lens = pad_batch([token_ids[i] for i in sel], getattr(self.tokenizer, "pad_id", 0),
                                  short_steps=tuple(st for st in (16, 32, 64) if st <= self.shape.max_seq))
            st = lanes[b & 1]
            with torch.cuda.stream(st):
                if b < 2:
                    st.wait_event(ready)        # `out` (and anything the caller queued) before the first write
                need = self.model.workspace_bytes(int(ids.shape[0]), int(ids.shape[1]))
                if lane_ws[b & 1] is None or lane_ws[b & 1].numel() < need:     # the encoder's own scratch is shared:
                    lane_ws[b & 1] = torch.empty(need, dtype=torch.uint8, device=out.device)   # concurrent forwards need one each
                emb = self.model.forward(ids, lens, normalize=bool(self.normalize), workspace=lane_ws[b & 1])
                out[torch.as_tensor(sel, device=out.device)] = emb
        for st in lanes:
            out.record_stream(st)
            cur.wait_stream(st)
        return out

    def embed(self, texts: Union[str, List[str]], show_progress: bool = False, kind: Optional[str] = None) -> np.ndarray:
        """Embeddings for text(s): numpy float32 [n, d] (n = 1 for a single string).  kind: as embed_device."""
        return self.embed_device(texts, kind=kind).cpu().numpy()

    def embed_chunks(self, chunks: List[Chunk], show_progress: bool = True) -> np.ndarray:
        return self.embed([chunk.text for chunk in chunks], show_progress=show_progress, kind='document')

    def embed_chunks_device(self, chunks: List[Chunk], show_progress: bool = True):
        """embed_chunks without leaving the device (additive): cuda fp32 [n, d] for VectorStore.create_index."""
        return self.embed_device([chunk.text for chunk in chunks], kind='document')

    def get_dimension(self) -> int:
        return self.dimension
