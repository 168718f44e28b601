"""ctypes binding of the encoder half of libcrs_hip.so (include/crs_encoder.h) + weight upload.

``HipEncoder`` owns the device copies of a BERT-family checkpoint (HuggingFace BertModel state-dict
names, fp32 numpy in; matrices are cast to fp16 and Q/K/V stacked on upload) and runs the forward
through ``crs_encoder_forward_ex``.  A weights dict that also carries ``pooler.dense.*`` and ``classifier.*`` (one label: a
BertForSequenceClassification cross-encoder) gets its head uploaded too, and ``score_pairs`` runs ``crs_encoder_score_pairs``.  MPNet checkpoints come in under the same names plus
``encoder.relative_attention_bias.weight`` (rag/embedding.py maps them), with ``ModelShape.rel_buckets``
and ``pos_offset`` set: the bias is resolved per offset on the host and handed to the library.  Token ids in, pooled sentence embeddings out; no CPU fallback.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, Structure, byref, c_float, c_int, c_int32, c_size_t, c_void_p
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from rag import _native as nat

POOL_MEAN, POOL_CLS = 0, 1
ENC_SMALL_LDS = 1      # CRS_ENC_SMALL_LDS: kernel forms of <= 48 KB of LDS (forwards that run beside a scan)


class EncoderDesc(Structure):
    _fields_ = [("vocab_size", c_int32), ("hidden", c_int32), ("layers", c_int32), ("heads", c_int32),
                ("ffn", c_int32), ("max_pos", c_int32), ("ln_eps", c_float), ("pooling", c_int32), ("flags", c_int32)]


class EncoderLayer(Structure):
    _fields_ = [(n, c_void_p) for n in ("w_qkv", "b_qkv", "w_o", "b_o", "ln1_g", "ln1_b", "w_up", "b_up",
                                        "w_down", "b_down", "ln2_g", "ln2_b")]


class EncoderWeights(Structure):
    _fields_ = [("word_emb", c_void_p), ("pos_emb", c_void_p), ("type_emb", c_void_p), ("emb_ln_g", c_void_p),
                ("emb_ln_b", c_void_p), ("layers", POINTER(EncoderLayer))]


class EncoderExt(Structure):      # crs_encoder_ext
    _fields_ = [("rel_bias_dev", c_void_p), ("rel_span", c_int32)]


class EncoderHead(Structure):     # crs_encoder_head
    _fields_ = [("w_pool", c_void_p), ("b_pool", c_void_p), ("w_cls", c_void_p), ("b_cls", c_void_p),
                ("type_rows", c_int32), ("activation", c_int32)]


HEAD_NAMES = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")
ACTIVATIONS = {"identity": 0, "sigmoid": 1}


nat.register_signatures({
    "crs_encoder_workspace_bytes": (c_int, [POINTER(EncoderDesc), c_int, c_int, POINTER(c_size_t)]),
    "crs_encoder_forward": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int,
                                    c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p]),
    "crs_encoder_forward_queries": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int,
                                            c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_void_p]),
    "crs_encoder_forward_ex": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int,
                                       c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p, POINTER(EncoderExt)]),
    "crs_encoder_forward_queries_ex": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int,
                                               c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_void_p,
                                               POINTER(EncoderExt)]),
    "crs_encoder_score_pairs": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), POINTER(EncoderHead), c_void_p, c_void_p,
                                        c_void_p, c_int, c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_gemm_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                             c_void_p]),
    # test-facing: one GEMM family / one projection + LayerNorm step on its own (include/crs_encoder.h)
    "crs_gemm_f16_routed": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_void_p]),
    "crs_gemm_plan_describe": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, POINTER(c_int), c_void_p, c_size_t]),
    "crs_proj_ln_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_int, c_int, c_int,
                                c_void_p, c_void_p, c_void_p, c_void_p]),
    "crs_proj_ln_plan_describe": (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_int), c_void_p, c_size_t]),
})


@dataclass(frozen=True)
class ModelShape:
    vocab_size: int
    hidden: int
    layers: int
    heads: int
    ffn: int
    max_pos: int
    ln_eps: float = 1e-12
    pooling: str = "mean"
    max_seq: int = 256
    rel_buckets: int = 0          # > 0: MPNet's bucketed relative-position bias ("encoder.relative_attention_bias.weight")
    rel_max_distance: int = 128
    pos_offset: int = 0           # first position id (MPNet: pad_token_id + 1 = 2); max_pos counts the table's rows


def relative_position_bucket(rel, num_buckets: int = 32, max_distance: int = 128):
    """MPNet's bidirectional bucket of the offsets `rel` = key - query (int array) -> int64 numpy array.  With
    n = query - key: half the buckets per sign (keys after the query add num_buckets / 2); within a half |n| < max_exact
    = num_buckets / 4 maps to itself, larger |n| to max_exact + floor(log(|n| / max_exact) / log(max_distance /
    max_exact) * (half - max_exact)), capped at half - 1.  The logarithm is evaluated in fp32 with torch's kernels, as
    the published model does: at |n| = 32, 128 the exact value is a whole number and the fp32 rounding decides the bucket."""
    import math
    import torch
    n = -torch.as_tensor(np.asarray(rel, dtype=np.int64))
    half = num_buckets // 2
    ret = (n < 0).to(torch.long) * half
    n = n.abs()
    max_exact = half // 2
    large = max_exact + (torch.log(n.float() / max_exact) / math.log(max_distance / max_exact) * (half - max_exact)).to(torch.long)
    large = torch.minimum(large, torch.full_like(large, half - 1))
    return (ret + torch.where(n < max_exact, n, large)).numpy()


def relative_bias_table(weight, span: int, num_buckets: int, max_distance: int = 128) -> np.ndarray:
    """relative_attention_bias.weight [buckets, heads] -> fp32 [heads, 2 * span - 1]: entry (key - query) + span - 1
    is the bias of that offset (what crs_encoder_ext.rel_bias_dev takes)."""
    w = np.asarray(weight, dtype=np.float32)
    if w.ndim != 2 or w.shape[0] != num_buckets:
        raise ValueError(f"relative_attention_bias.weight must be [{num_buckets}, heads], got {w.shape}")
    bucket = relative_position_bucket(np.arange(-(span - 1), span), num_buckets, max_distance)
    return np.ascontiguousarray(w[bucket].T)


def gemm_f16(a, w, bias=None, residual=None, mode: int = 0):
    """a: cuda fp16 [M, K]; w: cuda fp16 [N, K]; returns fp16 [M, N] (modes 0/1) or fp32 (mode 2)."""
    import torch
    m, k = a.shape
    n = w.shape[0]
    out = torch.empty((m, n), dtype=torch.float32 if mode == 2 else torch.float16, device=a.device)
    nat.check(nat.load().crs_gemm_f16(nat._ptr(a), nat._ptr(w), nat._ptr(bias), nat._ptr(residual), nat._ptr(out),
                                      m, n, k, mode, nat._stream_ptr()))
    return out


def _describe(call):
    """(text, slabs) of a describe entry: call(slabs_ref, buf, cap) -> length or error code"""
    cap, slabs = 512, c_int(0)
    while True:
        buf = ctypes.create_string_buffer(cap)
        need = call(byref(slabs), buf, cap)
        nat.check(min(need, 0))
        if need < cap:
            return buf.value.decode(), int(slabs.value)
        cap = need + 1


def gemm_plan_describe(m: int, n: int, k: int, mode: int, route: int = 0, flags: int = 0):
    """(launch line, slabs) of gemm_f16_routed for these sizes on the current device (crs_gemm_plan_describe)."""
    lib = nat.load()
    return _describe(lambda sl, buf, cap: lib.crs_gemm_plan_describe(m, n, k, mode, route, flags, sl, buf, cap))


def gemm_f16_routed(a, w, bias, residual, out, mode: int, route: int = 0, flags: int = 0) -> None:
    """crs_gemm_f16_routed into `out`: cuda fp16 [M, N] (modes 0 / 1), fp32 [M, N] (mode 2) or fp32 [slabs, M, N] (mode 3, no bias);
    route 0 plan_gemm, 1 the panel kernel, 2 the 256 x 256 kernel's split-K form."""
    m, k = a.shape
    nat.check(nat.load().crs_gemm_f16_routed(nat._ptr(a), nat._ptr(w), nat._ptr(bias), nat._ptr(residual), nat._ptr(out),
                                             m, w.shape[0], k, mode, route, flags, nat._stream_ptr()))


def proj_ln_plan_describe(tokens: int, hidden: int, k: int, flags: int = 0, big_ln: bool = False):
    """(launch lines, slabs) of proj_ln_f16 for these sizes on the current device (crs_proj_ln_plan_describe)."""
    lib = nat.load()
    return _describe(lambda sl, buf, cap: lib.crs_proj_ln_plan_describe(tokens, hidden, k, flags, int(big_ln), sl, buf, cap))


def proj_ln_f16(a, w, bias, g, b, eps: float, y32_ws, x32, x16, flags: int = 0, big_ln: bool = False) -> None:
    """crs_proj_ln_f16: x32 (cuda fp32 [T, H], the residual) <- LayerNorm(a w^T + bias + x32) in place, x16 its fp16 copy;
    y32_ws: cuda fp32 scratch of slabs * T * H elements."""
    t, k = a.shape
    nat.check(nat.load().crs_proj_ln_f16(nat._ptr(a), nat._ptr(w), nat._ptr(bias), nat._ptr(g), nat._ptr(b), float(eps), t, w.shape[0],
                                         k, flags, int(big_ln), nat._ptr(y32_ws), nat._ptr(x32), nat._ptr(x16), nat._stream_ptr()))


class HipEncoder:
    def __init__(self, shape: ModelShape, weights: Dict[str, np.ndarray], device=None):
        import torch
        nat.require_gpu()
        nat.load()
        self.shape = shape
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self._keep = []  # device tensors the C structs point into

        def dev32(name):
            t = torch.from_numpy(np.ascontiguousarray(weights[name], dtype=np.float32)).to(self.device)
            self._keep.append(t)
            return t

        def dev16(*names):
            arrs = [np.ascontiguousarray(weights[n], dtype=np.float32) for n in names]
            t = torch.from_numpy(np.concatenate(arrs, axis=0)).to(self.device).to(torch.float16).contiguous()
            self._keep.append(t)
            return t

        def cat32(*names):
            t = torch.from_numpy(np.concatenate([np.asarray(weights[n], dtype=np.float32) for n in names])).to(self.device)
            self._keep.append(t)
            return t

        # position ids start at pos_offset: the kernels index the table from its row pos_offset on
        if not 0 <= shape.pos_offset < shape.max_pos:
            raise ValueError("pos_offset must be inside the position table")
        self.desc = EncoderDesc(shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.ffn,
                                shape.max_pos - shape.pos_offset, shape.ln_eps, POOL_CLS if shape.pooling == "cls" else POOL_MEAN, 0)
        self._layers = (EncoderLayer * shape.layers)()
        for i in range(shape.layers):
            p = f"encoder.layer.{i}."
            vals = [
                dev16(p + "attention.self.query.weight", p + "attention.self.key.weight", p + "attention.self.value.weight"),
                cat32(p + "attention.self.query.bias", p + "attention.self.key.bias", p + "attention.self.value.bias"),
                dev16(p + "attention.output.dense.weight"), dev32(p + "attention.output.dense.bias"),
                dev32(p + "attention.output.LayerNorm.weight"), dev32(p + "attention.output.LayerNorm.bias"),
                dev16(p + "intermediate.dense.weight"), dev32(p + "intermediate.dense.bias"),
                dev16(p + "output.dense.weight"), dev32(p + "output.dense.bias"),
                dev32(p + "output.LayerNorm.weight"), dev32(p + "output.LayerNorm.bias"),
            ]
            for (fname, _), t in zip(EncoderLayer._fields_, vals):
                setattr(self._layers[i], fname, t.data_ptr())
        self.weights = EncoderWeights(
            dev32("embeddings.word_embeddings.weight").data_ptr(),
            dev32("embeddings.position_embeddings.weight")[shape.pos_offset:].data_ptr(),
            dev32("embeddings.token_type_embeddings.weight").data_ptr(),
            dev32("embeddings.LayerNorm.weight").data_ptr(),
            dev32("embeddings.LayerNorm.bias").data_ptr(),
            ctypes.cast(self._layers, POINTER(EncoderLayer)))
        self._ws = None
        # the same tensors in the order torch.ops.crs.encoder_forward takes them (csrc/torch_ops.cpp)
        self._wlist = self._keep[-5:] + self._keep[:-5]     # embeddings first, then 12 tensors per layer
        assert len(self._wlist) == 5 + 12 * shape.layers
        if shape.pos_offset:
            self._wlist[1] = self._wlist[1][shape.pos_offset:]       # (a contiguous view of the kept tensor)
        # additive relative-position bias, resolved per offset once: fp32 [heads, 2 * max_seq - 1] (crs_encoder_ext)
        self.rel_bias = None
        if shape.rel_buckets > 0:
            span = min(shape.max_seq, shape.max_pos - shape.pos_offset)
            table = relative_bias_table(weights["encoder.relative_attention_bias.weight"], span, shape.rel_buckets,
                                        shape.rel_max_distance)
            if table.shape[0] != shape.heads:
                raise ValueError("relative_attention_bias.weight must have one column per head")
            self.rel_bias = torch.from_numpy(table).to(self.device)
        # pair-classifier head (cross-encoders): [w_pool [H, H], b_pool [H], w_cls [H], b_cls [1]], fp32 as stored
        self.head = None
        if all(n in weights for n in HEAD_NAMES):
            if shape.rel_buckets > 0:
                raise ValueError("a pair head needs token types: MPNet shapes have none")
            h = shape.hidden
            want = {HEAD_NAMES[0]: (h, h), HEAD_NAMES[1]: (h,), HEAD_NAMES[2]: (1, h), HEAD_NAMES[3]: (1,)}
            for name, shp in want.items():
                if tuple(np.shape(weights[name])) != shp:
                    raise ValueError(f"{name} must be {shp} (one label), got {tuple(np.shape(weights[name]))}")
            self.head = [torch.from_numpy(np.ascontiguousarray(weights[n], dtype=np.float32).reshape(-1 if i else (h, h))).to(self.device)
                         for i, n in enumerate(HEAD_NAMES)]
            self.type_rows = int(np.shape(weights["embeddings.token_type_embeddings.weight"])[0])

    @property
    def _desc_list(self):
        """crs_encoder_desc as the int list torch.ops.crs.encoder_forward takes (read from `desc`, so tests that
        switch `desc.pooling` are honoured)."""
        d = self.desc
        return [d.vocab_size, d.hidden, d.layers, d.heads, d.ffn, d.max_pos, d.pooling, d.flags]

    def workspace_bytes(self, batch: int, seq: int) -> int:
        out = c_size_t(0)
        nat.check(nat.load().crs_encoder_workspace_bytes(byref(self.desc), batch, seq, byref(out)))
        return int(out.value)

    def forward(self, ids, lens, normalize: bool = True, return_hidden: bool = False, out=None, workspace=None,
                q16_out=None, slab_type: int = nat.SLAB_F16, small_lds: bool = False):
        """ids: int32 [B, S] (numpy or cuda tensor, right padded), lens: int32 [B].
        Returns cuda fp32 [B, H] (and [B, S, H] hidden states when return_hidden).  With `q16_out`
        (cuda fp16 [B, padded_dim]) the pooled, normalised embeddings are also written there in the scan's
        query layout (crs_encoder_forward_queries)."""
        import torch
        if not isinstance(ids, torch.Tensor):
            ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32))
        if not isinstance(lens, torch.Tensor):
            lens = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32))
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        lens = lens.to(device=self.device, dtype=torch.int32).contiguous()
        b, s = ids.shape
        need = self.workspace_bytes(b, s)
        ws = workspace
        if ws is None:   # private scratch; pass `workspace` to run several forwards concurrently on different streams
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ws = self._ws
        elif ws.numel() < need:
            raise ValueError(f"encoder workspace too small: {ws.numel()} < {need}")
        if out is None:
            out = torch.empty((b, self.shape.hidden), dtype=torch.float32, device=self.device)
        if q16_out is not None:
            if return_hidden or not normalize:
                raise ValueError("q16_out needs normalize=True and return_hidden=False")
            if tuple(q16_out.shape) != (b, nat.padded_dim(self.shape.hidden, slab_type)) or q16_out.dtype != torch.float16:
                raise ValueError("q16_out must be fp16 [batch, padded_dim]")
        hidden = torch.empty((b, s, self.shape.hidden), dtype=torch.float32, device=self.device) if return_hidden else None
        desc = self._desc_list
        if small_lds:          # per call, not process-wide: the role-lane engine asks for it, everyone else gets the default forms
            desc = desc[:7] + [desc[7] | ENC_SMALL_LDS]
        with nat._translate():
            nat.ops().encoder_forward_ex(ids, lens, self._wlist, desc, float(self.desc.ln_eps), ws, out, q16_out,
                                         int(slab_type), bool(normalize), hidden, self.rel_bias)
        return (out, hidden) if return_hidden else out

    def score_pairs(self, ids, type_ids, lens, activation="identity", return_pooled: bool = False, return_hidden: bool = False,
                    workspace=None, small_lds: bool = False):
        """Relevance scores of sentence pairs.  ids: int32 [B, S] rows "[CLS] a [SEP] b [SEP]" (numpy or cuda tensor, right
        padded); type_ids: int32 [B, S] segment ids (0 / 1; padding 0) or None for all 0; lens: int32 [B].  activation:
        'identity' (the logit) or 'sigmoid'.  Returns cuda fp32 [B]; with return_pooled / return_hidden a tuple that also
        holds the pooler output [B, H] and / or the final hidden states [B, S, H], in that order."""
        import torch
        if self.head is None:
            raise ValueError("this encoder has no pair head: its weights carry no pooler.dense.* / classifier.* (one label)")
        if activation not in ACTIVATIONS and activation not in (0, 1):
            raise ValueError(f"activation must be 'identity' or 'sigmoid', got {activation!r}")

        def dev_i32(a):
            if not isinstance(a, torch.Tensor):
                a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32))
            return a.to(device=self.device, dtype=torch.int32).contiguous()

        ids, lens = dev_i32(ids), dev_i32(lens)
        if type_ids is not None:
            type_ids = dev_i32(type_ids)
            if type_ids.shape != ids.shape:
                raise ValueError("type_ids must have the shape of ids")
        b, s = ids.shape
        need = self.workspace_bytes(b, s)
        ws = workspace
        if ws is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            ws = self._ws
        elif ws.numel() < need:
            raise ValueError(f"encoder workspace too small: {ws.numel()} < {need}")
        scores = torch.empty((b,), dtype=torch.float32, device=self.device)
        pooled = torch.empty((b, self.shape.hidden), dtype=torch.float32, device=self.device) if return_pooled else None
        hidden = torch.empty((b, s, self.shape.hidden), dtype=torch.float32, device=self.device) if return_hidden else None
        desc = self._desc_list
        if small_lds:
            desc = desc[:7] + [desc[7] | ENC_SMALL_LDS]
        with nat._translate():
            nat.ops().encoder_score_pairs(ids, type_ids, lens, self._wlist, self.head, desc, float(self.desc.ln_eps),
                                          int(ACTIVATIONS.get(activation, activation)), ws, scores, pooled, hidden)
        extra = tuple(t for t in (pooled, hidden) if t is not None)
        return (scores,) + extra if extra else scores
