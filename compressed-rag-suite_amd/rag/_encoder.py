"""ctypes binding of the encoder half of libcrs_hip.so (include/crs_encoder.h) + weight upload.

``HipEncoder`` owns the device copies of a BERT-family checkpoint (HuggingFace BertModel state-dict
names, fp32 numpy in; matrices are cast to fp16 and Q/K/V stacked on upload) and runs the forward
through ``crs_encoder_forward_ex``.  A weights dict that also carries ``pooler.dense.*`` and ``classifier.*`` (one label: a
BertForSequenceClassification cross-encoder) gets its head uploaded too, and ``score_pairs`` runs ``crs_encoder_score_pairs``.  MPNet checkpoints come in under the same names plus
``encoder.relative_attention_bias.weight`` (rag/embedding.py maps them), with ``ModelShape.rel_buckets``
and ``pos_offset`` set: the bias is resolved per offset on the host and handed to the library.  Rotary, gated encoders
(nomic-embed-text: ``ModelShape.rotary_theta`` > 0 and ``gated``) come in under transformers' NomicBertModel names
(``layers.N.self_attn.q_proj`` ..., ``mlp.gate_proj`` / ``up_proj`` / ``down_proj``): the gate and up matrices are interleaved
into one ``w_up`` (``interleave_gate_up``), the cos / sin table is built on the host (``rope_table``) and the forward goes
through ``torch.ops.crs.encoder_forward_rope``.  ModernBERT checkpoints (``ModelShape.prenorm``: pre-norm layers, sliding-window
attention in the layers that are not a multiple of ``global_every``, two rope thetas, GeGLU) come in under ModernBertModel's
names (``layers.N.attn.Wqkv`` / ``attn.Wo`` / ``attn_norm`` / ``mlp_norm`` / ``mlp.Wi`` / ``mlp.Wo``, ``final_norm``) and go through
``torch.ops.crs.encoder_forward_prenorm``.  Token ids in, pooled sentence embeddings out; no CPU fallback.
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
ENC_ROTARY = 2         # CRS_ENC_ROTARY: rope_qk_kernel between the QKV projection and attention, no position table
ENC_GATED_SILU = 4     # CRS_ENC_GATED_SILU: w_up holds interleaved gate / up rows, FFN-up runs GEMM mode 4
ENC_PRENORM = 8        # CRS_ENC_PRENORM: pre-norm layers + sliding-window attention (crs_encoder_forward_prenorm)
ENC_GATED_GELU = 16    # CRS_ENC_GATED_GELU: the gated layout with the erf GELU on the activated half (GEMM mode 5)
GATE_UP_BLOCK = 16     # rows of a gate (or up) block of the interleaved layout (include/crs_encoder.h)


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


class EncoderRope(Structure):     # crs_encoder_rope
    _fields_ = [("table_dev", c_void_p), ("positions", c_int32)]


class EncoderPrenorm(Structure):  # crs_encoder_prenorm
    _fields_ = [("rope_global_dev", c_void_p), ("rope_local_dev", c_void_p), ("positions", c_int32), ("window", c_int32),
                ("global_every", c_int32), ("final_ln_g", c_void_p), ("final_ln_b", c_void_p)]


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
    # rotary models (the forward reaches them through torch.ops.crs.encoder_forward_rope)
    "crs_encoder_forward_rope": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int,
                                         c_int, c_void_p, c_size_t, c_void_p, c_int, c_void_p, c_void_p, POINTER(EncoderExt),
                                         POINTER(EncoderRope)]),
    "crs_encoder_forward_queries_rope": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int,
                                                 c_int, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_void_p,
                                                 POINTER(EncoderExt), POINTER(EncoderRope)]),
    "crs_rope_qk_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    # test-facing: the attention step / the fused QKV + attention kernel on its own
    "crs_attention_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "crs_qkv_attn_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "crs_attention_plan_describe": (c_int, [c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    # test-facing: the row kernels (embedding + LayerNorm, LayerNorm, pooling, pair head) on their own
    "crs_embed_ln_f32": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int,
                                 c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "crs_layernorm_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "crs_pool_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p]),
    "crs_pair_head_f32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p]),
    "crs_row_plan_describe": (c_int, [c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    # pre-norm models (the forward reaches them through torch.ops.crs.encoder_forward_prenorm) and their kernels on their own
    "crs_encoder_forward_prenorm": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int, c_int, c_void_p,
                                            c_size_t, c_void_p, c_int, c_void_p, c_void_p, POINTER(EncoderPrenorm)]),
    "crs_encoder_forward_queries_prenorm": (c_int, [POINTER(EncoderDesc), POINTER(EncoderWeights), c_void_p, c_void_p, c_int, c_int,
                                                    c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_void_p, POINTER(EncoderPrenorm)]),
    "crs_encoder_prenorm_plan_describe": (c_int, [POINTER(EncoderDesc), c_int, c_int, c_int, c_void_p, c_size_t]),
    "crs_attention_window_f16": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "crs_attention_window_plan_describe": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_size_t]),
    "crs_add_layernorm_f32": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
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
    rotary_theta: float = 0.0     # > 0: rotary position embedding of Q and K with this base, no position table (nomic: 1000)
    gated: bool = False           # SwiGLU feed-forward: silu(x Wgate^T) * (x Wup^T) in place of GELU(x W^T + b)
    # ModernBERT: pre-norm layers; rotary_theta is the full-attention layers' base and local_theta the sliding layers'
    prenorm: bool = False         # x += attn(LN(x)), x += mlp(LN(x)), a final norm after the last layer
    window: int = 0               # largest |key - query| of a sliding layer (local_attention // 2)
    global_every: int = 1         # layer i attends the whole sequence when i % global_every == 0
    local_theta: float = 0.0
    gelu_gated: bool = False      # GeGLU: Wo(gelu(input) * gate), (input, gate) = Wi(x).chunk(2)


def interleave_wi(wi) -> np.ndarray:
    """ModernBERT's Wi [2F, ...] (its output is chunked into (input, gate): rows [0, F) feed the GELU, rows [F, 2F) multiply) in the
    layout CRS_ENC_GATED_GELU takes: the activated half in the "gate" rows of interleave_gate_up, the linear half in the "up" rows."""
    w = np.asarray(wi)
    if w.shape[0] % 2:
        raise ValueError(f"Wi must have an even number of rows, got {w.shape}")
    return interleave_gate_up(w[: w.shape[0] // 2], w[w.shape[0] // 2:])


def interleave_gate_up(gate, up) -> np.ndarray:
    """gate, up: [F, ...] (F a multiple of 16) -> [2F, ...] in the layout CRS_ENC_GATED_SILU takes: rows [32 b, 32 b + 16) are
    rows [16 b, 16 b + 16) of gate (the half SiLU acts on), rows [32 b + 16, 32 b + 32) the same rows of up."""
    g, u = np.asarray(gate), np.asarray(up)
    if g.shape != u.shape or g.shape[0] % GATE_UP_BLOCK:
        raise ValueError(f"gate and up must have one shape with a multiple of {GATE_UP_BLOCK} rows, got {g.shape} and {u.shape}")
    blocks = (g.shape[0] // GATE_UP_BLOCK, GATE_UP_BLOCK) + g.shape[1:]
    return np.ascontiguousarray(np.stack([g.reshape(blocks), u.reshape(blocks)], axis=1).reshape((2 * g.shape[0],) + g.shape[1:]))


def split_gate_up(w):
    """The inverse of interleave_gate_up: [2F, ...] -> (gate, up)."""
    w = np.asarray(w)
    if w.shape[0] % (2 * GATE_UP_BLOCK):
        raise ValueError(f"an interleaved gate / up array has a multiple of {2 * GATE_UP_BLOCK} rows, got {w.shape}")
    b = w.reshape((w.shape[0] // (2 * GATE_UP_BLOCK), 2, GATE_UP_BLOCK) + w.shape[1:])
    half = (w.shape[0] // 2,) + w.shape[1:]
    return np.ascontiguousarray(b[:, 0].reshape(half)), np.ascontiguousarray(b[:, 1].reshape(half))


def rope_table(positions: int, head_dim: int, theta: float) -> np.ndarray:
    """fp32 [positions, head_dim], what crs_encoder_rope.table_dev takes: row p holds cos(p * theta^(-2 j / head_dim)) for
    j < head_dim / 2 in its first half and the sines of the same angles in its second half; fp64 on the host, rounded once."""
    if positions < 1 or head_dim % 2 or theta <= 0:
        raise ValueError("rope_table: positions >= 1, an even head_dim and theta > 0")
    inv = np.float64(theta) ** (-2.0 * np.arange(head_dim // 2, dtype=np.float64) / head_dim)
    ang = np.arange(positions, dtype=np.float64)[:, None] * inv[None, :]
    return np.ascontiguousarray(np.concatenate([np.cos(ang), np.sin(ang)], axis=1).astype(np.float32))


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


ATTN_ROUTE_FUSED = 16  # attention_plan_describe only: the launch of qkv_attn_f16


def attention_plan_describe(batch: int, seq: int, hidden: int, heads: int, rel_bias: bool = False, route: int = -1) -> str:
    """The launch line of attention_f16 (route 16: of qkv_attn_f16) for these sizes (crs_attention_plan_describe); needs no device."""
    lib = nat.load()
    return _describe(lambda sl, buf, cap: lib.crs_attention_plan_describe(batch, seq, hidden, heads, int(bool(rel_bias)), route, buf, cap))[0]


def attention_f16(qkv, lens, ctx, batch: int, seq: int, heads: int, rel_bias=None, route: int = -1) -> None:
    """crs_attention_f16: ctx (cuda fp16 [batch * seq, H]) <- attention of qkv (cuda fp16 [batch * seq, 3 H]) under lens (cuda int32
    [batch]); rel_bias: cuda fp32 [heads, 2 span - 1] or None; route < 0 the process's knobs, else bits 1 attn_seq off, 2 attn_short
    off, 4 attn_x32 off, 8 attn_qt4 on over the defaults."""
    span = (int(rel_bias.shape[1]) + 1) // 2 if rel_bias is not None else 0
    nat.check(nat.load().crs_attention_f16(nat._ptr(qkv), nat._ptr(lens), nat._ptr(ctx), int(batch), int(seq), int(qkv.shape[1]) // 3,
                                           int(heads), nat._ptr(rel_bias), span, int(route), nat._stream_ptr()))


def qkv_attn_f16(x16, w_qkv, b_qkv, lens, ctx, batch: int, seq: int, heads: int) -> None:
    """crs_qkv_attn_f16: ctx (cuda fp16 [batch * seq, H]) <- attention of the projection x16 w_qkv^T + b_qkv in one kernel; x16 cuda
    fp16 [batch * seq, H], w_qkv cuda fp16 [3 H, H], b_qkv cuda fp32 [3 H]."""
    nat.check(nat.load().crs_qkv_attn_f16(nat._ptr(x16), nat._ptr(w_qkv), nat._ptr(b_qkv), nat._ptr(lens), nat._ptr(ctx), int(batch),
                                          int(seq), int(x16.shape[1]), int(heads), nat._stream_ptr()))


def rope_qk_f16(qkv, table, batch: int, seq: int, heads: int) -> None:
    """crs_rope_qk_f16: rotates the Q and K column blocks of qkv (cuda fp16 [batch * seq, 3 H]) in place against table (cuda fp32
    [positions, H / heads], rope_table's layout)."""
    nat.check(nat.load().crs_rope_qk_f16(nat._ptr(qkv), nat._ptr(table), int(table.shape[0]), int(batch), int(seq), int(qkv.shape[1]) // 3,
                                         int(heads), nat._stream_ptr()))


ROW_EMBED, ROW_LAYERNORM, ROW_POOL, ROW_PAIR_HEAD = 0, 1, 2, 3   # crs_row_plan_describe's kinds
ROW_ADD_LAYERNORM = 4


def attention_window_plan_describe(batch: int, seq: int, hidden: int, heads: int, window: int) -> str:
    """The launch line of attention_window_f16 for these sizes (crs_attention_window_plan_describe); needs no device."""
    lib = nat.load()
    return _describe(lambda sl, buf, cap: lib.crs_attention_window_plan_describe(batch, seq, hidden, heads, int(window), buf, cap))[0]


def attention_window_f16(qkv, lens, ctx, batch: int, seq: int, heads: int, window: int) -> None:
    """crs_attention_window_f16: ctx (cuda fp16 [batch * seq, H]) <- attention of qkv (cuda fp16 [batch * seq, 3 H]) over the keys with
    |key - query| <= window and key < lens[b]; a query without any allowed key gets a zero row."""
    nat.check(nat.load().crs_attention_window_f16(nat._ptr(qkv), nat._ptr(lens), nat._ptr(ctx), int(batch), int(seq),
                                                  int(qkv.shape[1]) // 3, int(heads), int(window), nat._stream_ptr()))


def add_layernorm_f32(y, bias, residual, g, b, eps: float, r32, x16, n32=None) -> None:
    """crs_add_layernorm_f32: r32 (cuda fp32 [tokens, H]) <- sum of the slabs of y (cuda fp32 [nsplit, tokens, H]) + bias + residual;
    x16 (fp16) and n32 (fp32 or None) <- LayerNorm(r32) g + b.  bias / residual / b may be None, residual may be r32."""
    nsplit, tokens, hidden = y.shape
    nat.check(nat.load().crs_add_layernorm_f32(nat._ptr(y), int(nsplit), nat._ptr(bias), nat._ptr(residual), nat._ptr(g), nat._ptr(b),
                                               float(eps), int(tokens), int(hidden), nat._ptr(r32), nat._ptr(x16), nat._ptr(n32),
                                               nat._stream_ptr()))


def row_plan_describe(kind: int, rows: int, hidden: int, arg: int = 0) -> str:
    """The launch line of embed_ln_f32 (kind 0, rows = tokens, arg: typed), layernorm_f32 (1, tokens, arg = nsplit), pool_f32 (2, rows =
    batch) or pair_head_f32 (3, batch) for these sizes (crs_row_plan_describe); needs no device."""
    lib = nat.load()
    return _describe(lambda sl, buf, cap: lib.crs_row_plan_describe(int(kind), int(rows), int(hidden), int(arg), buf, cap))[0]


def embed_ln_f32(ids, type_ids, word, pos, type_tab, g, b, eps: float, seq: int, x32, x16) -> None:
    """crs_embed_ln_f32: x32 (cuda fp32 [tokens, H]) and x16 (fp16) <- LayerNorm((word[ids] + type_tab[type_ids]) + pos[t % seq]); ids cuda
    int32 [tokens]; type_ids cuda int32 [tokens] or None (row 0); pos cuda fp32 [>= seq, H] or None."""
    nat.check(nat.load().crs_embed_ln_f32(nat._ptr(ids), nat._ptr(type_ids), int(type_tab.shape[0]), nat._ptr(word), nat._ptr(pos),
                                          nat._ptr(type_tab), nat._ptr(g), nat._ptr(b), float(eps), int(ids.numel()), int(seq),
                                          int(word.shape[1]), int(word.shape[0]), nat._ptr(x32), nat._ptr(x16), nat._stream_ptr()))


def layernorm_f32(y, bias, residual, g, b, eps: float, x32, x16) -> None:
    """crs_layernorm_f32: x32 (cuda fp32 [tokens, H]) and x16 (fp16) <- LayerNorm(sum of the slabs of y (cuda fp32 [nsplit, tokens, H]) +
    bias + residual); bias / residual may be None, residual may be x32."""
    nsplit, tokens, hidden = y.shape
    nat.check(nat.load().crs_layernorm_f32(nat._ptr(y), int(nsplit), nat._ptr(bias), nat._ptr(residual), nat._ptr(g), nat._ptr(b),
                                           float(eps), int(tokens), int(hidden), nat._ptr(x32), nat._ptr(x16), nat._stream_ptr()))


def pool_f32(x32, lens, pooling: int, normalize: bool, out, out16=None, slab_type: int = nat.SLAB_F16) -> None:
    """crs_pool_f32: out (cuda fp32 [batch, H]) <- mean (pooling 0) or [CLS] (1) pooling of x32 (cuda fp32 [batch, seq, H]) under lens
    (cuda int32 [batch]), L2-normalised if asked; out16 (cuda fp16 [batch, padded_dim(H, slab_type)] or None): the query block."""
    batch, seq, hidden = x32.shape
    nat.check(nat.load().crs_pool_f32(nat._ptr(x32), nat._ptr(lens), int(batch), int(seq), int(hidden), int(pooling), int(bool(normalize)),
                                      nat._ptr(out), nat._ptr(out16), int(slab_type), nat._stream_ptr()))


def pair_head_f32(hidden32, w_pool, b_pool, w_cls, b_cls, activation: int, scores, pooled_out=None) -> None:
    """crs_pair_head_f32: scores (cuda fp32 [batch]) <- w_cls . tanh(w_pool h + b_pool) + b_cls of token 0 of every pair of hidden32 (cuda
    fp32 [batch, seq, H]), activation 1: then the sigmoid; pooled_out (cuda fp32 [batch, H] or None): the tanh layer."""
    batch, seq, hidden = hidden32.shape
    nat.check(nat.load().crs_pair_head_f32(nat._ptr(hidden32), int(batch), int(seq), int(hidden), nat._ptr(w_pool), nat._ptr(b_pool),
                                           nat._ptr(w_cls), nat._ptr(b_cls), int(activation), nat._ptr(scores), nat._ptr(pooled_out),
                                           nat._stream_ptr()))


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
        self.rope_table = None        # cuda fp32 [min(max_seq, max_pos), head_dim] of a rotary model
        prenorm = bool(shape.prenorm)
        rotary, gated = shape.rotary_theta > 0, bool(shape.gated) or bool(shape.gelu_gated)
        if rotary != gated:
            raise NotImplementedError("rotary_theta and gated come together (nomic-embed-text): no loader builds one without the other")
        if prenorm != bool(shape.gelu_gated) or (prenorm and shape.gated):
            raise NotImplementedError("prenorm and gelu_gated come together (ModernBERT): no loader builds one without the other")
        if prenorm and (not rotary or shape.local_theta <= 0 or shape.window < 1 or shape.global_every < 1):
            raise ValueError("a prenorm model needs rotary_theta > 0, local_theta > 0, window >= 1 and global_every >= 1")
        if rotary and (shape.rel_buckets or shape.pos_offset):
            raise ValueError("a rotary model has no position table: rel_buckets and pos_offset must be 0")
        flags = (ENC_ROTARY if rotary else 0) | (ENC_GATED_SILU if shape.gated else 0)
        flags |= (ENC_PRENORM | ENC_GATED_GELU) if prenorm else 0
        self.desc = EncoderDesc(shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.ffn,
                                shape.max_pos - shape.pos_offset, shape.ln_eps, POOL_CLS if shape.pooling == "cls" else POOL_MEAN, flags)
        self._layers = (EncoderLayer * shape.layers)()

        def keep(arr, dtype=None):
            t = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(self.device)
            t = t.to(dtype).contiguous() if dtype is not None else t
            self._keep.append(t)
            return t

        def bias_or_zeros(name, n):      # a checkpoint without this bias: a zero vector, so no kernel changes
            return keep(weights[name] if name in weights else np.zeros(n, dtype=np.float32))

        def nomic_layer(i):
            """the 12 tensors of crs_encoder_layer from NomicBertModel's names; biases only where the checkpoint carries them: zero
            vectors for b_qkv / b_o / b_down otherwise, and an EMPTY b_up (NULL for the library)"""
            p, h = f"layers.{i}.", shape.hidden
            bq = [np.asarray(weights.get(p + f"self_attn.{n}_proj.bias", np.zeros(h)), dtype=np.float32) for n in "qkv"]
            if p + "mlp.gate_proj.bias" in weights and p + "mlp.up_proj.bias" in weights:
                b_up = interleave_gate_up(weights[p + "mlp.gate_proj.bias"], weights[p + "mlp.up_proj.bias"])
            else:
                b_up = np.zeros(0, dtype=np.float32)
            return [
                dev16(p + "self_attn.q_proj.weight", p + "self_attn.k_proj.weight", p + "self_attn.v_proj.weight"),
                keep(np.concatenate(bq)),
                dev16(p + "self_attn.o_proj.weight"), bias_or_zeros(p + "self_attn.o_proj.bias", h),
                dev32(p + "post_attention_layernorm.weight"), dev32(p + "post_attention_layernorm.bias"),
                keep(interleave_gate_up(weights[p + "mlp.gate_proj.weight"], weights[p + "mlp.up_proj.weight"]), torch.float16),
                keep(b_up),
                dev16(p + "mlp.down_proj.weight"), bias_or_zeros(p + "mlp.down_proj.bias", h),
                dev32(p + "post_mlp_layernorm.weight"), dev32(p + "post_mlp_layernorm.bias"),
            ]

        empty = np.zeros(0, dtype=np.float32)      # an EMPTY vector is NULL for the library

        def modernbert_layer(i):
            """the 12 tensors of crs_encoder_layer from ModernBertModel's names: ln1 = attn_norm (absent on layer 0: identity), ln2 =
            mlp_norm; biases only where the checkpoint carries them, EMPTY (NULL) otherwise"""
            p = f"layers.{i}."

            def opt(name, arr=None):
                return keep(weights[name] if arr is None else arr) if name in weights else keep(empty)

            if i > 0 and p + "attn_norm.weight" not in weights:
                raise ValueError(f"{p}attn_norm.weight is missing (only layer 0 has no attention norm)")
            if i == 0 and (p + "attn_norm.weight" in weights or p + "attn_norm.bias" in weights):
                raise ValueError(f"{p}attn_norm.* is present: layer 0 of a pre-norm model has no attention norm, and the forward would ignore it")
            wi_b = interleave_wi(weights[p + "mlp.Wi.bias"]) if p + "mlp.Wi.bias" in weights else None
            return [
                dev16(p + "attn.Wqkv.weight"), opt(p + "attn.Wqkv.bias"),
                dev16(p + "attn.Wo.weight"), opt(p + "attn.Wo.bias"),
                opt(p + "attn_norm.weight"), opt(p + "attn_norm.bias"),
                keep(interleave_wi(weights[p + "mlp.Wi.weight"]), torch.float16), opt(p + "mlp.Wi.bias", wi_b),
                dev16(p + "mlp.Wo.weight"), opt(p + "mlp.Wo.bias"),
                dev32(p + "mlp_norm.weight"), opt(p + "mlp_norm.bias"),
            ]

        def bert_layer(i):
            p = f"encoder.layer.{i}."
            return [
                dev16(p + "attention.self.query.weight", p + "attention.self.key.weight", p + "attention.self.value.weight"),
                cat32(p + "attention.self.query.bias", p + "attention.self.key.bias", p + "attention.self.value.bias"),
                dev16(p + "attention.output.dense.weight"), dev32(p + "attention.output.dense.bias"),
                dev32(p + "attention.output.LayerNorm.weight"), dev32(p + "attention.output.LayerNorm.bias"),
                dev16(p + "intermediate.dense.weight"), dev32(p + "intermediate.dense.bias"),
                dev16(p + "output.dense.weight"), dev32(p + "output.dense.bias"),
                dev32(p + "output.LayerNorm.weight"), dev32(p + "output.LayerNorm.bias"),
            ]

        layer_tensors = []
        for i in range(shape.layers):
            vals = modernbert_layer(i) if prenorm else nomic_layer(i) if rotary else bert_layer(i)
            layer_tensors += vals
            for (fname, _), t in zip(EncoderLayer._fields_, vals):
                setattr(self._layers[i], fname, t.data_ptr() if t.numel() else None)
        if rotary:      # an EMPTY position table: NULL for the library, which then adds no position row
            pos = keep(np.zeros((0, shape.hidden), dtype=np.float32))
        else:           # (a contiguous view of the kept tensor from its row pos_offset on)
            pos = dev32("embeddings.position_embeddings.weight")[shape.pos_offset:]
        if prenorm:     # ModernBERT: no token types (a zero row), norms without bias unless the checkpoint carries one
            emb = [dev32("embeddings.tok_embeddings.weight"), pos, keep(np.zeros((1, shape.hidden), dtype=np.float32)),
                   dev32("embeddings.norm.weight"), bias_or_zeros("embeddings.norm.bias", shape.hidden)]
        else:
            emb = [dev32("embeddings.word_embeddings.weight"), pos, dev32("embeddings.token_type_embeddings.weight"),
                   dev32("embeddings.LayerNorm.weight"), dev32("embeddings.LayerNorm.bias")]
        self.weights = EncoderWeights(*[t.data_ptr() if t.numel() else None for t in emb], ctypes.cast(self._layers, POINTER(EncoderLayer)))
        self._ws = None
        # the same tensors in the order torch.ops.crs.encoder_forward takes them (csrc/torch_ops.cpp): embeddings, then 12 per layer
        self._wlist = emb + layer_tensors
        assert len(self._wlist) == 5 + 12 * shape.layers
        if rotary:
            self.rope_table = torch.from_numpy(rope_table(min(shape.max_seq, shape.max_pos), shape.hidden // shape.heads,
                                                          shape.rotary_theta)).to(self.device)
        self.rope_local = self.final_ln = None
        if prenorm:
            self.rope_local = torch.from_numpy(rope_table(min(shape.max_seq, shape.max_pos), shape.hidden // shape.heads,
                                                          shape.local_theta)).to(self.device)
            self.final_ln = (dev32("final_norm.weight"), dev32("final_norm.bias") if "final_norm.bias" in weights else None)
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

    def prenorm_plan_describe(self, batch: int, seq: int) -> str:
        """The launches of a pre-norm model's forward on the current device, one line each (crs_encoder_prenorm_plan_describe): the
        full-attention layers' attention line, then the sliding layers'."""
        lib = nat.load()
        return _describe(lambda sl, buf, cap: lib.crs_encoder_prenorm_plan_describe(byref(self.desc), batch, seq, int(self.shape.window), buf, cap))[0]

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
            if self.desc.flags & ENC_PRENORM:
                nat.ops().encoder_forward_prenorm(ids, lens, self._wlist, desc, float(self.desc.ln_eps), ws, out, q16_out,
                                                  int(slab_type), bool(normalize), hidden, self.rope_table, self.rope_local,
                                                  int(self.shape.window), int(self.shape.global_every), self.final_ln[0], self.final_ln[1])
            elif self.desc.flags & ENC_ROTARY:
                nat.ops().encoder_forward_rope(ids, lens, self._wlist, desc, float(self.desc.ln_eps), ws, out, q16_out,
                                               int(slab_type), bool(normalize), hidden, self.rel_bias, self.rope_table)
            else:
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
