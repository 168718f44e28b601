"""References of the learned-sparse-retrieval tests (no tests here).

  f16                round an array to fp16 (nearest even) and give it back in fp64: the operands the device multiplies.
  transform_ref      cls.predictions.transform in fp64: t = LayerNorm(GELU(W_t h + b_t)), erf-form GELU, biased variance.
  pool_ref           out[b, v] = log1p(max(0, max_{i < lens[b]} (t_i . Wd_v + bias_v))) in fp64, and per (b, v) the largest
                     sum_k |t_ik Wd_vk| over the text's real tokens: what the rounding bound of a device result is made of.
  head_ref           the two chained, nothing rounded: the whole head in fp64.
  pool_bound         2 gamma_K sum|a_k w_k| + one fp32 ulp of the result (derived in its docstring).
  compact_ref        crs_sparse_compact (csrc/sparse_compact.hip) for one row, in numpy.
  sparse_scores_ref  crs_sparse_topk's scores (csrc/sparse_scan.hip) restated operation for operation in numpy fp32: same bits.
  sparse_topk_ref    the kernel's outputs for a query batch.
  corpus / queries   the seeded short texts the CPU and GPU retrieval tests share.
  model_reference    a SparseEncoder's whole computation in fp64 on the CPU (oracle/encoder_ref.py's BERT, then head_ref).
"""
import math

import numpy as np

from _bm25_ref import topk_of

U32 = 2.0 ** -24            # unit roundoff of fp32


def f16(a):
    return np.asarray(a).astype(np.float16).astype(np.float64)


def _erf(x):
    import torch
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def transform_ref(hidden, w_t, b_t, gamma, beta, eps):
    """fp64 [..., H]: LayerNorm(GELU(hidden W_t^T + b_t)); w_t is [out, in] as torch.nn.Linear stores it."""
    x = np.asarray(hidden, dtype=np.float64) @ np.asarray(w_t, dtype=np.float64).T + np.asarray(b_t, dtype=np.float64)
    x = 0.5 * x * (1.0 + _erf(x / math.sqrt(2.0)))
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + float(eps)) * np.asarray(gamma, dtype=np.float64) + np.asarray(beta, dtype=np.float64)


def pool_ref(t, lens, w_d, bias):
    """t fp64 [batch, seq, H]; lens [batch]; w_d [V, H]; bias [V] -> (weights fp64 [batch, V], absdot fp64 [batch, V]).  Positions at
    or past lens[b] are not looked at (they may hold NaN)."""
    t, w_d, bias = np.asarray(t, dtype=np.float64), np.asarray(w_d, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    batch, V = t.shape[0], w_d.shape[0]
    out = np.zeros((batch, V))
    absdot = np.zeros((batch, V))
    for b in range(batch):
        n = int(lens[b])
        if n <= 0:
            continue
        logits = t[b, :n] @ w_d.T + bias
        out[b] = np.log1p(np.maximum(logits.max(0), 0.0))
        absdot[b] = (np.abs(t[b, :n]) @ np.abs(w_d).T).max(0)
    return out, absdot


def head_ref(hidden, lens, w_t, b_t, gamma, beta, eps, w_d, bias):
    """The whole head in fp64 from unrounded operands: weights fp64 [batch, V]."""
    hidden = np.asarray(hidden, dtype=np.float64)
    t = np.zeros_like(hidden)
    for b in range(hidden.shape[0]):
        n = int(lens[b])
        t[b, :n] = transform_ref(hidden[b, :n], w_t, b_t, gamma, beta, eps)
    return pool_ref(t, lens, w_d, bias)[0]


def pool_bound(absdot, result, K):
    """Derived, not fitted.  The device multiplies fp16 operands exactly (an fp16 x fp16 product has 22 significant bits) and adds
    the K products and the bias in fp32: K additions, each with relative error <= u = 2^-24, so a logit is off by at most
    gamma_K sum_k |a_k w_k| (gamma_K = K u / (1 - K u); the bias is the last addend and its rounding is within the same sum as
    long as |bias| <= K sum|a w|).  The factor 2 leaves room for the matrix instruction adding its 32 products of a step in an
    order of its own.  A maximum moves by no more than its largest argument does, and log1p is 1-Lipschitz on [0, inf), so the
    same bound holds after both; the device takes log1p in fp64 and rounds once: one fp32 ulp of the result covers that."""
    gamma = K * U32 / (1.0 - K * U32)
    ulp = np.spacing(np.abs(np.asarray(result)).astype(np.float32)).astype(np.float64)
    return 2.0 * gamma * np.asarray(absdot) + ulp


def compact_ref(row, cap, skip_ids=()):
    """(ids int32 [cap], weights fp32 [cap], count) of one fp32 row: the ids with weight > 0 outside skip_ids; the cap largest when
    there are more, ties by lower id; ascending id; (-1, 0) in the unused slots."""
    row = np.asarray(row, dtype=np.float32)
    ok = row > 0                                       # NaN and -0.0 are not
    for s in skip_ids:
        if 0 <= s < row.shape[0]:
            ok[s] = False
    ids = np.nonzero(ok)[0]
    if ids.size > cap:
        order = np.lexsort((ids, -row[ids].astype(np.float64)))         # weight descending, id ascending
        ids = np.sort(ids[order[:cap]])
    out_i = np.full(cap, -1, dtype=np.int32)
    out_w = np.zeros(cap, dtype=np.float32)
    out_i[: ids.size], out_w[: ids.size] = ids, row[ids]
    return out_i, out_w, int(ids.size)


def sparse_scores_ref(doc_off, doc_tok, doc_w, n_rows, q_tok, q_w):
    """fp32 scores [n_rows] and hit flags of ONE query (q_tok ascending distinct ids) over the CSR rows: the terms of a row added one
    at a time in ascending token id (the m-th matching token of every row in pass m), every product and sum rounded to fp32."""
    scores = np.zeros(n_rows, dtype=np.float32)
    hit = np.zeros(n_rows, dtype=bool)
    q_tok, q_w = np.asarray(q_tok, dtype=np.int64), np.asarray(q_w, dtype=np.float32)
    doc_off, doc_tok, doc_w = np.asarray(doc_off), np.asarray(doc_tok), np.asarray(doc_w, dtype=np.float32)
    if q_tok.size == 0 or n_rows == 0:
        return scores, hit
    total = doc_tok.shape[0]
    off = np.clip(doc_off[: n_rows + 1], 0, total)                  # (a well-formed CSR: ascending offsets)
    idx = np.nonzero(np.isin(doc_tok[: off[n_rows]], q_tok))[0]
    if idx.size == 0:
        return scores, hit
    rows = np.searchsorted(off, idx, side="right") - 1
    term = q_w[np.searchsorted(q_tok, doc_tok[idx])] * doc_w[idx]
    assert term.dtype == np.float32
    start = np.r_[0, np.nonzero(np.diff(rows))[0] + 1]
    rank = np.arange(idx.size) - np.repeat(start, np.diff(np.r_[start, idx.size]))
    order = np.argsort(rank, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(rank))]
    for m in range(len(bounds) - 1):
        sel = order[bounds[m]: bounds[m + 1]]
        scores[rows[sel]] = scores[rows[sel]] + term[sel]
    hit[rows] = True
    return scores, hit


def sparse_scores_scalar(doc_off, doc_tok, doc_w, n_rows, q_tok, q_w):
    """The same with np.float32 scalars in a plain loop; offsets clamped as the kernel clamps them (lo into [0, total], hi into
    [lo, total]), so it also serves a malformed CSR."""
    f32 = np.float32
    weight = {int(t): f32(w) for t, w in zip(q_tok, q_w)}
    scores = np.zeros(n_rows, dtype=np.float32)
    hit = np.zeros(n_rows, dtype=bool)
    total = len(doc_tok)
    for r in range(n_rows):
        lo = min(max(int(doc_off[r]), 0), total)
        hi = min(max(int(doc_off[r + 1]), lo), total)
        acc = f32(0.0)
        for t in range(lo, hi):
            w = weight.get(int(doc_tok[t]))
            if w is None:
                continue
            acc = acc + w * f32(doc_w[t])
            hit[r] = True
        scores[r] = acc
    return scores, hit


def sparse_topk_ref(doc_off, doc_tok, doc_w, n_rows, q_off, q_tok, q_w, k, scalar=False):
    """The kernel's outputs for a query batch: (scores fp32 [nq, k], rows int64 [nq, k])."""
    q_off, q_tok, q_w = np.asarray(q_off), np.asarray(q_tok), np.asarray(q_w)
    nq = len(q_off) - 1
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    score = sparse_scores_scalar if scalar else sparse_scores_ref
    for q in range(nq):
        lo, hi = int(q_off[q]), int(q_off[q + 1])
        s, h = score(doc_off, doc_tok, doc_w, n_rows, q_tok[lo:hi], q_w[lo:hi])
        out_s[q], out_r[q] = topk_of(s, h, k)
    return out_s, out_r


def csr_of(rows):
    """(offsets int64, tokens int32, weights fp32) of a list of (ids, weights) rows."""
    off = np.r_[0, np.cumsum([len(i) for i, _ in rows])].astype(np.int64)
    tok = np.concatenate([np.asarray(i, dtype=np.int32) for i, _ in rows]) if rows else np.zeros(0, dtype=np.int32)
    w = np.concatenate([np.asarray(x, dtype=np.float32) for _, x in rows]) if rows else np.zeros(0, dtype=np.float32)
    return off, tok.astype(np.int32), w.astype(np.float32)


# ---- the seeded texts the CPU and GPU retrieval tests share --------------------------------------------------------------------------
WORDS = ("retrieval augmented generation answers questions from compressed documents with a vector index and an encoder on the device "
         "while learned sparse models expand every text into weighted vocabulary terms so that rare identifiers still match exactly "
         "bm25 counts words splade learns them kernels scan rows merge lists fuse ranks").split()


def corpus(n: int, seed: int = 0):
    """n short texts of 1 to 30 words, each ending in a word of its own; text 1 is empty and text 2 longer than the model's max_seq."""
    rng = np.random.default_rng(seed)
    out = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(1, 31)))) + f" item{i}" for i in range(n)]
    if n > 3:
        out[1] = ""
        out[2] = " ".join(str(w) for w in rng.choice(WORDS, 200))
    return out


def queries(n: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    return [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(1, 9)))) for _ in range(n)]


TILE_N = 128          # kMlmTileN of csrc/mlm_plan.h: test_sparse_cpu.py pins it against crs_mlm_pool_plan, the GPU tests build shapes on it


def _head_f32(hidden, w_t, b_t, gamma, beta, eps, w_d, bias):
    """The head for one text in numpy fp32 throughout (erf through fp64, rounded): the fp32 model's own distance from fp64."""
    f = np.float32
    x = hidden.astype(f) @ np.asarray(w_t, dtype=f).T + np.asarray(b_t, dtype=f)
    x = (f(0.5) * x * (f(1.0) + _erf(x.astype(np.float64) / math.sqrt(2.0)).astype(f))).astype(f)
    mean = x.mean(-1, keepdims=True, dtype=f)
    var = ((x - mean) ** 2).mean(-1, keepdims=True, dtype=f)
    t = ((x - mean) / np.sqrt(var + f(eps)) * np.asarray(gamma, dtype=f) + np.asarray(beta, dtype=f)).astype(f)
    logits = t @ np.asarray(w_d, dtype=f).T + np.asarray(bias, dtype=f)
    return np.log1p(np.maximum(logits.max(0), f(0.0))).astype(np.float64)


def model_reference(weights, shape, token_ids, with_bound=False):
    """fp64 weights [n, V] and absdot [n, V] of texts given as token-id lists, from a SparseEncoder's host weights (internal names)
    and ModelShape: oracle.encoder_ref.encode_ref in fp64 for the hidden states, then the head in fp64.  Nothing is rounded.

    with_bound: also bound [n], what a device result for text i may differ from the fp64 weights by, in the form
    tests/_encoder_cases.py uses for the encoder -- computed from references alone, never from a device:
        bound = 2 E_q + 4 a + one fp32 ulp
        E_q = max_v |emulated - fp64|   the quantisation floor: fp64 arithmetic with a round trip through fp16 exactly where the
                                        kernels store or consume fp16 (the encoder's points of oracle/encoder_ref.py, then h, W_t,
                                        t and W_d in the head)
        a   = max_v |fp32 - fp64|       accumulation order: the plain fp32 model's own distance from fp64, times 4 because the
                                        device's summation order differs from numpy's as numpy's does from fp64's
    The factor 2 on E_q: a rounding point can fall the other way on the device than in the emulation (its input already differs
    in the last bits), which moves the result by up to twice the floor."""
    import torch
    from oracle import encoder_ref as er
    from rag import sparse as sp
    cfg = er.EncoderConfig(vocab_size=shape.vocab_size, hidden=shape.hidden, layers=shape.layers, heads=shape.heads, ffn=shape.ffn,
                           max_pos=shape.max_pos, max_seq=shape.max_seq, pooling="cls", ln_eps=shape.ln_eps)
    body = {k: v for k, v in weights.items() if k not in sp.HEAD}
    head = (weights[sp.T_DENSE_W], weights[sp.T_DENSE_B], weights[sp.T_LN_W], weights[sp.T_LN_B], shape.ln_eps)
    n, V = len(token_ids), shape.vocab_size
    lens = np.asarray([len(t) for t in token_ids], dtype=np.int64)
    ids = np.zeros((n, int(lens.max())), dtype=np.int64)
    for i, t in enumerate(token_ids):
        ids[i, : len(t)] = t
    mask = (np.arange(ids.shape[1])[None, :] < lens[:, None]).astype(np.int64)      # padding is masked out of the attention and the pool

    def rows(t, w_d):
        return pool_ref(t, lens, w_d, weights[sp.DEC_B])

    hidden = er.encode_ref(ids, mask, body, cfg, return_hidden=True, dtype=torch.float64)
    out, absdot = rows(transform_ref(hidden, *head), weights[sp.DEC_W])
    if not with_bound:
        return out, absdot
    hem = er.encode_ref(ids, mask, body, cfg, return_hidden=True, dtype=torch.float64, emulate_fp16=True)
    oem = rows(f16(transform_ref(f16(hem), f16(head[0]), *head[1:])), f16(weights[sp.DEC_W]))[0]
    h32 = er.encode_ref(ids, mask, body, cfg, return_hidden=True)
    o32 = np.stack([_head_f32(h32[i, : lens[i]], *head, weights[sp.DEC_W], weights[sp.DEC_B]) for i in range(n)])
    ulp = np.spacing(np.maximum(out.max(1), 1.0).astype(np.float32)).astype(np.float64)
    bound = 2.0 * np.abs(oem - out).max(1) + 4.0 * np.abs(o32 - out).max(1) + ulp
    return out, absdot, bound
