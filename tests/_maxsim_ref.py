"""fp64 restatements, error bounds and input generators of the late-interaction tests (tests/test_late_interaction_cpu.py,
tests/test_maxsim_gpu.py, tests/test_late_interaction_gpu.py).  Plain numpy; nothing here touches a device.

MaxSim (csrc/maxsim.hip):   out[q][c] = sum_{i < q_len[q]} max_{j in doc} <q_i, d_j>,  doc = tokens [offsets[r], offsets[r + 1]) of
r = rows[q][c]; -inf for a row outside [0, n_rows); 0 for an empty document or query.

Its error bound, with u = 2^-24, derived (not measured):

    |err| <= 2 u [ (dimp + 1) sum_i |q_i| max_j |d_j|  +  q_len sum_i |max_i| ]

  * the products of two fp16 numbers are exact in fp32; a dot product of dimp of them accumulated in fp32 in ANY order is off by at
    most gamma_dimp sum_k |q_ik d_jk| <= (dimp + 1) u |q_i| |d_j| (Cauchy-Schwarz); the factor 2 covers the matrix core's unspecified
    internal summation order and its accumulation across k-steps;
  * a maximum moves by no more than its arguments do, so row i's maximum is off by at most (dimp + 1) u |q_i| max_j |d_j|;
  * adding q_len maxima in fp32 in a fixed order is off by at most (q_len - 1) u sum_i |max_i| to first order.

The projection (csrc/token_project.hip): y = v / |v|, v = W h (+ b) with h rounded to fp16 on load.  First-order bound per element
j, against fp64 over the SAME fp32 hidden states and fp16 weights:

    4 [ (2^-10 + (H + 1) u) sum_k |W_jk| |h_k| / |v| ] + 2^-11

(2^-10 bounds the rounding of h to fp16 twice over, (H + 1) u the fp32 accumulation, the factor 4 the norm's share and the
division, 2^-11 the final rounding of |y_j| <= 1 to fp16.)
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24


def dimp_of(dim: int) -> int:
    return (int(dim) + 31) // 32 * 32


# ---------------------------------------------------------------------------------------------------------------- MaxSim
def maxsim_ref(q16, q_len, tok16, offsets, rows):
    """(scores fp64 [nq, m_max], bound fp64 [nq, m_max]) from the fp16 inputs themselves; the bound is the docstring's (0 where the
    score is exact by rule: a bad row, an empty document, an empty query)."""
    q = np.asarray(q16).astype(np.float64)
    t = np.asarray(tok16).astype(np.float64)
    offsets = np.clip(np.asarray(offsets, dtype=np.int64), 0, t.shape[0])
    rows = np.asarray(rows, dtype=np.int64)
    nq, lq_max, dimp = q.shape
    n_rows = len(offsets) - 1
    out = np.zeros(rows.shape, dtype=np.float64)
    bound = np.zeros(rows.shape, dtype=np.float64)
    tnorm = np.sqrt((t * t).sum(1))
    for a in range(nq):
        lq = int(min(max(int(q_len[a]), 0), lq_max))
        qa = q[a, :lq]
        qnorm = np.sqrt((qa * qa).sum(1))
        for c in range(rows.shape[1]):
            r = int(rows[a, c])
            if r < 0 or r >= n_rows:
                out[a, c] = -np.inf
                continue
            t0, t1 = int(offsets[r]), int(offsets[r + 1])
            if lq == 0 or t1 <= t0:
                continue
            best = (qa @ t[t0:t1].T).max(1)
            out[a, c] = best.sum()
            bound[a, c] = 2.0 * U * ((dimp + 1) * qnorm.sum() * tnorm[t0:t1].max() + lq * np.abs(best).sum())
    return out, bound


def maxsim_brute(q16, q_len, tok16, offsets, rows):
    """The same scores by three nested loops over python floats (small cases only)."""
    q = np.asarray(q16).astype(np.float64)
    t = np.asarray(tok16).astype(np.float64)
    n_tokens, n_rows = t.shape[0], len(offsets) - 1
    out = np.zeros(np.shape(rows), dtype=np.float64)
    for a in range(q.shape[0]):
        lq = min(max(int(q_len[a]), 0), q.shape[1])
        for c in range(np.shape(rows)[1]):
            r = int(rows[a][c])
            if r < 0 or r >= n_rows:
                out[a, c] = -np.inf
                continue
            t0 = min(max(int(offsets[r]), 0), n_tokens)
            t1 = min(max(int(offsets[r + 1]), 0), n_tokens)
            if lq == 0 or t1 <= t0:
                continue
            total = 0.0
            for i in range(lq):
                best = -np.inf
                for j in range(t0, t1):
                    dot = 0.0
                    for k in range(q.shape[2]):
                        dot += float(q[a, i, k]) * float(t[j, k])
                    best = max(best, dot)
                total += best
            out[a, c] = total
    return out


def _unit16(x):
    x = x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-30)
    return x.astype(np.float16)


DOC_LENS = (0, 1, 15, 16, 17, 31, 33, 180, 513)
Q_LENS = (0, 1, 15, 16, 17, 32, 33, 64)


def make_case(seed: int, dimp: int, nq: int, m_max: int, lq_max: int = 64, q_lens=None, doc_lens=DOC_LENS, poison_padding: bool = True):
    """One launch's inputs: unit-length fp16 token vectors (zeros in the last 3 coordinates when dimp > 32: a dim that is no
    multiple of 32), documents of `doc_lens` tokens in shuffled order, each a mix of noise and of copies of query tokens at a
    strength drawn per document (so the scores spread over a wide range), and rows [nq, m_max] drawn from them.  Query rows at and
    past q_len carry LARGE values (poison_padding): a kernel that reads them shows it."""
    rng = np.random.default_rng(seed)
    dim = dimp - 3 if dimp > 32 else dimp
    q_lens = list(Q_LENS if q_lens is None else q_lens)
    q_len = np.asarray([q_lens[i % len(q_lens)] for i in range(nq)], dtype=np.int32)
    q_len = np.minimum(q_len, lq_max).astype(np.int32)
    q = np.zeros((nq, lq_max, dimp), dtype=np.float64)
    q[:, :, :dim] = rng.standard_normal((nq, lq_max, dim))
    q16 = _unit16(q)
    lens = np.asarray(doc_lens, dtype=np.int64)[rng.permutation(len(doc_lens))]
    offsets = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    tok = np.zeros((int(offsets[-1]), dimp), dtype=np.float64)
    tok[:, :dim] = rng.standard_normal((tok.shape[0], dim))
    flat_q = q16.astype(np.float64).reshape(-1, dimp)
    for r in range(len(lens)):
        strength = rng.uniform(0.0, 2.5)
        for j in range(int(offsets[r]), int(offsets[r + 1])):
            tok[j] = _unit16(tok[j]).astype(np.float64) + strength * rng.uniform(0.0, 1.0) * flat_q[rng.integers(0, flat_q.shape[0])]
    tok16 = _unit16(tok)
    if poison_padding:
        for a in range(nq):
            q16[a, q_len[a]:] = np.float16(200.0)
    rows = rng.integers(0, len(lens), (nq, m_max)).astype(np.int64)
    return {"q16": q16, "q_len": q_len, "tok16": tok16, "offsets": offsets, "rows": rows, "n_rows": len(lens)}


def ordering_case(seed: int = 41, dimp: int = 128, m_max: int = 64):
    """The ordering test's input: 5 queries of 32 tokens, 64 documents of 20-180 tokens, every document once per list."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 181, m_max)
    case = make_case(seed, dimp, 5, m_max, lq_max=32, q_lens=[32], doc_lens=tuple(int(x) for x in lens))
    case["rows"] = np.stack([rng.permutation(m_max) for _ in range(5)]).astype(np.int64)
    return case


def separated_fraction(scores, bound) -> float:
    """Fraction of adjacent pairs, in each list's descending fp64 order, whose gap exceeds twice the larger of the two bounds."""
    good = total = 0
    for s, b in zip(scores, bound):
        order = np.argsort(-s, kind="stable")
        for x, y in zip(order[:-1], order[1:]):
            total += 1
            good += (s[x] - s[y]) > 2.0 * max(b[x], b[y])
    return good / max(total, 1)


# ---------------------------------------------------------------------------------------------------------------- projection
def project_ref(hidden32, w16, bias32, dst, dim: int):
    """(y fp64 [slots, dimp], bound fp64 [slots, dimp], written bool [slots]) of crs_token_project: slot dst[t] <- the unit vector of
    W h_t (+ b), zeros in [dim, dimp) and for a zero v; slots = max(dst) + 1.  Rows with dst < 0 are not looked at."""
    h = np.asarray(hidden32, dtype=np.float32)
    w = np.asarray(w16).astype(np.float64)
    dst = np.asarray(dst, dtype=np.int64)
    dimp = dimp_of(dim)
    slots = int(dst.max()) + 1 if dst.size and dst.max() >= 0 else 0
    y = np.zeros((slots, dimp))
    bound = np.full((slots, dimp), 2.0 ** -11)
    written = np.zeros(slots, dtype=bool)
    H = h.shape[1]
    for t in np.flatnonzero(dst >= 0):
        ht = h[t].astype(np.float64)
        v = w @ ht + (0.0 if bias32 is None else np.asarray(bias32, dtype=np.float64))
        norm = np.sqrt((v * v).sum())
        written[dst[t]] = True
        if norm == 0.0:
            continue
        y[dst[t], :dim] = v / norm
        bound[dst[t], :dim] += 4.0 * (2.0 ** -10 + (H + 1) * U) * (np.abs(w) @ np.abs(ht)) / norm
    return y, bound, written


# ---------------------------------------------------------------------------------------------------------------- high offsets
HIGH_DIMP = 128
HIGH_TOKENS = (1 << 24) + 1061
HIGH_HEAD = 64                              # the queries' support; background tokens live on [64, 128)
HIGH_DOC = 40                               # tokens of a planted document
HIGH_CONTROL = 3000                         # first token of the low-address control document
HIGH_LINES = (1 << 23, 1 << 24)             # token offsets of 2^31 bytes and of 2^32 bytes (= 2^31 elements) at 256 bytes a token
HIGH_SEED = 20_261_021


def high_offsets() -> np.ndarray:
    """CSR offsets of 8 rows: the odd rows are the planted documents -- a low-address control, one across each line, the last
    tokens of the array -- and the even rows the background between them.  The control starts at token HIGH_CONTROL, far from
    token 0: an offset wrapped at 2^31 or 2^32 bytes (or elements) lands on tokens 0..HIGH_DOC, which are background only."""
    cuts = [0, HIGH_CONTROL, HIGH_CONTROL + HIGH_DOC]
    for line in HIGH_LINES:
        cuts += [line - HIGH_DOC // 2, line + HIGH_DOC // 2]
    cuts += [HIGH_TOKENS - HIGH_DOC + 3, HIGH_TOKENS]
    return np.asarray(cuts, dtype=np.int64)


HIGH_PLANTED_ROWS = (1, 3, 5, 7)


def high_queries(nq: int = 3, lq: int = 20):
    """fp16 [nq, lq, 128] unit vectors on coordinates [0, 64)."""
    rng = np.random.default_rng(HIGH_SEED)
    q = np.zeros((nq, lq, HIGH_DIMP))
    q[:, :, :HIGH_HEAD] = rng.standard_normal((nq, lq, HIGH_HEAD))
    return _unit16(q)


def high_planted():
    """row -> fp16 [tokens, 128]: the planted documents' tokens, each a mix of a query token and noise on [0, 64), a different
    strength per document so that no two documents score alike."""
    rng = np.random.default_rng(HIGH_SEED + 1)
    q = high_queries().astype(np.float64).reshape(-1, HIGH_DIMP)
    off = high_offsets()
    out = {}
    for n, r in enumerate(HIGH_PLANTED_ROWS):
        m = int(off[r + 1] - off[r])
        x = np.zeros((m, HIGH_DIMP))
        x[:, :HIGH_HEAD] = 0.5 * rng.standard_normal((m, HIGH_HEAD)) / np.sqrt(HIGH_HEAD)
        x += (0.9 - 0.15 * n) * q[rng.integers(0, q.shape[0], m)]
        out[r] = _unit16(x)
    return out
