"""References of the hybrid-retrieval tests (no tests here).

  bm25_topk_ref      crs_bm25_topk (csrc/bm25.hip; include/crs_hip.h) restated operation for operation in numpy fp32 scalars: same
                     inputs, same bits.
  bm25_textbook      Okapi BM25 with Lucene's non-negative idf in Python floats (fp64), from collections.Counter on the raw
                     documents: independent of the collection's token CSR.
  fuse_rrf_ref       crs_fuse_rrf (csrc/fuse.hip) in Python floats.
  corpus / queries   the seeded Zipf-like documents and queries the CPU and GPU tests share.
"""
import math
from collections import Counter

import numpy as np

EPS32 = 2.0 ** -24


def bm25_scores_ref(doc_off, doc_tok, doc_tf, doc_len, n_rows, q_tok, q_w, c0, c1, k1p1):
    """bm25_scores_scalar over arrays: the same fp32 operations element by element, the terms of a row added one at a time in
    ascending token id (the m-th matching token of every row in pass m), so the bits are the scalar loop's (test_bm25_cpu pins it)."""
    f32 = np.float32
    c0, c1, k1p1 = f32(c0), f32(c1), f32(k1p1)
    scores = np.zeros(n_rows, dtype=np.float32)
    hit = np.zeros(n_rows, dtype=bool)
    q_tok, q_w = np.asarray(q_tok, dtype=np.int64), np.asarray(q_w, dtype=np.float32)
    if q_tok.size == 0 or n_rows == 0:
        return scores, hit
    idx = np.nonzero(np.isin(doc_tok, q_tok))[0]                     # CSR order: row ascending, token id ascending inside a row
    if idx.size == 0:
        return scores, hit
    rows = np.searchsorted(doc_off[: n_rows + 1], idx, side="right") - 1
    w = q_w[np.searchsorted(q_tok, doc_tok[idx])]
    tf = doc_tf[idx].astype(np.float32)
    scaled = c1 * doc_len[rows].astype(np.float32)
    dn = c0 + scaled
    num = tf * k1p1
    den = tf + dn
    prod = w * num
    term = prod / den
    assert term.dtype == np.float32
    start = np.r_[0, np.nonzero(np.diff(rows))[0] + 1]              # first matching entry of each row
    rank = np.arange(idx.size) - np.repeat(start, np.diff(np.r_[start, idx.size]))
    order = np.argsort(rank, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(rank))]
    for m in range(len(bounds) - 1):
        sel = order[bounds[m]: bounds[m + 1]]
        scores[rows[sel]] = scores[rows[sel]] + term[sel]
    hit[rows] = True
    return scores, hit


def bm25_scores_scalar(doc_off, doc_tok, doc_tf, doc_len, n_rows, q_tok, q_w, c0, c1, k1p1):
    """fp32 scores [n_rows] and hit flags of ONE query (q_tok ascending distinct ids, q_w their fp32 weights) over the CSR rows:
    csrc/bm25.hip operation for operation with np.float32 scalars."""
    f32 = np.float32
    c0, c1, k1p1 = f32(c0), f32(c1), f32(k1p1)
    weight = {int(t): f32(w) for t, w in zip(q_tok, q_w)}
    scores = np.zeros(n_rows, dtype=np.float32)
    hit = np.zeros(n_rows, dtype=bool)
    if not weight:
        return scores, hit
    wanted = np.isin(doc_tok, np.fromiter(weight, dtype=np.int64, count=len(weight)))
    cand = np.unique(np.searchsorted(doc_off, np.nonzero(wanted)[0], side="right") - 1)
    for r in cand.tolist():
        lo, hi = int(doc_off[r]), int(doc_off[r + 1])
        dn = c0 + c1 * f32(int(doc_len[r]))
        acc = f32(0.0)
        for t in range(lo, hi):                       # ascending token id: the row's ids are sorted
            w = weight.get(int(doc_tok[t]))
            if w is None:
                continue
            tf = f32(int(doc_tf[t]))
            num = tf * k1p1
            den = tf + dn
            prod = w * num
            acc = acc + prod / den
            hit[r] = True
        scores[r] = acc
    return scores, hit


def topk_of(scores, hit, k):
    """(scores fp32 [k], rows int64 [k]): the hits by score descending, ties by lower row; (-inf, -1) past them."""
    rows = np.nonzero(hit)[0]
    order = rows[np.lexsort((rows, -scores[rows].astype(np.float64)))][:k]
    out_s = np.full(k, -np.inf, dtype=np.float32)
    out_r = np.full(k, -1, dtype=np.int64)
    out_s[: order.size], out_r[: order.size] = scores[order], order
    return out_s, out_r


def bm25_topk_ref(doc_off, doc_tok, doc_tf, doc_len, n_rows, q_off, q_tok, q_w, c0, c1, k1p1, k):
    """The kernel's outputs for a query batch: (scores fp32 [nq, k], rows int64 [nq, k])."""
    doc_off, doc_tok, doc_tf, doc_len = (np.asarray(a) for a in (doc_off, doc_tok, doc_tf, doc_len))
    q_off, q_tok, q_w = np.asarray(q_off), np.asarray(q_tok), np.asarray(q_w)
    nq = len(q_off) - 1
    out_s = np.full((nq, k), -np.inf, dtype=np.float32)
    out_r = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        lo, hi = int(q_off[q]), int(q_off[q + 1])
        s, h = bm25_scores_ref(doc_off, doc_tok, doc_tf, doc_len, n_rows, q_tok[lo:hi], q_w[lo:hi], c0, c1, k1p1)
        out_s[q], out_r[q] = topk_of(s, h, k)
    return out_s, out_r


def constants(n_rows, total_len, k1=1.5, b=0.75):
    """(c0, c1, k1 + 1): fp64, each rounded once to fp32 (include/crs_hip.h)."""
    c1 = k1 * b / (total_len / n_rows) if total_len > 0 and n_rows > 0 else 0.0
    return np.float32(k1 * (1.0 - b)), np.float32(c1), np.float32(k1 + 1.0)


def weight(n_rows, df):
    return np.float32(math.log(1.0 + (n_rows - df + 0.5) / (df + 0.5)))


class Textbook:
    """fp64 BM25 from the raw documents: Counter per document, df over the collection, nothing of the product's code."""

    def __init__(self, documents, k1=1.5, b=0.75):
        self.k1, self.b = k1, b
        self.counts = [Counter(d.lower().split()) for d in documents]
        self.lens = [sum(c.values()) for c in self.counts]
        self.n = len(documents)
        self.total = sum(self.lens)
        self.avgdl = self.total / self.n if self.total else 1.0
        self.df = Counter(w for c in self.counts for w in c)
        self.postings = {}
        for r, c in enumerate(self.counts):
            for w in c:
                self.postings.setdefault(w, []).append(r)

    def scores(self, query):
        """{row: (score fp64, matching terms)} of the rows that share a word with the query."""
        out = {}
        for w in sorted(set(query.lower().split())):
            df = self.df.get(w, 0)
            if not df:
                continue
            idf = math.log(1.0 + (self.n - df + 0.5) / (df + 0.5))
            for r in self.postings[w]:
                tf = self.counts[r][w]
                term = idf * (tf * (self.k1 + 1.0)) / (tf + self.k1 * (1.0 - self.b + self.b * self.lens[r] / self.avgdl))
                s, m = out.get(r, (0.0, 0))
                out[r] = (s + term, m + 1)
        return out


def fuse_rrf_ref(dense, lex, k_out, c=60.0, w_dense=1.0, w_lex=1.0):
    """crs_fuse_rrf for ONE query in Python floats: (rows, fused, dense_pos, lex_pos, count), padded with (-1, 0.0, -1, -1)."""
    dense, lex = [int(r) for r in dense], [int(r) for r in lex]
    d_at = {}
    for i, r in enumerate(dense):
        if r >= 0:
            d_at.setdefault(r, i)
    l_at = {}
    for j, r in enumerate(lex):
        if r >= 0:
            l_at.setdefault(r, j)
    cand = []
    inf = float("inf")
    for r in list(d_at) + [r for r in l_at if r not in d_at]:
        i, j = d_at.get(r), l_at.get(r)
        if i is not None and j is not None:
            f = w_dense / ((c + float(i)) + 1.0) + w_lex / ((c + float(j)) + 1.0)
        elif i is not None:
            f = w_dense / ((c + float(i)) + 1.0)
        else:
            f = w_lex / ((c + float(j)) + 1.0)
        cand.append((-f, inf if i is None else i, inf if j is None else j, r))
    cand.sort()
    cand = cand[:k_out]
    rows = [r for *_, r in cand] + [-1] * (k_out - len(cand))
    fused = [-f for f, *_ in cand] + [0.0] * (k_out - len(cand))
    dpos = [(-1 if i == inf else int(i)) for _, i, _, _ in cand] + [-1] * (k_out - len(cand))
    lpos = [(-1 if j == inf else int(j)) for _, _, j, _ in cand] + [-1] * (k_out - len(cand))
    return (np.array(rows, dtype=np.int64), np.array(fused, dtype=np.float64), np.array(dpos, dtype=np.int32),
            np.array(lpos, dtype=np.int32), len(cand))


# ---- the seeded corpus the CPU and GPU tests share ------------------------------------------------------------------------------------
VOCAB = 2000
STOP = "the"
CHUNK_TOKENS = 2048          # kChunk of csrc/bm25.hip: one row of the corpus is longer


def corpus(n_rows, seed=11, long_row=True, duplicates=20):
    """n_rows Zipf-like documents over a 2000-word vocabulary: the stopword in every non-empty document, repeated words (tf > 1),
    5 % empty documents, (n_rows >= 40) one row of more distinct tokens than the kernel stages per round among short ones, and
    `duplicates` exact copies of one document spread over the rows."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    docs = []
    for r in range(n_rows):
        if n_rows > 1 and rng.random() < 0.05:
            docs.append("")
            continue
        n = int(rng.integers(3, 120))
        words = [f"w{t}" for t in rng.choice(VOCAB, size=n, p=p).tolist()]
        docs.append(" ".join([STOP] + words + [STOP] * int(rng.integers(0, 3))))
    if n_rows >= 40:
        if long_row:
            docs[n_rows // 3] = " ".join([STOP] + [f"w{t}" for t in range(VOCAB)] + [f"x{t}" for t in range(600)] + ["w7", "w7", "w3"])
        dup = "the w1987 w1993 w1993 w1999 rareword w1971 w1971 w1971"     # rare words: random queries seldom rank the copies
        for r in rng.choice(np.arange(n_rows // 2, n_rows), size=min(duplicates, n_rows // 2), replace=False).tolist():
            docs[r] = dup
    return docs


def queries(n, seed=5):
    """n queries: the stopword and 1..7 Zipf words each; query 1 knows no word, query 2 hits fewer rows than any k, query 3 (n >= 4)
    has 200 distinct words, query 4 matches the duplicate documents."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    out = []
    for i in range(n):
        words = [f"w{t}" for t in rng.choice(VOCAB, size=int(rng.integers(1, 8)), p=p).tolist()]
        out.append(" ".join([STOP.upper() if i % 2 else STOP] + words))
    if n > 1:
        out[1] = "zzz-unknown never-seen"
    if n > 2:
        out[2] = "rareword"
    if n > 3:
        out[3] = " ".join([STOP] + [f"w{t}" for t in range(40, 239)])
    if n > 4:
        out[4] = "the w1993 w1971 rareword w1999"
    return out


def plain_queries(n, seed=9):
    """n queries without special cases, for the comparison of row sets with the fp64 textbook: the stopword, two of the 30 most
    frequent words and 1..5 Zipf words, so that far more than k rows match several terms and the k-th score is seldom tied."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    out = []
    for _ in range(n):
        words = [f"w{t}" for t in rng.choice(30, size=2, replace=False).tolist()]
        words += [f"w{t}" for t in rng.choice(VOCAB, size=int(rng.integers(1, 6)), p=p).tolist()]
        out.append(" ".join([STOP] + words))
    return out
