"""Pure-Python restatement of the post-search rule of ContextRetriever.retrieve_batch (cosine score, similarity_threshold, the
token-overlap re-rank and its stable sort), and the case generators of the re-rank tests.

A list is (scores fp32 [m], rows [m], texts, query, k, threshold): rows are indices into `texts` (negative = an empty slot, a row
at or past len(texts) = a candidate without text).  Arithmetic is Python floats (fp64), token sets are set(text.lower().split()),
the order is list.sort(reverse=True) -- nothing here shares code with rag/ or the kernel.

    dist = float(np.float32(1) - np.float32(score))        the store's distance (fp32 subtraction, as search_batch returns it)
    d = min(max(dist, 0), 2);  sim = min(max(1 - d * d / 2, 0), 1);  a NaN stays a NaN, as numpy's minimum / maximum keep it
    keep iff sim >= threshold
    kept > k:  rr = sim * 0.7 + (|query tokens & text tokens| / max(|query tokens|, 1)) * 0.3, stable sort by rr descending, first k
    else:      the first min(kept, k) kept

The outputs are laid out as the kernel's: order (input positions, -1 past the count), count, sim and rr by input position (0.0
where undefined: empty slots; rr of candidates that were not kept or of lists that were not re-ranked), reranked."""
import numpy as np

NAN = float("nan")

POOL = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine similarity "
        "vector index chunk context answer question compression memory latency throughput accuracy benchmark").split()
assert len(POOL) == 24


def similarity(dist):
    """_distance_to_similarity's cosine branch as retrieve_batch vectorises it (np.minimum / np.maximum propagate a NaN;
    Python's min / max do not, so that case is written out)."""
    if dist != dist:
        return NAN
    d = min(max(dist, 0.0), 2.0)
    return min(max(1.0 - (d * d / 2.0), 0.0), 1.0)


def post_search(dists, rows, texts, query, k, threshold):
    """The rule over fp64 distances -> dict(order, count, sim, rr, reranked) in the kernel's layout (see the module docstring)."""
    m = len(rows)
    sim, rr = [0.0] * m, [0.0] * m
    kept = []
    for pos in range(m):
        if rows[pos] < 0:
            continue
        sim[pos] = similarity(dists[pos])
        if sim[pos] >= threshold:
            kept.append(pos)
    reranked = 0
    if len(kept) > k:
        reranked = 1
        wanted = set(query.lower().split())
        norm = max(len(wanted), 1)
        for pos in kept:
            text = texts[rows[pos]] if rows[pos] < len(texts) else ""
            hits = len(wanted & set(text.lower().split()))
            rr[pos] = sim[pos] * 0.7 + (hits / norm) * 0.3
        kept.sort(key=lambda pos: rr[pos], reverse=True)
    kept = kept[:k]
    return {"order": kept + [-1] * (m - len(kept)), "count": len(kept), "sim": sim, "rr": rr, "reranked": reranked}


def rerank_ref(scores, rows, texts, query, k, threshold):
    """The rule over the store's fp32 scores."""
    dists = [float(np.float32(1.0) - np.float32(s)) for s in scores]
    return post_search(dists, [int(r) for r in rows], texts, query, k, threshold)


def rerank_ref_batch(scores, rows, texts, queries, k, threshold):
    """rerank_ref per list -> numpy arrays shaped as the kernel's outputs."""
    nq, m = rows.shape
    out = {"order": np.full((nq, m), -1, np.int32), "count": np.zeros(nq, np.int32), "sim": np.zeros((nq, m)), "rr": np.zeros((nq, m)),
           "reranked": np.zeros(nq, np.int32)}
    for i in range(nq):
        one = rerank_ref(scores[i], rows[i], texts, queries[i], k, threshold)
        out["order"][i], out["count"][i], out["reranked"][i] = one["order"], one["count"], one["reranked"]
        out["sim"][i], out["rr"][i] = one["sim"], one["rr"]
    return out


# ---- generators ---------------------------------------------------------------------------------------------------------------
def make_documents(n_rows, seed):
    """n_rows documents of 6-12 words: words of the 24-word POOL (mixed case now and then) plus one token only this row has."""
    rng = np.random.default_rng(seed)
    docs = []
    for r in range(n_rows):
        words = [POOL[j] for j in rng.integers(0, len(POOL), size=int(rng.integers(5, 12)))]
        if r % 7 == 0:
            words[0] = words[0].upper()
        words.insert(int(rng.integers(0, len(words) + 1)), f"u{r}")
        docs.append(" ".join(words))
    return docs


def make_lists(nq, m_max, k, n_rows, seed):
    """nq lists over rows [0, n_rows): (scores fp32 [nq, m_max] descending, rows int64 [nq, m_max] with -1 past each list's length,
    queries).  Lengths 0, 1, k, k + 1 and m_max lead (clipped to m_max), the others are random; a query is 2-7 POOL words, sometimes
    with a listed row's own token and sometimes with a word no document holds."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, m_max + 1, size=nq)
    lead = [0, 1, min(k, m_max), min(k + 1, m_max), m_max]
    lengths[:len(lead)] = lead
    scores = np.zeros((nq, m_max), dtype=np.float32)
    rows = np.full((nq, m_max), -1, dtype=np.int64)
    queries = []
    for i in range(nq):
        n = int(lengths[i])
        rows[i, :n] = rng.choice(n_rows, size=n, replace=False)
        scores[i, :n] = np.sort(rng.uniform(0.15, 0.97, size=n).astype(np.float32))[::-1]
        words = [POOL[j] for j in rng.integers(0, len(POOL), size=int(rng.integers(2, 8)))]
        if n and i % 3 == 0:
            words.append(f"u{int(rows[i, int(rng.integers(0, n))])}")
        if i % 5 == 0:
            words.append(f"nowhere{i}")
        if i % 4 == 0:
            words[0] = words[0].capitalize()
        queries.append(" ".join(words))
    return scores, rows, queries
