"""GPU: the BM25 scan (csrc/bm25.hip, crs::bm25_topk) and VectorStore.bm25_rows against tests/_bm25_ref.py.

The kernel's fp32 arithmetic rounds every operation on its own and adds a row's terms in ascending token id, so it is a pure
function of its inputs and there is no tolerance: scores are compared as int32 words and rows with ==.  Beside that, on the
1000-row corpus, the row sets equal an independent fp64 textbook BM25's top-k for every query whose k-th and (k+1)-th fp64 scores
are further apart than the fp32 rounding bound (tests/test_bm25_cpu.py checks that at most 2 % of the queries are dropped)."""
import numpy as np
import pytest

import _bm25_ref as ref

pytestmark = pytest.mark.gpu


def _csr(docs):
    from rag.indexing import _TokenCSR
    csr = _TokenCSR()
    csr.extend(docs)
    return csr


_CACHE = {}


def _case(n_rows):
    """(documents, token CSR, the 64 seeded queries' blocks, constants) of a corpus size: built once per module run."""
    if n_rows not in _CACHE:
        docs = ref.corpus(n_rows)
        csr = _csr(docs)
        queries = ref.queries(64)
        ids = [csr.query_ids(q)[0] for q in queries]
        weights = [[ref.weight(csr.rows, int(csr.df[t])) for t in ts] for ts in ids]
        _CACHE[n_rows] = dict(docs=docs, csr=csr, queries=queries, ids=ids, weights=weights, const=ref.constants(csr.rows, csr.total_len),
                              want={})
    return _CACHE[n_rows]


def _block(case, nq):
    ids, weights = case["ids"][:nq], case["weights"][:nq]
    q_off = np.r_[0, np.cumsum([len(t) for t in ids])].astype(np.int64)
    q_tok = np.array([t for ts in ids for t in ts], dtype=np.int32)
    q_w = np.array([w for ws in weights for w in ws], dtype=np.float32)
    return q_off, q_tok, q_w


def _want(case, k):
    """The reference lists of all 64 queries at k (a prefix of them serves every nq): every row scored once per corpus, the
    selection once per (corpus, k)."""
    csr = case["csr"]
    if "scored" not in case:
        q_off, q_tok, q_w = _block(case, 64)
        case["scored"] = [ref.bm25_scores_ref(csr.offsets, csr.token_ids, csr.tfs, csr.doc_len, csr.rows, q_tok[q_off[q]:q_off[q + 1]],
                                              q_w[q_off[q]:q_off[q + 1]], *case["const"]) for q in range(64)]
    if k not in case["want"]:
        lists = [ref.topk_of(s, h, k) for s, h in case["scored"]]
        case["want"][k] = np.stack([s for s, _ in lists]), np.stack([r for _, r in lists])
    return case["want"][k]


def _run_op(cuda, case, nq, k):
    import torch
    from rag import _native as nat
    csr = case["csr"]
    q_off, q_tok, q_w = _block(case, nq)
    c0, c1, k1p1 = case["const"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)          # noqa: E731
    ws = torch.empty(nat.bm25_workspace_bytes(nq, k, csr.rows), dtype=torch.uint8, device=cuda)
    out_s = torch.empty((nq, k), dtype=torch.float32, device=cuda)
    out_r = torch.empty((nq, k), dtype=torch.int64, device=cuda)
    torch.ops.crs.bm25_topk(dev(csr.offsets), dev(csr.token_ids), dev(csr.tfs), dev(csr.doc_len), csr.rows, dev(q_off), dev(q_tok), dev(q_w),
                            float(c0), float(c1), float(k1p1), k, ws, out_s, out_r)
    torch.cuda.synchronize()
    return out_s.cpu().numpy(), out_r.cpu().numpy()


def _assert_bits(got, want, what):
    (got_s, got_r), (want_s, want_r) = got, want
    assert got_s.dtype == np.float32 and got_r.dtype == np.int64 and got_s.shape == want_s.shape and got_r.shape == want_r.shape, what
    bad = np.argwhere(got_r != want_r)
    assert bad.size == 0, f"{what}: rows differ first at {bad[0].tolist()}: {got_r[tuple(bad[0])]} != {want_r[tuple(bad[0])]}"
    bad = np.argwhere(got_s.view(np.int32) != want_s.view(np.int32))
    assert bad.size == 0, f"{what}: scores differ in their bits first at {bad[0].tolist()}: {got_s[tuple(bad[0])]!r} != {want_s[tuple(bad[0])]!r}"


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 1000, 20000])
def test_op_matches_the_fp32_reference_bit_for_bit(cuda, n_rows):
    """Every corpus size x nq in {1, 3, 64} x k in {1, 10, 64}: ragged last tiles, fewer rows than a tile, several workgroups with
    several tiles each (20 000 rows), 5 % empty documents, a row longer than the staging chunk, twenty exact duplicates, the
    stopword in every document and (almost) every query, a query with no known word, one with fewer hits than k, one of 200 words."""
    case = _case(n_rows)
    csr = case["csr"]
    if n_rows >= 1000:
        assert (np.diff(csr.offsets) > ref.CHUNK_TOKENS).sum() == 1 and (np.diff(csr.offsets) == 0).sum() >= n_rows // 40
        assert len(case["ids"][3]) == 200 and case["ids"][1] == [] and csr.tfs.max() > 1
    for nq, k in ((1, 1), (1, 10), (3, 10), (3, 64), (64, 1), (64, 10), (64, 64)):
        want_s, want_r = _want(case, k)
        _assert_bits(_run_op(cuda, case, nq, k), (want_s[:nq], want_r[:nq]), f"n_rows={n_rows} nq={nq} k={k}")
    want_s, want_r = _want(case, 64)
    assert (want_r[1] == -1).all() and np.isneginf(want_s[1]).all()                       # no known word: an empty list
    if n_rows >= 1000:
        assert (want_r[2] >= 0).sum() == 20 and (np.diff(want_r[2][:20]) > 0).all()       # 20 hits < k; the duplicates tie: row order
        assert len(set(want_s[2][:20].tolist())) == 1
        dup = set(want_r[2][:20].tolist())
        assert set(want_r[4][:20].tolist()) == dup and (np.diff(want_r[4][:20]) > 0).all()


def _store(docs, cfg=None):
    """A VectorStore over `docs` with random embeddings (the lexical path never reads them)."""
    import torch
    from rag.chunking import Chunk
    from rag.indexing import VectorStore
    store = VectorStore(dict({"collection_name": "bm25"}, **(cfg or {})))
    chunks = [Chunk(text=d, chunk_id=f"c{r}", start_char=0, end_char=1, page_number=None) for r, d in enumerate(docs)]
    g = torch.Generator().manual_seed(5)
    store.create_index(chunks, torch.randn((len(docs), 64), generator=g).numpy())
    return store


def test_store_matches_the_reference_for_65_queries_and_the_textbook_row_sets(cuda):
    case = _case(1000)
    csr = case["csr"]
    store = _store(case["docs"])
    queries = case["queries"] + ["THE w3 w11 w29"]                                          # 65: two launches
    got = store.bm25_rows(queries, 10)
    ids = csr.query_ids(queries[64])[0]
    q_w = np.array([ref.weight(csr.rows, int(csr.df[t])) for t in ids], dtype=np.float32)
    last = ref.bm25_topk_ref(csr.offsets, csr.token_ids, csr.tfs, csr.doc_len, csr.rows, np.array([0, len(ids)]), np.array(ids, dtype=np.int32),
                             q_w, *case["const"], 10)
    want_s, want_r = _want(case, 10)
    _assert_bits(got, (np.vstack([want_s, last[0]]), np.vstack([want_r, last[1]])), "bm25_rows, 65 queries")
    lex = store.search_lexical_batch(queries[:2], top_k=10)
    assert lex["ids"][0] == [f"c{r}" for r in want_r[0]] and lex["ids"][1] == [] and lex["scores"][0] == want_s[0].astype(np.float64).tolist()
    # row sets against the fp64 textbook, on the plain queries (100: two launches), ambiguous ones dropped (<= 2 %)
    book = ref.Textbook(case["docs"])
    plain = ref.plain_queries(100)
    for k in (1, 10):
        _, rows = store.bm25_rows(plain, k)
        dropped = 0
        for q, query in enumerate(plain):
            want = book.scores(query)
            ranked = sorted(want.items(), key=lambda rs: (-rs[1][0], rs[0]))
            if len(ranked) > k:
                (a, ma), (b, mb) = ranked[k - 1][1], ranked[k][1]
                if a - b <= (ma + 6) * ref.EPS32 * a + (mb + 6) * ref.EPS32 * b:
                    dropped += 1
                    continue
            assert set(rows[q].tolist()) - {-1} == {r for r, _ in ranked[:k]}, (k, q, query)
        assert dropped <= 0.02 * len(plain), (k, dropped)


def test_store_follows_delete_and_update(cuda):
    docs = ref.corpus(300, seed=8)
    store = _store(docs)
    queries = ref.queries(8)

    def check(docs_now, what):
        csr = _csr(docs_now)
        ids = [csr.query_ids(q)[0] for q in queries]
        q_off = np.r_[0, np.cumsum([len(t) for t in ids])].astype(np.int64)
        q_tok = np.array([t for ts in ids for t in ts], dtype=np.int32)
        q_w = np.array([ref.weight(csr.rows, int(csr.df[t])) for t in q_tok.tolist()], dtype=np.float32)
        want = ref.bm25_topk_ref(csr.offsets, csr.token_ids, csr.tfs, csr.doc_len, csr.rows, q_off, q_tok, q_w,
                                 *ref.constants(csr.rows, csr.total_len), 10)
        _assert_bits(store.bm25_rows(queries, 10), want, what)
        return want

    first = check(docs, "fresh store")
    gone = sorted({int(first[1][0, 0]), int(first[1][0, 3]), 7})
    assert store.delete(ids=[f"c{r}" for r in gone]) == len(gone)                           # rows renumbered, N / df / avgdl change
    docs = [d for r, d in enumerate(docs) if r not in gone]
    after = check(docs, "after delete")
    assert not (after[1] == first[1]).all()
    target = store.collection.ids[40]
    store.update(ids=[target], documents=["rareword rareword zzz-unknown w5 the the the"])
    docs[40] = "rareword rareword zzz-unknown w5 the the the"
    last = check(docs, "after update")
    assert 40 in last[1][1].tolist() and 40 in last[1][2].tolist()                         # 'zzz-unknown' is a known word now


def test_sharded_store_gives_the_same_lexical_lists(cuda):
    docs = ref.corpus(500, seed=6)
    queries = ref.queries(16)
    one = _store(docs).bm25_rows(queries, 10)
    two_store = _store(docs, {"devices": ["cuda:0", "cuda:0"]})
    assert len(two_store.collection.shards) == 2
    _assert_bits(two_store.bm25_rows(queries, 10), one, "two shards on one card")
