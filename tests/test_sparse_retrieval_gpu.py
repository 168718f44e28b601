"""GPU: learned sparse retrieval end to end with synthetic:tiny-splade over a few hundred short texts -- SparseEncoder, the
store's sparse index (rag/indexing.py: _SparseIndex), VectorStore.sparse_rows and the retriever's `sparse_model` key."""
import numpy as np
import pytest

import _sparse_ref as ref

pytestmark = pytest.mark.gpu

ROWS = 300
DOC_TERMS, QUERY_TERMS = 256, 64


def _pipeline(name, retrieval=None, store_cfg=None, rows=ROWS):
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    cfg = {"embedding": {"model_name": "synthetic:tiny", "device": "cuda", "batch_size": 64, "normalize": True},
           "retrieval": dict({"top_k": 5, "similarity_threshold": 0.0, "rerank": False, "diversity_penalty": 0.0, "batch_queries": 64},
                             **(retrieval or {})),
           "vector_store": dict({"collection_name": name}, **(store_cfg or {}))}
    p = RAGPipeline(cfg)
    p.setup(Stub())
    texts = ref.corpus(rows)
    chunks = [Chunk(text=t, chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=None) for r, t in enumerate(texts)]
    p.vector_store.create_index(chunks, p.embedding_model.embed(texts))
    return p, texts, chunks


@pytest.fixture(scope="module")
def sparse(cuda):
    """The pipeline with hybrid + sparse_model, its texts and the index, built once."""
    p, texts, chunks = _pipeline("sparse-e2e", {"hybrid": True, "sparse_model": "synthetic:tiny-splade"})
    enc = p.retriever.sparse_encoder
    host_weights = dict(enc._weights)                  # the host copy: released once the model is on the device
    index = p.vector_store.sparse_index()
    return dict(p=p, texts=texts, chunks=chunks, enc=enc, index=index, host_weights=host_weights)


def _csr_host(index):
    return index.offsets.copy(), index.tokens[: index.n_terms].cpu().numpy(), index.weights[: index.n_terms].cpu().numpy()


def _query_block(enc, queries, cap=QUERY_TERMS):
    ids, w, counts = (t.cpu().numpy() for t in enc.encode_queries_device(queries, cap))
    assert ((ids >= 0).sum(1) == counts).all()
    return ref.csr_of([(i[i >= 0], x[i >= 0]) for i, x in zip(ids, w)])


def _compare_rows(rows, want, bound, skip_ids, cap):
    """rows: per text (ids, weights) as emitted; want fp64 [n, V]; bound [n, V] or [n, 1].  An id both sides hold agrees within
    the bound; an id on one side only must have a reference weight within the bound of 0 or of the cap-th weight.  Returns
    (emitted ids, ids on one side only, ids per text)."""
    want = want.copy()
    want[:, skip_ids] = 0.0
    bound = np.broadcast_to(bound, want.shape)
    emitted = one_sided = 0
    counts = []
    for j, (ids, got) in enumerate(rows):
        got = got.astype(np.float64)
        assert (np.diff(ids) > 0).all() and (got > 0).all() and not np.isin(ids, skip_ids).any() and len(ids) <= cap, j
        counts.append(len(ids))
        ref_ids = np.nonzero(want[j] > 0)[0]
        kth = np.sort(want[j][ref_ids])[-cap] if ref_ids.size > cap else 0.0
        if ref_ids.size > cap:
            ref_ids = ref_ids[want[j][ref_ids] >= kth]
        both = np.intersect1d(ids, ref_ids)
        err = np.abs(got[np.isin(ids, both)] - want[j][both])
        assert (err <= bound[j][both]).all(), (j, float((err / bound[j][both]).max()))
        for v in np.setxor1d(ids, ref_ids):
            assert min(abs(want[j][v]), abs(want[j][v] - kth)) <= bound[j][v], (j, int(v), want[j][v], bound[j][v])
            one_sided += 1
        emitted += len(ids)
    return emitted, one_sided, counts


def test_device_csr_matches_the_independent_fp64_model(cuda, sparse):
    """The whole of SparseEncoder -- tokenisation, which weights reach the encoder, the forward, the head's wiring, compaction,
    the scatter into input order, the index's packing -- against tests/_sparse_ref.model_reference: oracle/encoder_ref.py's BERT
    and the head in fp64 from the host weights and the token ids alone.  The bound per text is the reference's own
    (2 E_q + 4 a + 1 ulp, derived in model_reference's docstring; no device value enters it).  An id on one side only must have a
    reference weight within the bound of 0 or of the cap-th weight, and such ids are at most 1 % of all emitted ids
    (tests/test_sparse_cpu.py checks on the CPU that the reference alone leaves that margin)."""
    enc, index = sparse["enc"], sparse["index"]
    off, tok, w = _csr_host(index)
    assert index.n_rows == ROWS and off[-1] == index.n_terms
    want, _, bound = ref.model_reference(sparse["host_weights"], enc.shape, enc.tokenize(sparse["texts"]), with_bound=True)
    rows = [(tok[off[r]:off[r + 1]], w[off[r]:off[r + 1]]) for r in range(ROWS)]
    emitted, one_sided, counts = _compare_rows(rows, want, bound[:, None], enc.skip_ids, DOC_TERMS)
    print(f"{emitted} terms over {ROWS} rows (median {int(np.median(counts))}, max {max(counts)} a row); {one_sided} on one side only; "
          f"bound median {np.median(bound):.2e}, max {bound.max():.2e}")
    assert one_sided <= 0.01 * emitted and emitted > 10 * ROWS and np.median(counts) >= 3


def test_projection_matches_fp64_on_the_devices_own_transform_output(cuda, sparse):
    """The tight check beside the end-to-end one: one batch of 64 texts, the head's workspace read back by the test (it begins with
    t as fp16 [tokens_padded, H], include/crs_encoder.h), fp64 on those operands and the fp16 decoder, the bound of
    _sparse_ref.pool_bound.  The batch is walked as encode_device walks it: longest first, padded to 16 / 32 / 64."""
    import torch
    from rag.tokenizer import pad_batch
    enc = sparse["enc"]
    texts = sparse["texts"][:64]
    token_ids = enc.tokenize(texts)
    order = sorted(range(64), key=lambda i: (-len(token_ids[i]), i))
    block, lens = pad_batch([token_ids[i] for i in order], 0, short_steps=(16, 32, 64))
    width = int(block.shape[1])
    ids, w, counts = (t.cpu().numpy() for t in enc.encode_docs_device(texts, DOC_TERMS))
    H = enc.shape.hidden
    t16 = enc._mlm_ws[: 64 * width * H * 2].view(torch.float16).view(64, width, H).cpu().numpy()
    head = enc.head_tensors()
    w_d, bias = head["w_d"].cpu().numpy().astype(np.float64), head["bias"].cpu().numpy().astype(np.float64)
    want, absdot = ref.pool_ref(t16.astype(np.float64), lens, w_d, bias)
    for j in range(64):
        assert (t16[j, lens[j]:] == 0).all()
    bound = ref.pool_bound(absdot, want, H)
    rows = [(ids[i][: counts[i]], w[i][: counts[i]]) for i in order]
    emitted, one_sided, _ = _compare_rows(rows, want, bound, enc.skip_ids, DOC_TERMS)
    assert one_sided <= 0.01 * emitted and emitted > 640


def test_sparse_rows_equals_the_reference_on_the_devices_own_csr(cuda, sparse):
    store, enc = sparse["p"].vector_store, sparse["enc"]
    queries = ref.queries(70)                                                                  # two launches
    off, tok, w = _csr_host(sparse["index"])
    for k in (1, 10, 64):
        got = store.sparse_rows(queries, k)
        want = ref.sparse_topk_ref(off, tok, w, ROWS, *_query_block(enc, queries), k)
        assert (got[1] == want[1]).all() and (got[0].view(np.int32) == want[0].view(np.int32)).all(), k
    assert store.last_sparse == {"queries": 70, "query_terms": QUERY_TERMS, "launches": 2}
    assert (got[1][:, 0] >= 0).sum() >= 60
    lex = store.search_sparse_batch(queries[:2], top_k=10)
    assert lex["ids"][0] == [f"c_{r}" for r in want[1][0, :10] if r >= 0] and lex["scores"][0] == [float(s) for s in want[0][0, :len(lex["ids"][0])]]


def test_device_tokenisation_gives_the_same_vectors(cuda, sparse):
    from rag.sparse import SparseEncoder
    dev_enc = SparseEncoder({"model_name": "synthetic:tiny-splade", "tokenize": "device"})
    texts = sparse["texts"][:70]
    a = sparse["enc"].encode_docs_device(texts)
    b = dev_enc.encode_docs_device(texts)
    for x, y in zip(a, b):
        assert (x.cpu().numpy().view(np.int32) == y.cpu().numpy().view(np.int32)).all()


def test_append_extends_and_changes_drop_the_index(cuda):
    from rag.chunking import Chunk
    p, texts, chunks = _pipeline("sparse-life", {"hybrid": True, "sparse_model": "synthetic:tiny-splade"}, rows=120)
    store, enc = p.vector_store, p.retriever.sparse_encoder
    queries = ref.queries(6)

    def fresh(texts_now):
        from rag.indexing import VectorStore
        other = VectorStore({"collection_name": "sparse-fresh"})
        cs = [Chunk(text=t, chunk_id=f"f_{r}", start_char=0, end_char=1, page_number=None) for r, t in enumerate(texts_now)]
        other.create_index(cs, p.embedding_model.embed(texts_now))
        other.attach_sparse_encoder(enc)
        return other.sparse_rows(queries, 10)

    def same(a, b, what):
        assert (a[1] == b[1]).all() and (a[0].view(np.int32) == b[0].view(np.int32)).all(), what

    index = store.sparse_index()
    assert enc.texts_encoded == 120
    more = ref.corpus(40, seed=9)
    store.create_index([Chunk(text=t, chunk_id=f"m_{r}", start_char=0, end_char=1, page_number=None) for r, t in enumerate(more)],
                       p.embedding_model.embed(more))
    before = enc.texts_encoded
    got = store.sparse_rows(queries, 10)
    assert store.sparse_index() is index and index.n_rows == 160
    assert enc.texts_encoded - before == 40 + len(queries)                                     # the new rows and the queries, nothing else
    texts = texts + more
    before = enc.texts_encoded
    same(got, fresh(texts), "after append")
    # delete: rows renumbered, the index is dropped and rebuilt on the next search
    gone = sorted({int(got[1][0, 0]), 5, 130})
    ids = store.collection.ids
    assert store.delete(ids=[ids[r] for r in gone]) == len(gone) and "_sp" not in store.collection.__dict__
    texts = [t for r, t in enumerate(texts) if r not in gone]
    same(store.sparse_rows(queries, 10), fresh(texts), "after delete")
    assert store.sparse_index() is not index
    # update of a document
    store.update(ids=[store.collection.ids[40]], documents=["kernels scan rows merge lists fuse ranks"])
    assert "_sp" not in store.collection.__dict__
    texts[40] = "kernels scan rows merge lists fuse ranks"
    same(store.sparse_rows(queries, 10), fresh(texts), "after update")
    # upsert: one changed text, one new
    up = [Chunk(text="splade learns them", chunk_id=store.collection.ids[7], start_char=0, end_char=1, page_number=None),
          Chunk(text="bm25 counts words", chunk_id="brand-new", start_char=0, end_char=1, page_number=None)]
    store.upsert(up, p.embedding_model.embed([c.text for c in up]))
    assert "_sp" not in store.collection.__dict__
    texts[7] = "splade learns them"
    texts.append("bm25 counts words")
    assert store.collection.documents == texts
    same(store.sparse_rows(queries, 10), fresh(texts), "after upsert")


def test_the_index_is_guarded_and_lives_on_one_device(cuda, sparse):
    from rag.sparse import SparseEncoder
    enc = SparseEncoder("synthetic:tiny-splade")
    small, _, _ = _pipeline("sparse-small", store_cfg={"max_index_bytes": ROWS * DOC_TERMS * 8 - 1})
    with pytest.raises(ValueError, match="max_index_bytes"):
        small.vector_store.sparse_index(enc)
    assert enc.forwards == 0 and enc.texts_encoded == 0                                        # refused before any encoding
    two, _, _ = _pipeline("sparse-two", store_cfg={"devices": ["cuda:0", "cuda:0"]})
    with pytest.raises(NotImplementedError, match="one device"):
        two.vector_store.sparse_index(enc)
    with pytest.raises(NotImplementedError, match="one device"):
        two.vector_store.sparse_rows(["x"], 5)


def test_retrieve_batch_fuses_the_dense_and_the_sparse_lists(cuda, sparse):
    """By hand: search_rows for the dense lists (similarity_threshold 0 keeps every row), sparse_rows for the lexical ones, fuse_rrf
    on the two; retrieve_batch must return exactly those rows with those scores."""
    p = sparse["p"]
    store, r = p.vector_store, p.retriever
    queries = ref.queries(12, seed=4)
    out = r.retrieve_batch(queries)
    assert r.last_sparse == {"queries": 12, "query_terms": QUERY_TERMS, "launches": 1} and r.last_hybrid["lists"] == 12
    k = 5
    d_s, d_r = store.search_rows(p.embedding_model.embed(queries), k)
    l_s, l_r = store.sparse_rows(queries, k)
    rows, fused, dpos, lpos, count = store.fuse_rrf(d_r, l_r, k, c=60.0, weights=(1.0, 1.0))
    assert (l_r[:, 0] >= 0).sum() >= 10
    for i, chunks in enumerate(out):
        n = int(count[i])
        assert [c["chunk_id"] for c in chunks] == [f"c_{x}" for x in rows[i, :n]]
        assert [c["score"] for c in chunks] == [f / (2.0 / 61.0) for f in fused[i, :n].tolist()]
        assert [c["lexical_rank"] for c in chunks] == [int(x) if x >= 0 else None for x in lpos[i, :n]]
        assert [c["bm25_score"] for c in chunks] == [float(l_s[i, x]) if x >= 0 else 0.0 for x in lpos[i, :n]]
        assert [c["dense_rank"] for c in chunks] == [int(x) if x >= 0 else None for x in dpos[i, :n]]
    assert [c["chunk_id"] for c in r.retrieve(queries[0])] == [c["chunk_id"] for c in out[0]]


def test_without_sparse_model_the_lexical_list_is_bm25(cuda, sparse):
    from rag.retrieval import ContextRetriever
    p = sparse["p"]
    cfg = {k: v for k, v in p.config["retrieval"].items() if k != "sparse_model"}
    plain = ContextRetriever(p.vector_store, p.embedding_model, cfg)
    calls = []
    inner = p.vector_store.sparse_rows
    p.vector_store.sparse_rows = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]
    try:
        queries = ref.queries(8, seed=4)
        out = plain.retrieve_batch(queries)
        b_s, b_r = p.vector_store.bm25_rows(queries, 5)
        for i, chunks in enumerate(out):
            for c in chunks:
                if c["lexical_rank"] is not None:
                    assert c["chunk_id"] == f"c_{b_r[i, c['lexical_rank']]}" and c["bm25_score"] == float(b_s[i, c["lexical_rank"]])
        assert calls == [] and plain.sparse_encoder is None and plain.last_sparse == {"queries": 0, "query_terms": 0, "launches": 0}
        assert any(c["lexical_rank"] is not None for chunks in out for c in chunks)
    finally:
        del p.vector_store.sparse_rows
