"""GPU: late-interaction re-ranking end to end with ``synthetic:tiny-colbert`` on stores of at most 200 rows -- the store's token
index (offsets, token rows, incremental append, invalidation by delete / update / upsert, the size guard) and the retriever's
``late_interaction`` key (scores and order against the fp64 restatement of MaxSim over the SAME token vectors, within the bound of
tests/_maxsim_ref.py; retrieve against retrieve_batch; the hybrid and the filtered path; the key absent)."""
import numpy as np
import pytest

import _late_cases as lc
import _maxsim_ref as mr

pytestmark = pytest.mark.gpu

N_ROWS = 160
LI_CFG = {"model_name": "synthetic:tiny-colbert", "batch_size": 48, "query_maxlen": 16}


class _Stub:
    def generate(self, prompt, **kw):
        return "n/a"


def _chunks(texts, first=0, tag="c"):
    from rag.chunking import Chunk
    return [Chunk(text=t, chunk_id=f"{tag}_{first + r}", start_char=0, end_char=1, page_number=(first + r) % 3) for r, t in enumerate(texts)]


def _pipeline(name, texts, retrieval=None, store_cfg=None):
    from rag import RAGPipeline
    p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny", "device": "cuda", "batch_size": 256, "normalize": True},
                     "vector_store": dict({"collection_name": name}, **(store_cfg or {})),
                     "retrieval": dict({"top_k": 5, "rerank": True, "similarity_threshold": 0.0, "diversity_penalty": 0.0}, **(retrieval or {}))})
    p.setup(_Stub())
    if texts:
        chunks = _chunks(texts)
        p.vector_store.create_index(chunks, p.embedding_model.embed_chunks_device(chunks), metadata_fields=["page_number"])
    return p


def _bits(t):
    return t.detach().cpu().numpy().tobytes()


@pytest.fixture(scope="module")
def texts():
    return lc.corpus(N_ROWS)


@pytest.fixture(scope="module")
def late(cuda, texts):
    return _pipeline("li-on", texts, {"late_interaction": LI_CFG})


# ---- the token index -----------------------------------------------------------------------------------------------------------
def test_token_index_equals_the_encoders_output(cuda, late, texts):
    li = late.retriever.late_interaction
    store = late.vector_store
    index = store.token_index()
    counts = li.doc_token_counts(texts)
    assert index.n_rows == N_ROWS and index.offsets.dtype == np.int64
    assert np.array_equal(index.offsets, np.concatenate([[0], np.cumsum(counts)]))
    assert np.array_equal(index.offsets_dev.cpu().numpy(), index.offsets) and index.n_tokens == int(counts.sum())
    ids = li.tokenize_docs(texts)
    assert counts[1] == 2 and len(ids[2]) == li.doc_maxlen              # the empty text: [CLS] [SEP]; the long one: cut
    assert np.array_equal(counts, [int(li.keep_mask(t).sum()) for t in ids])
    assert (counts < np.asarray([len(t) for t in ids])).sum() > N_ROWS // 2             # punctuation was dropped in most documents
    tok, cnt = li.encode_docs_device(texts)                             # the same texts, the same batches
    assert np.array_equal(cnt.cpu().numpy(), counts)
    assert _bits(index.tok16[:index.n_tokens]) == _bits(tok)
    norms = index.tok16[:index.n_tokens].float().norm(dim=1).cpu().numpy()
    assert np.abs(norms - 1).max() < 2e-3                               # unit vectors
    assert store.token_index() is index                                 # nothing new: the same object, no encoding


def test_append_encodes_only_the_new_rows(cuda, texts):
    p = _pipeline("li-append", texts[:100], {"late_interaction": LI_CFG})
    li, store = p.retriever.late_interaction, p.vector_store
    index = store.token_index()
    assert li.docs_encoded == 100
    first_bits, first_tokens = _bits(index.tok16[:index.n_tokens]), index.n_tokens
    new = _chunks(texts[100:], first=100)
    store.create_index(new, p.embedding_model.embed_chunks_device(new), metadata_fields=["page_number"])
    again = store.token_index()
    assert again is index and index.n_rows == N_ROWS
    assert li.docs_encoded == N_ROWS                                    # 60 more documents went through the encoder, not 160
    assert _bits(index.tok16[:first_tokens]) == first_bits              # rows already held were not touched
    tail, _ = li.encode_docs_device(texts[100:])
    assert _bits(index.tok16[first_tokens:index.n_tokens]) == _bits(tail)
    assert np.array_equal(index.offsets, np.concatenate([[0], np.cumsum(li.doc_token_counts(texts))]))


def _scores(p, questions, rows):
    return p.retriever.late_interaction.score_rows(questions, rows, p.vector_store)


def test_delete_update_and_upsert_drop_the_index(cuda, texts):
    questions = lc.queries(6)
    docs = list(texts[:60])
    p = _pipeline("li-mutate", docs, {"late_interaction": LI_CFG})
    store, emb = p.vector_store, p.embedding_model
    rng = np.random.default_rng(3)

    def check(step):
        index = store.token_index()
        fresh = _pipeline("li-fresh-" + step, list(store.collection.documents), {"late_interaction": LI_CFG})
        f_index = fresh.vector_store.token_index()
        assert np.array_equal(index.offsets, f_index.offsets), step
        assert _bits(index.tok16[:index.n_tokens]) == _bits(f_index.tok16[:f_index.n_tokens]), step
        rows = np.stack([rng.permutation(index.n_rows)[:10] for _ in questions]).astype(np.int64)
        assert _bits(_scores(p, questions, rows)) == _bits(_scores(fresh, questions, rows)), step
        return index

    first = check("built")
    assert store.delete(ids=["c_3", "c_17"]) == 2
    after_delete = check("delete")
    assert after_delete is not first and after_delete.n_rows == 58
    store.update(ids=["c_5"], metadatas=[{"page_number": 9}])           # no document changed: the index stays
    assert store.token_index() is after_delete
    store.update(ids=["c_5"], documents=["a brand new document , with punctuation !"])
    after_update = check("update")
    assert after_update is not after_delete
    ups = _chunks(["an upserted text for a known id", "and one for a new id"], first=0, tag="c")
    ups[1].chunk_id = "c_new"
    store.upsert(ups, emb.embed_chunks_device(ups), metadata_fields=["page_number"])
    after_upsert = check("upsert")
    assert after_upsert is not after_update and after_upsert.n_rows == 59
    assert store.collection.documents[0] == "an upserted text for a known id"


def test_size_guard_refuses_before_encoding(cuda, texts):
    p = _pipeline("li-guard", texts[:40], {"late_interaction": LI_CFG}, {"max_index_bytes": 4096})
    li = p.retriever.late_interaction
    need = int(li.doc_token_counts(texts[:40]).sum()) * li.dimp * 2
    with pytest.raises(ValueError, match=str(need)):
        p.vector_store.token_index()
    assert li.docs_encoded == 0
    p.vector_store.max_index_bytes = need
    assert p.vector_store.token_index().n_tokens * li.dimp * 2 == need


# ---- the retriever -------------------------------------------------------------------------------------------------------------
def _restated(p, questions, lists):
    """fp64 MaxSim of every returned chunk over the index's own token vectors and the queries as this batch encodes them."""
    li, store = p.retriever.late_interaction, p.vector_store
    index = store.token_index()
    q16, q_len = li.encode_queries_device(questions)
    m = max(1, max(len(c) for c in lists))
    rows = np.full((len(lists), m), -1, dtype=np.int64)
    row_of = {cid: r for r, cid in enumerate(store.collection.ids)}
    for i, chunks in enumerate(lists):
        rows[i, :len(chunks)] = [row_of[c["chunk_id"]] for c in chunks]
    return mr.maxsim_ref(q16.cpu().numpy(), q_len.cpu().numpy(), index.tok16[:index.n_tokens].cpu().numpy(), index.offsets, rows), rows


def test_retrieve_batch_scores_and_order_match_fp64(cuda, late):
    r = late.retriever
    k = r.top_k
    questions = lc.queries(40)
    lists = late.retrieve_batch(questions)
    assert r.last_rerank == {"mode": "late-interaction", "lists": 40}
    # every candidate of every list (the 2 k survivors of the search), restated
    cand = []
    for q in questions:
        hits = r.vector_store.search(query_embedding=r.embedding_model.embed(q), top_k=2 * k)
        cand.append(r._hits_to_chunks(hits["ids"][0], hits["documents"][0], hits["metadatas"][0], hits["distances"][0]))
    (want, bound), _ = _restated(late, questions, cand)
    worst = 0.0
    for i, (chunks, pool) in enumerate(zip(lists, cand)):
        assert len(pool) == 2 * k and len(chunks) == k
        pos = {c["chunk_id"]: j for j, c in enumerate(pool)}
        rr = [c["rerank_score"] for c in chunks]
        assert rr == sorted(rr, reverse=True)
        for a, b in zip(chunks, chunks[1:]):                              # stable: ties keep the search order
            assert a["rerank_score"] > b["rerank_score"] or pos[a["chunk_id"]] < pos[b["chunk_id"]]
        for c in chunks:
            j = pos[c["chunk_id"]]
            assert abs(c["rerank_score"] - want[i, j]) <= bound[i, j]
            worst = max(worst, abs(c["rerank_score"] - want[i, j]) / bound[i, j])
        kept = {pos[c["chunk_id"]] for c in chunks}
        for x in kept:                                                   # nobody left out beats somebody kept by more than the bounds
            for y in set(range(2 * k)) - kept:
                assert want[i, y] - want[i, x] <= bound[i, x] + bound[i, y]
        order64 = [j for j in np.argsort(-want[i], kind="stable")]
        clear = all(want[i, a] - want[i, b] > 2 * max(bound[i, a], bound[i, b]) for a, b in zip(order64[:k], order64[1:k + 1]))
        if clear:
            assert [pos[c["chunk_id"]] for c in chunks] == order64[:k]
    print(f"late-interaction retrieve_batch: largest |rerank_score error| / bound {worst:.3e}")


def test_retrieve_equals_retrieve_batch_of_one(cuda, late):
    for q in lc.queries(5, seed=9):
        one, batch = late.retrieve(q), late.retrieve_batch([q])[0]
        assert [(c["chunk_id"], c["rerank_score"], c["score"]) for c in one] == [(c["chunk_id"], c["rerank_score"], c["score"]) for c in batch]
        assert late.retriever.last_rerank == {"mode": "late-interaction", "lists": 1}
        assert len(one) == late.retriever.top_k


def test_filters_and_hybrid_go_through_the_same_scoring(cuda, late, texts):
    r = late.retriever
    questions = lc.queries(8, seed=5)
    for q in questions[:4]:                                              # the filtered path of retrieve()
        chunks = r.retrieve(q, filters={"page_number": 1})
        assert r.last_rerank == {"mode": "late-interaction", "lists": 1}
        assert chunks and all(c["metadata"]["page_number"] == 1 for c in chunks)
        (want, bound), _ = _restated(late, [q], [chunks])
        rr = np.asarray([c["rerank_score"] for c in chunks])
        assert (np.abs(rr - want[0, :len(chunks)]) <= bound[0, :len(chunks)]).all() and list(rr) == sorted(rr, reverse=True)
    hybrid = _pipeline("li-hybrid", texts, {"late_interaction": LI_CFG, "hybrid": True})
    lists = hybrid.retrieve_batch(questions)
    assert hybrid.retriever.last_rerank == {"mode": "late-interaction", "lists": 8} and hybrid.retriever.last_hybrid["lists"] == 8
    (want, bound), _ = _restated(hybrid, questions, lists)
    for i, chunks in enumerate(lists):
        assert 0 < len(chunks) <= hybrid.retriever.top_k and all("bm25_score" in c for c in chunks)
        rr = np.asarray([c["rerank_score"] for c in chunks])
        assert (np.abs(rr - want[i, :len(chunks)]) <= bound[i, :len(chunks)]).all() and list(rr) == sorted(rr, reverse=True)


def test_without_the_key_nothing_changes(cuda, texts):
    plain = _pipeline("li-off", texts, {})
    r = plain.retriever
    assert r.late_interaction is None and plain.vector_store._token_encoder is None
    questions = lc.queries(12, seed=7)
    lists = plain.retrieve_batch(questions)
    assert r.last_rerank == {"mode": "host", "lists": 12}
    assert "_li" not in plain.vector_store.collection.__dict__          # no token index was built
    for q, chunks in zip(questions, lists):
        assert [(c["chunk_id"], c.get("rerank_score")) for c in chunks] == [(c["chunk_id"], c.get("rerank_score")) for c in plain.retrieve(q)]
        assert any("rerank_score" in c for c in chunks)
        for c in (c for c in chunks if "rerank_score" in c):             # the token-overlap rule, as before
            hits_q = len(set(q.lower().split()) & set(c["text"].lower().split())) / max(len(set(q.lower().split())), 1)
            assert c["rerank_score"] == c["score"] * 0.7 + hits_q * 0.3
    with pytest.raises(ValueError, match="attach_token_encoder"):
        plain.vector_store.token_index()
