"""GPU: hybrid retrieval end to end -- ContextRetriever with `hybrid` over a store of 2000 chunks and a tiny synthetic encoder: a
query for a made-up identifier that only one chunk carries gets that chunk through the lexical list, whatever the encoder makes of
it; with hybrid off the retriever answers as before; the re-rank and the device MMR step run on the fused lists; a store of two
shards gives the same lexical lists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = 2000
WORDS = ("retrieval generation quantization encoder attention relevance chunk model memory evidence passage index vector cosine "
         "kernel lexical dense fusion rank token").split()
IDENTS = [f"ZQX-{1000 + 37 * i}-{'ABCDEFGHIJ'[i]}" for i in range(10)]
IDENT_ROWS = [50 + 190 * i for i in range(10)]
OLD_KEYS = {"text", "score", "distance", "metadata", "chunk_id"}
NEW_KEYS = OLD_KEYS | {"dense_score", "bm25_score", "dense_rank", "lexical_rank"}


def _pipeline(name, retrieval=None, store_cfg=None):
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
    rng = np.random.default_rng(31)
    texts = [" ".join(rng.choice(WORDS, size=8)) + f" n{r}" for r in range(ROWS)]
    for ident, r in zip(IDENTS, IDENT_ROWS):
        texts[r] = texts[r] + f" serial {ident} noted"
    chunks = [Chunk(text=t, chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=None) for r, t in enumerate(texts)]
    emb = p.embedding_model.embed(texts)
    p.vector_store.create_index(chunks[:1200], emb[:1200])
    p.vector_store.create_index(chunks[1200:], emb[1200:])
    return p


@pytest.fixture(scope="module")
def hybrid(cuda):
    return _pipeline("hybrid-e2e", {"hybrid": True})


QUESTIONS = [f"find {ident}" for ident in IDENTS] + ["dense vector retrieval", "nothing-known-here at-all"]


def test_an_identifier_query_gets_its_chunk_through_the_lexical_list(cuda, hybrid):
    r = hybrid.retriever
    out = r.retrieve_batch(QUESTIONS)
    assert len(out) == len(QUESTIONS) and r.last_hybrid["lists"] == len(QUESTIONS)
    for row, chunks in zip(IDENT_ROWS, out[:10]):
        assert 1 <= len(chunks) <= 5 and all(set(c) == NEW_KEYS for c in chunks)
        hit = [c for c in chunks if c["chunk_id"] == f"c_{row}"]
        assert len(hit) == 1 and hit[0]["lexical_rank"] == 0 and hit[0]["bm25_score"] > 0.0
        assert [c["score"] for c in chunks] == sorted((c["score"] for c in chunks), reverse=True)
        assert all(0.0 < c["score"] <= 1.0 for c in chunks)
        for c in chunks:
            assert (c["dense_rank"] is None) == (c["distance"] is None) == (c["dense_score"] is None)
            assert (c["lexical_rank"] is None) == (c["bm25_score"] == 0.0)
            assert c["dense_rank"] is not None or c["lexical_rank"] is not None
    assert r.last_hybrid["lexical_only_hits"] >= 1
    assert all(c["lexical_rank"] is None for c in out[11])                    # no known word: the dense list alone
    assert [c["chunk_id"] for c in r.retrieve(QUESTIONS[0])] == [c["chunk_id"] for c in out[0]]     # retrieve() is retrieve_batch of one
    with pytest.raises(ValueError, match="filters"):
        r.retrieve(QUESTIONS[0], filters={"page": 1})


def test_with_hybrid_off_the_retriever_answers_as_before(cuda, hybrid):
    from rag.retrieval import ContextRetriever
    base = dict(hybrid.config["retrieval"])
    base["hybrid"] = False
    off = ContextRetriever(hybrid.vector_store, hybrid.embedding_model, base)
    calls = []
    inner = hybrid.vector_store.bm25_rows
    hybrid.vector_store.bm25_rows = lambda *a, **kw: (calls.append(1), inner(*a, **kw))[1]
    try:
        for q in QUESTIONS:
            got = off.retrieve_batch([q])
            assert got == [off.retrieve(q)] and all(set(c) == OLD_KEYS for c in got[0])
        absent = {k: v for k, v in base.items() if k != "hybrid"}
        plain = ContextRetriever(hybrid.vector_store, hybrid.embedding_model, absent)
        assert plain.retrieve_batch(QUESTIONS) == off.retrieve_batch(QUESTIONS)
        assert calls == [] and off.last_hybrid == {"lists": 0, "lexical_only_hits": 0}
    finally:
        del hybrid.vector_store.bm25_rows


def test_rerank_and_device_mmr_run_on_hybrid_lists(cuda, hybrid):
    from rag.retrieval import ContextRetriever
    cfg = dict(hybrid.config["retrieval"], rerank=True, diversity_penalty=0.2, mmr_vectors="device", lexical_rerank="device")
    r = ContextRetriever(hybrid.vector_store, hybrid.embedding_model, cfg)
    out = r.retrieve_batch(QUESTIONS)
    assert r.last_mmr["mode"] == "device" and r.last_rerank["mode"] == "host" and r.last_hybrid["lists"] == len(QUESTIONS)
    for row, chunks in zip(IDENT_ROWS, out[:10]):
        assert 2 <= len(chunks) <= 5 and all("rerank_score" in c for c in chunks)
        assert f"c_{row}" in [c["chunk_id"] for c in chunks]
        assert len({c["chunk_id"] for c in chunks}) == len(chunks)


def test_two_shards_give_the_same_lexical_lists(cuda, hybrid):
    two = _pipeline("hybrid-two", {"hybrid": True}, {"devices": ["cuda:0", "cuda:0"]})
    assert len(two.vector_store.collection.shards) == 2
    a_s, a_r = hybrid.vector_store.bm25_rows(QUESTIONS, 10)
    b_s, b_r = two.vector_store.bm25_rows(QUESTIONS, 10)
    assert (a_r == b_r).all() and (a_s.view(np.int32) == b_s.view(np.int32)).all()
    assert [int(a_r[i, 0]) for i in range(10)] == IDENT_ROWS
    out = two.retriever.retrieve_batch(QUESTIONS[:10])
    for row, chunks in zip(IDENT_ROWS, out):
        assert [c["lexical_rank"] for c in chunks if c["chunk_id"] == f"c_{row}"] == [0]
