"""GPU: an fp8 token index end to end with ``synthetic:tiny-colbert`` (``token_dtype: 'fp8'``) -- the store's index is
uint8 rows of dimp bytes, search_late_batch is the brute-force ranking by crs_maxsim_f8, and both first stages of the retriever
return the kernel's sum as rerank_score."""
import numpy as np
import pytest

import _late_cases as lc
from test_late_interaction_gpu import LI_CFG, _chunks, _pipeline

pytestmark = pytest.mark.gpu

F8_CFG = dict(LI_CFG, token_dtype="fp8")


@pytest.fixture(scope="module")
def texts():
    return lc.corpus(150)


def _check_store(p, questions, k):
    """search_late_batch against crs_maxsim_f8 over every row: same rows, same score bits; the index holds one byte a coordinate."""
    import torch
    store, li = p.vector_store, p.retriever.late_interaction
    n = store.collection.count()
    index = store.token_index()
    assert index.tok16.dtype == torch.uint8 and index.n_rows == n
    assert index.n_tokens * index.dimp * index.elem_bytes == int(li.doc_token_counts(store.collection.documents).sum()) * li.dimp
    full = li.score_rows(questions, np.tile(np.arange(n, dtype=np.int64), (len(questions), 1)), store).cpu().numpy()
    got = store.search_late_batch(questions, top_k=k)
    for a in range(len(questions)):
        order = sorted(range(n), key=lambda r: (-full[a, r], r))[:k]
        assert got["rows"][a] == order
        assert np.asarray(got["scores"][a], np.float32).tobytes() == full[a, order].tobytes()
    return index


def test_fp8_store_append_delete_and_size_guard(cuda, texts):
    questions = lc.queries(9)
    p = _pipeline("f8-store", texts[:100], {"late_interaction": dict(F8_CFG, first_stage="scan")})
    store, li = p.vector_store, p.retriever.late_interaction
    index = _check_store(p, questions, 10)
    new = _chunks(texts[100:], first=100)
    store.create_index(new, p.embedding_model.embed_chunks_device(new), metadata_fields=["page_number"])
    assert _check_store(p, questions, 32) is index and li.docs_encoded == 150          # extended in place: 50 more documents encoded
    assert store.delete(ids=["c_3", "c_117"]) == 2
    assert _check_store(p, questions, 7) is not index                                   # dropped and rebuilt
    store.max_index_bytes = index.n_tokens * li.dimp                                    # what fp8 needs; fp16 needs twice that
    from rag.late_interaction import LateInteractionReranker
    with pytest.raises(ValueError, match="max_index_bytes"):
        store.token_index(LateInteractionReranker(LI_CFG))                              # the other dtype: the index is forgotten
    assert store.token_index(li) is not index and store.token_index().tok16.dtype == index.tok16.dtype


@pytest.mark.parametrize("stage", ["dense", "scan"])
def test_rerank_score_is_the_kernels_sum(cuda, texts, stage):
    questions = lc.queries(5)
    docs = [t or "an empty chunk" for t in texts[:40]]
    p = _pipeline("f8-" + stage, docs, {"late_interaction": dict(F8_CFG, first_stage=stage), "top_k": 20})
    p.retriever.similarity_threshold = -1.0
    li, store = p.retriever.late_interaction, p.vector_store
    full = li.score_rows(questions, np.tile(np.arange(40, dtype=np.int64), (5, 1)), store).cpu().numpy()
    for a, chunks in enumerate(p.retriever.retrieve_batch(questions)):
        assert len(chunks) == 20
        rows = [int(c["chunk_id"].split("_")[1]) for c in chunks]
        assert rows == sorted(range(40), key=lambda r: (-full[a, r], r))[:20]
        assert [np.float32(c["rerank_score"]) for c in chunks] == [full[a, r] for r in rows]
