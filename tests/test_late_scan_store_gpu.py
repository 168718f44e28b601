"""GPU: the late-interaction sweep end to end with ``synthetic:tiny-colbert`` -- VectorStore.search_late_batch against the host
top-k of score_rows over every row (same ids, same score bits) through create_index, an append and a delete, and the retriever's
``late_interaction.first_stage``."""
import numpy as np
import pytest

import _late_cases as lc
from test_late_interaction_gpu import LI_CFG, _chunks, _pipeline

pytestmark = pytest.mark.gpu

SCAN_CFG = dict(LI_CFG, first_stage="scan")


@pytest.fixture(scope="module")
def texts():
    return lc.corpus(150)


def _check_store(p, questions, k):
    store, li = p.vector_store, p.retriever.late_interaction
    n = store.collection.count()
    full = li.score_rows(questions, np.tile(np.arange(n, dtype=np.int64), (len(questions), 1)), store).cpu().numpy()
    got = store.search_late_batch(questions, top_k=k)
    for a in range(len(questions)):
        order = sorted(range(n), key=lambda r: (-full[a, r], r))[:k]
        assert got["rows"][a] == order and got["ids"][a] == [store.collection.ids[r] for r in order]
        assert got["documents"][a] == [store.collection.documents[r] for r in order]
        assert np.asarray(got["scores"][a], np.float32).tobytes() == full[a, order].tobytes()


def test_search_late_batch_is_the_top_k_of_score_rows(cuda, texts):
    questions = lc.queries(9)
    p = _pipeline("ls-store", texts[:100], {"late_interaction": SCAN_CFG})
    store = p.vector_store
    _check_store(p, questions, 10)
    new = _chunks(texts[100:], first=100)
    store.create_index(new, p.embedding_model.embed_chunks_device(new), metadata_fields=["page_number"])
    _check_store(p, questions, 64)
    assert store.delete(ids=["c_3", "c_117"]) == 2
    _check_store(p, questions, 7)
    with pytest.raises(NotImplementedError, match="top_k"):
        store.search_late_batch(questions, top_k=65)


def test_scan_and_dense_agree_when_the_candidates_are_every_row(cuda, texts):
    questions = lc.queries(7)
    docs = [t or "an empty chunk" for t in texts[:40]]
    lists = {}
    for stage in ("dense", "scan"):
        p = _pipeline("ls-" + stage, docs, {"late_interaction": dict(LI_CFG, first_stage=stage), "top_k": 20})
        p.retriever.similarity_threshold = -1.0          # the dense score is in [0, 1], the sweep's mean maximum in [-1, 1]: keep all
        lists[stage] = p.retriever.retrieve_batch(questions)
        assert lists[stage][0] == p.retriever.retrieve(questions[0])
    for d, s in zip(lists["dense"], lists["scan"]):
        assert len(s) == 20 and [c["chunk_id"] for c in d] == [c["chunk_id"] for c in s]
        assert [c["rerank_score"] for c in d] == [c["rerank_score"] for c in s]
        assert all(-1.0 <= c["score"] <= 1.0 and c["distance"] == 1.0 - c["score"] for c in s)


def test_filters_take_the_dense_path_and_bad_values_are_refused(cuda, texts, monkeypatch):
    p = _pipeline("ls-filter", texts[:40], {"late_interaction": SCAN_CFG})

    def boom(*a, **k):
        raise AssertionError("the sweep must not run under filters")
    monkeypatch.setattr(p.vector_store, "late_rows", boom)
    hits = p.retriever.retrieve(lc.queries(1)[0], filters={"page_number": 1})
    assert hits and all(c["metadata"]["page_number"] == 1 for c in hits)
    with pytest.raises(ValueError, match="first_stage"):
        _pipeline("ls-bad", [], {"late_interaction": dict(LI_CFG, first_stage="nope")})
