"""index_dtype 'mxfp4' through VectorStore and ContextRetriever: the fp32 re-rank of the block-scaled sweep's k' candidates
against the fp32 oracle and a numpy emulation of quantise / slab top-k' / re-rank, the exactness tally, the stats, the refusals."""
from __future__ import annotations

import numpy as np
import pytest

from _mxfp4_ref import dequant_fp4, quant_dequant_e4m3, quant_fp4, unit_rows

pytestmark = pytest.mark.gpu
DIM = 384


def make_store(n, seed=0, **cfg):
    from rag.chunking import Chunk
    from rag.indexing import VectorStore
    store = VectorStore(dict({"index_dtype": "mxfp4", "collection_name": f"mx{n}"}, **cfg))
    x = np.random.default_rng(seed).standard_normal((n, DIM)).astype(np.float32)
    chunks = [Chunk(text=f"text {i}", chunk_id=f"c_{i}", start_char=0, end_char=1) for i in range(n)]
    cut = n // 3                                       # two appends, the second starting mid-tile
    store.create_index(chunks[:cut], x[:cut])
    store.create_index(chunks[cut:], x[cut:])
    return store, x


def queries(x, nq, seed=1):
    rng = np.random.default_rng(seed)
    return unit_rows(rng.standard_normal((nq, DIM)) + 0.5 * x[rng.integers(0, len(x), nq)])


def ranked(scores, k):
    order = np.lexsort((np.broadcast_to(np.arange(scores.shape[1]), scores.shape), -scores), axis=1)[:, :k]
    return order, np.take_along_axis(scores, order, axis=1)


def same_ids_up_to_ties(got, want, want_scores, tol):
    gap = np.diff(want_scores, axis=1)
    near = np.zeros(want.shape, bool)
    near[:, 1:] |= -gap < tol
    near[:, :-1] |= -gap < tol
    differ = got != want
    assert not (differ & ~near).any() and differ.mean() <= 0.01


def test_fewer_rows_than_candidates_is_the_fp32_oracle(cuda):
    store, x = make_store(50)
    q = queries(x, 17)
    shadow = store.collection.shadow[:50].cpu().numpy()
    assert np.array_equal(shadow.view(np.uint32), unit_rows(x).view(np.uint32))
    s, r = store.search_rows(q, 10)                    # k' = 64 >= 50 rows: every row is re-ranked
    want_r, want_s = ranked(q.astype(np.float64) @ shadow.astype(np.float64).T, 10)
    assert np.array_equal(r, want_r) and np.abs(s - want_s).max() <= DIM * 2.0 ** -24
    assert store.last_exactness == {"queries": 17, "certified": 0, "escalated": 0, "unproven": 17, "mode": "mxfp4"}
    stats = store.get_stats()
    assert stats["index_dtype"] == "mxfp4" and stats["bytes_per_row"] == 208 and stats["slab_bytes"] == 50 * 208 and stats["row_err_max"] > 0


@pytest.mark.parametrize("refine", [True, False])
def test_search_batch_is_quantise_slab_topk_rerank(cuda, refine):
    n, k, over = 4099, 10, 4                           # k' = 64
    store, x = make_store(n, mxfp4_overfetch=over, refine_fp32=refine)
    import torch
    q = queries(x, 64)
    v = unit_rows(x)
    # the store normalises its queries once more on the device: the emulation starts from those bits
    qn = torch.nn.functional.normalize(torch.from_numpy(q).to(cuda), p=2, dim=1, eps=1e-12).cpu().numpy()
    slab = quant_dequant_e4m3(qn, DIM) @ dequant_fp4(*quant_fp4(v)).T
    cand, cand_s = ranked(slab, 64)
    if refine:                                         # fp32 re-rank of the 64 candidates
        exact = np.take_along_axis(qn.astype(np.float64) @ v.astype(np.float64).T, cand, axis=1)
        pos, want_s = ranked(exact, k)
        want = np.take_along_axis(cand, pos, axis=1)
    else:
        want, want_s = cand[:, :k], cand_s[:, :k]
    out = store.search_batch(q, top_k=k)
    got = np.array([[int(c[2:]) for c in ids] for ids in out["ids"]])
    same_ids_up_to_ties(got, want, want_s, 2 * DIM * 2.0 ** -24)
    dist = np.array(out["distances"])
    assert (np.diff(dist, axis=1) >= 0).all()
    if refine:                                         # the true fp32 cosines of the rows returned
        cos = np.take_along_axis(qn.astype(np.float64) @ v.astype(np.float64).T, got, axis=1)
        assert np.abs((1.0 - dist) - cos).max() <= 2 * DIM * 2.0 ** -24
        assert store.last_exactness["unproven"] == 64 and store.last_exactness["certified"] == 0
    else:
        assert store.last_exactness["mode"] == "slab"
    assert store.search(q[0], top_k=k)["ids"][0] == out["ids"][0]


def test_retrieve_batch_counts_nothing_certified(cuda):
    from rag.retrieval import ContextRetriever
    store, x = make_store(4099)
    q = queries(x, 8)

    class Model:                                       # duck-typed: the query texts are indices into q
        def embed(self, texts, show_progress=False):
            return q[[int(t) for t in ([texts] if isinstance(texts, str) else texts)]]

    r = ContextRetriever(store, Model(), {"top_k": 10, "rerank": True, "similarity_threshold": 0.0})
    out = r.retrieve_batch([str(i) for i in range(8)])
    assert len(out) == 8 and all(0 < len(chunks) <= 10 for chunks in out)
    assert store.last_exactness["certified"] == 0 and store.last_exactness["escalated"] == 0 and store.last_exactness["unproven"] == 8
    assert [c["chunk_id"] for c in r.retrieve("0")] == [c["chunk_id"] for c in out[0]]


@pytest.mark.parametrize("cfg, option", [
    ({"sharded": True}, "sharded"), ({"num_gpus": 2}, "num_gpus"), ({"devices": ["cuda:0", "cuda:0"]}, "devices"),
    ({"space": "ip"}, "space"), ({"space": "l2"}, "space"), ({"persist_directory": "/nonexistent/mx"}, "persist_directory"),
    ({"dedup_threshold": 0.9}, "dedup_threshold"),
])
def test_unsupported_configurations_are_named(cuda, cfg, option):
    from rag.indexing import VectorStore
    with pytest.raises(NotImplementedError, match=option):
        VectorStore(dict({"index_dtype": "mxfp4"}, **cfg))


@pytest.mark.parametrize("call, option", [
    (lambda s, q: s.delete(ids=["c_0"]), "delete"),
    (lambda s, q: s.update(["c_0"], embeddings=q[:1]), "update"),
    (lambda s, q: s.upsert([], q[:0]), "upsert"),
    (lambda s, q: s.search_batch(q, top_k=5, where={"section": "a"}), "where"),
    (lambda s, q: s.search_batch(q, top_k=5, where_document={"$contains": "a"}), "where"),
    (lambda s, q: s.search_batch(q, top_k=65), "top_k"),
    (lambda s, q: s.collection.shards[0].view(), "fused chunks"),
    (lambda s, q: s.persist(), "persist"),
    (lambda s, q: s.near_duplicates(0.9), "near-duplicate"),
    (lambda s, q: s.deduplicate(0.9), "near-duplicate"),
    (lambda s, q: s.token_index(), "token index"),
    (lambda s, q: s.sparse_index(), "sparse index"),
    (lambda s, q: s.bm25_rows(["a"], 5), "token index"),
])
def test_unsupported_calls_are_named(cuda, call, option):
    store, x = make_store(70)
    assert store.engine_view() is None
    with pytest.raises(NotImplementedError, match=option):
        call(store, queries(x, 2))
