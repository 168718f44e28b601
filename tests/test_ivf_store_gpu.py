"""The ``ivf`` option of VectorStore (rag/_ivf.py) beside a flat store of the same rows: identical answers when every
list is probed, the invariants of the lists through build, append and delete, the fallbacks to the certified path, the refusals.
Recall at small nprobe is a property of the data and of k-means: tools/bench_ivf.py reports it, nothing here asserts it."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, NLIST, NQ = 3000, 32, 64


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def chunks_of(first, count):
    from rag.chunking import Chunk
    return [Chunk(text=f"text {i}", chunk_id=f"c_{i}", start_char=0, end_char=1, page_number=i % 4) for i in range(first, first + count)]


def make_stores(dim, **ivf):
    """(flat store, ivf store, rows, queries): N random unit rows, NQ random unit queries."""
    from rag.indexing import VectorStore
    rng = np.random.default_rng(dim)
    x, q = unit(rng.standard_normal((N, dim))), unit(rng.standard_normal((NQ, dim)))
    stores = [VectorStore(dict({"collection_name": f"ivf{dim}_{on}"}, **({"ivf": dict({"min_rows": 0, "nlist": NLIST}, **ivf)} if on else {})))
              for on in (0, 1)]
    for store in stores:
        store.create_index(chunks_of(0, N), x)
    return stores[0], stores[1], x, q


def same_answer(a, b):
    return a["ids"] == b["ids"] and np.array_equal(np.array(a["distances"], np.float32).view(np.uint32), np.array(b["distances"], np.float32).view(np.uint32))


def check_lists(store, n):
    """list_rows is a permutation, list_offsets monotone, and every row sits in the list of its fp64 arg-max centroid unless the
    two best centroid scores lie within the scan's score bound (twice pdim 2^-24 sum |c_i x_i|: one bound per score)."""
    index, sh = store.ivf_index(), store.collection.shards[0]
    offsets, rows = index.list_offsets.cpu().numpy(), index.list_rows.cpu().numpy()
    assert np.array_equal(np.sort(rows), np.arange(n)) and offsets[0] == 0 and offsets[-1] == n and (np.diff(offsets) >= 0).all()
    assign = np.empty(n, np.int64)
    for l in range(index.nlist):
        assert (np.diff(rows[offsets[l]:offsets[l + 1]]) > 0).all()
        assign[rows[offsets[l]:offsets[l + 1]]] = l
    c, x = index.centroids.cpu().numpy().astype(np.float64), sh.slab[:n].cpu().numpy().astype(np.float64)
    score = x @ c.T
    bound = x.shape[1] * 2.0 ** -24 * (np.abs(x) @ np.abs(c).T)
    top = np.sort(score, axis=1)[:, -2:]
    differ = assign != score.argmax(1)
    assert not (differ & (top[:, 1] - top[:, 0] > 2 * bound.max(1))).any() and differ.mean() <= 0.01
    return index


@pytest.mark.parametrize("dim", [384, 100])
def test_probing_every_list_is_the_flat_answer(cuda, dim):
    flat, ivf, x, q = make_stores(dim, nprobe=NLIST)
    want = flat.search_batch(q, top_k=10)
    assert flat.last_exactness["mode"] == "certificate" and flat.last_exactness["unproven"] == 0
    assert same_answer(ivf.search_batch(q, top_k=10), want)
    assert ivf.last_exactness == {"queries": NQ, "certified": 0, "escalated": 0, "unproven": NQ, "mode": "ivf"}
    assert ivf.engine_view() is None and flat.engine_view() is not None
    stats = ivf.get_stats()["ivf"]
    assert stats["nlist"] == NLIST and stats["nprobe"] == NLIST and stats["built"] and 0 < stats["largest_list"] <= N
    assert "ivf" not in flat.get_stats()
    assert same_answer(ivf.search(q[0], top_k=10), flat.search(q[0], top_k=10))


@pytest.mark.parametrize("dim", [384, 100])
def test_lists_through_build_append_and_delete(cuda, dim):
    flat, ivf, x, q = make_stores(dim)
    index = check_lists(ivf, N)
    centroids = index.centroids.cpu().numpy().copy()
    extra = unit(np.random.default_rng(5).standard_normal((200, dim)))
    for store in (flat, ivf):
        store.create_index(chunks_of(N, 200), extra)
    assert check_lists(ivf, N + 200) is index and np.array_equal(index.centroids.cpu().numpy().view(np.uint16), centroids.view(np.uint16))
    ivf.nprobe = 1
    assert [ids[0] for ids in ivf.search_batch(extra[:16], top_k=3)["ids"]] == [f"c_{N + i}" for i in range(16)]
    dead = [f"c_{i}" for i in range(7, 3007, 300)]
    assert flat.delete(ids=dead) == 10 and ivf.delete(ids=dead) == 10
    assert not ivf.get_stats()["ivf"]["built"]
    ivf.nprobe = NLIST
    assert same_answer(ivf.search_batch(q, top_k=10), flat.search_batch(q, top_k=10))
    assert ivf.get_stats()["ivf"]["built"]
    check_lists(ivf, N + 190)


@pytest.mark.parametrize("search", [lambda s, q: s.search_batch(q, top_k=10, where={"page_number": 2}), lambda s, q: s.search_batch(q, top_k=100)],
                         ids=["where", "top_k 100"])
def test_filters_and_large_k_take_the_certified_path(cuda, search):
    flat, ivf, x, q = make_stores(384, nprobe=1)
    assert same_answer(search(ivf, q), search(flat, q))
    assert ivf.last_exactness == flat.last_exactness and ivf.last_exactness["mode"] == "certificate"


def test_below_min_rows_the_store_searches_flat(cuda):
    flat, ivf, x, q = make_stores(384, nprobe=1, min_rows=N + 1)
    assert same_answer(ivf.search_batch(q, top_k=10), flat.search_batch(q, top_k=10))
    assert ivf.last_exactness == flat.last_exactness and not ivf.get_stats()["ivf"]["built"] and ivf.engine_view() is not None


@pytest.mark.parametrize("option, name", [({"index_dtype": "int8"}, "index_dtype"), ({"index_dtype": "mxfp4"}, "index_dtype"),
                                          ({"space": "ip"}, "space"), ({"sharded": True}, "sharded"), ({"num_gpus": 2}, "num_gpus"),
                                          ({"devices": [0]}, "devices")])
def test_refusals_name_the_option(cuda, option, name):
    from rag.indexing import VectorStore
    with pytest.raises(NotImplementedError, match=name):
        VectorStore(dict({"ivf": {}}, **option))
