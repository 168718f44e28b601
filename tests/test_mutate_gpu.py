"""GPU: delete / update / upsert of VectorStore rows in place (csrc/mutate.hip, rag/indexing.py).

The acceptance test needs no tolerance: rows are independent, scores do not depend on where a row sits and ties break by row
number, so a store that was STABLY compacted after a delete is, row for row, the store create_index of the survivors alone
builds -- search results must be identical lists with bit-identical distances.  Same for update (crs::slab_write_rows runs the
append's own per-row function).  The kernels are also checked directly against torch.index_select of clones."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import retrieve_ref as rr, scan_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("ids", "documents", "metadatas", "distances")


def _chunks(n, seed=0, first=0, pages=5):
    from rag.chunking import Chunk
    rng = np.random.default_rng(seed)
    words = "alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma".split()
    out = []
    for i in range(first, first + n):
        text = " ".join(rng.choice(words, size=int(rng.integers(4, 12))))
        out.append(Chunk(text=text, chunk_id=f"chunk_{i}", start_char=0, end_char=len(text), page_number=int(i % pages) + 1,
                         section=None, tokens=len(text.split())))
    return out


def _same(a, b):
    """identical lists, bit-identical distances (python floats compare exactly)"""
    for key in KEYS:
        assert a[key] == b[key], key


# ---- 1. the kernels against torch ------------------------------------------------------------------------------------------------
N_K = 100_003


def _dead_sets(n, rng):
    yield "empty", np.zeros(0, dtype=np.int64)
    yield "all", np.arange(n, dtype=np.int64)
    yield "row 0", np.array([0])
    yield "last row", np.array([n - 1])
    yield "one middle row", np.array([n // 2 + 1])
    yield "every other row", np.arange(0, n, 2)
    yield "random 1 %", np.sort(rng.choice(n, n // 100, replace=False))
    yield "random 50 %", np.sort(rng.choice(n, n // 2, replace=False))
    yield "block of 3 windows", np.arange(20_001, 20_001 + 3 * 1024)


@pytest.mark.parametrize("dim", [100, 101, 384, 768, 1000])
@pytest.mark.parametrize("dtype", ["fp16", "int8"])
def test_slab_compact_against_index_select(cuda, dim, dtype):
    import torch
    from rag import _native as nat
    st = nat.SLAB_I8 if dtype == "int8" else nat.SLAB_F16
    pd = nat.padded_dim(dim, st)
    g = torch.Generator(device=cuda).manual_seed(dim)
    if st == nat.SLAB_I8:
        slab0 = torch.randint(-127, 128, (N_K, pd), device=cuda, generator=g, dtype=torch.int8)
    else:
        slab0 = torch.randn((N_K, pd), device=cuda, generator=g).half()
    scales0 = torch.rand(N_K, device=cuda, generator=g)
    shadow0 = torch.randn((N_K, dim), device=cuda, generator=g)
    rg0 = torch.arange(N_K, device=cuda) * 3 + 7
    least = nat.slab_compact_bounce_bytes(dim, st, True)
    assert nat.slab_compact_window_rows(dim, st, True, least) == 1024          # dozens of windows at the minimum
    rng = np.random.default_rng(dim + st)
    for name, dead_np in _dead_sets(N_K, rng):
        dead = torch.from_numpy(np.asarray(dead_np, dtype=np.int64)).to(cuda)
        keep = torch.ones(N_K, dtype=torch.bool, device=cuda)
        keep[dead] = False
        keep = keep.nonzero().flatten()
        n_out = N_K - dead.numel()
        for bounce_bytes in (None, least):
            slab, scales, shadow, rgl = slab0.clone(), scales0.clone(), shadow0.clone(), rg0.clone()
            ptrs = [t.data_ptr() for t in (slab, scales, shadow, rgl)]
            bounce = None if bounce_bytes is None else torch.empty(bounce_bytes, dtype=torch.uint8, device=cuda)
            first = int(dead_np[0]) if len(dead_np) and bounce_bytes is None else 0      # with and without the host's hint
            nat.slab_compact(dead, N_K, slab, scales=scales, shadow=shadow, rows_global=rgl, bounce=bounce, first_row=first)
            torch.cuda.synchronize()
            tag = (name, bounce_bytes)
            assert ptrs == [t.data_ptr() for t in (slab, scales, shadow, rgl)], tag
            for got, old in ((slab, slab0), (scales, scales0), (shadow, shadow0), (rgl, rg0)):
                assert torch.equal(got[:n_out], old.index_select(0, keep)), tag
                if len(dead_np):
                    assert torch.equal(got[: int(dead_np[0])], old[: int(dead_np[0])]), tag
    # the optional arrays may be absent
    dead = torch.from_numpy(np.arange(5, N_K, 7, dtype=np.int64)).to(cuda)
    keep = torch.ones(N_K, dtype=torch.bool, device=cuda); keep[dead] = False
    slab = slab0.clone()
    nat.slab_compact(dead, N_K, slab, first_row=5)
    assert torch.equal(slab[: N_K - dead.numel()], slab0[keep])


def test_slab_compact_refuses_bad_tensors(cuda):
    import torch
    from rag import _native as nat
    slab = torch.zeros((2048, 384), dtype=torch.float16, device=cuda)
    dead = torch.tensor([3], device=cuda)
    big = torch.empty(nat.slab_compact_bounce_bytes(384, 0, False), dtype=torch.uint8, device=cuda)
    with pytest.raises(nat.NativeError):
        nat.slab_compact(dead.int(), 2048, slab, bounce=big)                      # dead must be int64
    with pytest.raises(nat.NativeError):
        nat.slab_compact(dead.cpu(), 2048, slab, bounce=big)                      # ... on the device
    with pytest.raises(nat.NativeError):
        nat.slab_compact(dead, 4096, slab, bounce=big)                            # n_rows past the slab
    with pytest.raises(nat.NativeError):
        nat.slab_compact(dead, 2048, slab, bounce=big[:1000])                     # bounce too small
    with pytest.raises(nat.NativeError):
        nat.slab_compact(dead, 2048, slab[:, :128], bounce=big)                   # not contiguous
    with pytest.raises(nat.NativeError):
        nat.slab_write_rows_f32(torch.zeros((1, 384), device=cuda), dead.int(), slab, 2048)
    with pytest.raises(nat.NativeError):
        nat.slab_write_rows_f32(torch.zeros((2, 384), device=cuda), dead, slab, 2048)      # rows [m] vs emb [m, dim]


@pytest.mark.parametrize("dim", [100, 101, 384, 768, 1000])
@pytest.mark.parametrize("dtype", ["fp16", "int8"])
def test_slab_write_rows_equals_an_append_of_the_same_vectors(cuda, dim, dtype):
    import torch
    from rag import _native as nat
    st = nat.SLAB_I8 if dtype == "int8" else nat.SLAB_F16
    pd = nat.padded_dim(dim, st)
    n, m = 5000, 700
    g = torch.Generator(device=cuda).manual_seed(dim + 1)
    base = torch.randn((n, dim), device=cuda, generator=g)
    new = torch.randn((m, dim), device=cuda, generator=g) * torch.logspace(-3, 3, m, device=cuda)[:, None]
    rows = torch.randperm(n, device=cuda, generator=g)[:m].contiguous()

    def fresh():
        slab = torch.zeros((n, pd), dtype=torch.int8 if st else torch.float16, device=cuda)
        scales = torch.zeros(n, device=cuda) if st else None
        shadow = torch.zeros((n, dim), device=cuda)
        err = torch.zeros(1, device=cuda)
        nat.slab_append_f32(base, slab, 0, st, scales=scales, shadow=shadow, row_err=err)
        return slab, scales, shadow, err

    slab, scales, shadow, err = fresh()
    before = float(err.item())
    keep = (slab.clone(), shadow.clone())
    nat.slab_write_rows_f32(new, rows, slab, n, scales=scales, shadow=shadow, row_err=err)
    # the same vectors APPENDED into a scratch slab, the error scalar starting from the same value
    s2 = torch.zeros((m, pd), dtype=slab.dtype, device=cuda)
    sc2 = torch.zeros(m, device=cuda) if st else None
    sh2 = torch.zeros((m, dim), device=cuda)
    err2 = torch.full((1,), before, device=cuda)
    nat.slab_append_f32(new, s2, 0, st, scales=sc2, shadow=sh2, row_err=err2)
    torch.cuda.synchronize()
    assert torch.equal(slab[rows], s2) and torch.equal(shadow[rows], sh2)
    if st:
        assert torch.equal(scales[rows], sc2)
    assert float(err.item()) >= before and float(err.item()) == float(err2.item())
    other = torch.ones(n, dtype=torch.bool, device=cuda); other[rows] = False
    assert torch.equal(slab[other], keep[0][other]) and torch.equal(shadow[other], keep[1][other])
    # rows outside the shard are skipped, never written
    nat.slab_write_rows_f32(new[:2].contiguous(), torch.tensor([n + 5, -1], device=cuda), slab, n, scales=scales, shadow=shadow)
    torch.cuda.synchronize()
    assert torch.equal(slab[rows], s2)


# ---- 2. the equivalence -----------------------------------------------------------------------------------------------------------
N_E, D_E = 20_000, 384


def _corpus():
    emb = scan_ref.synth_corpus(N_E, D_E, seed=1)
    q = scan_ref.synth_queries(emb, 64, seed=9)
    dead = np.unique(np.concatenate([np.random.default_rng(0).choice(N_E, N_E // 10, replace=False), [0, N_E - 1]]))
    return emb, q, dead


LAYOUTS = [("fp16", True, 1), ("fp16", True, 2), ("int8", True, 1), ("int8", True, 2), ("fp16", False, 1), ("int8", False, 1)]


def _cfg(dtype, refine, devices, **more):
    cfg = {"index_dtype": dtype, "refine_fp32": refine, **more}
    if devices == 2:
        cfg["devices"] = ["cuda:0", "cuda:0"]
    return cfg


@pytest.mark.parametrize("dtype,refine,devices", LAYOUTS)
def test_delete_equals_a_fresh_index_of_the_survivors(cuda, dtype, refine, devices):
    from rag.indexing import VectorStore
    emb, q, dead = _corpus()
    chunks = _chunks(N_E, 2)
    a = VectorStore(_cfg(dtype, refine, devices))
    for lo, hi in ((0, 12_000), (12_000, N_E)):                     # two adds: growth, uneven shards, a non-identity row map
        a.create_index(chunks[lo:hi], emb[lo:hi])
    ptrs = [(sh.slab.data_ptr(), sh.capacity, sh.rows_global.data_ptr()) for sh in a.collection.shards]
    assert a.delete(ids=[chunks[r].chunk_id for r in dead] + ["no such id"]) == len(dead) and a.mutation_epoch == 1
    assert ptrs == [(sh.slab.data_ptr(), sh.capacity, sh.rows_global.data_ptr()) for sh in a.collection.shards]
    keep = np.setdiff1d(np.arange(N_E), dead)
    b = VectorStore(_cfg(dtype, refine, devices))
    b.create_index([chunks[r] for r in keep], emb[keep])
    sa, sb = a.get_stats(), b.get_stats()
    assert sa["count"] == sb["count"] == len(keep) == a.collection.count() and sum(sa["rows_per_device"]) == len(keep)
    assert sa["slab_bytes"] == sb["slab_bytes"]
    if devices == 1:
        assert a.collection.shards[0].identity and a.engine_view() is not None
        if refine:
            assert np.array_equal(a.rows_f32([0, 5, len(keep) - 1]), b.rows_f32([0, 5, len(keep) - 1]))
    for top_k in (1, 5, 10, 64, 100):
        _same(a.search_batch(q, top_k=top_k), b.search_batch(q, top_k=top_k))
        if refine and dtype == "fp16":
            assert a.last_exactness["unproven"] == 0 and a.last_exactness["queries"] == 64
    assert a.delete(ids=["no such id"]) == 0 and a.mutation_epoch == 1

    if dtype == "fp16" and refine:        # against the oracle, top_k 10, the tolerance of tests/test_store_gpu.py for this comparison
        ref = rr.StoreRef()
        ref.create_index([chunks[r] for r in keep], emb[keep])
        e64 = emb[keep].astype(np.float64)
        e64 /= np.linalg.norm(e64, axis=1, keepdims=True)
        q64 = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
        top11 = -np.sort(-(q64 @ e64.T), axis=1)[:, :11]
        clear = [i for i in range(64) if np.diff(-top11[i]).min() > 1e-5]           # first 11 scores pairwise > 1e-5 apart
        assert len(clear) >= 64 - 6                                                  # at most 10 % of the queries left out
        for i in clear:
            got, exp = a.search(q[i], top_k=10), ref.search(q[i], top_k=10)
            assert got["ids"] == exp["ids"]
            assert np.abs(np.array(got["distances"][0]) - np.array(exp["distances"][0])).max() < 1e-3


@pytest.mark.parametrize("dtype,refine,devices", [("fp16", True, 1), ("fp16", True, 2), ("int8", True, 1), ("fp16", False, 1)])
def test_tie_order_of_exact_duplicates_survives_compaction(cuda, dtype, refine, devices):
    from rag.indexing import VectorStore
    emb, q, _ = _corpus()
    emb = emb.copy()
    dup = np.arange(137, N_E, N_E // 40)[:40]                       # 40 exact copies of one vector, spread over the store
    emb[dup] = emb[137]
    rng = np.random.default_rng(3)
    dead = np.unique(np.concatenate([dup[:-1] + 1 + rng.integers(0, 50, size=39), dup[[4, 17]], rng.choice(N_E, 500, replace=False)]))
    dead = np.setdiff1d(dead, np.setdiff1d(dup, dup[[4, 17]]))       # deleted rows lie BETWEEN the copies; two copies go too
    chunks = _chunks(N_E, 2)
    a = VectorStore(_cfg(dtype, refine, devices))
    a.create_index(chunks, emb)
    assert a.delete(ids=[chunks[r].chunk_id for r in dead]) == len(dead)
    keep = np.setdiff1d(np.arange(N_E), dead)
    b = VectorStore(_cfg(dtype, refine, devices))
    b.create_index([chunks[r] for r in keep], emb[keep])
    qq = np.concatenate([emb[137:138], q[:15]])
    for top_k in (5, 38, 64):
        ga, gb = a.search_batch(qq, top_k=top_k), b.search_batch(qq, top_k=top_k)
        _same(ga, gb)
        left = [chunks[r].chunk_id for r in dup if r not in (dup[4], dup[17])]
        assert ga["ids"][0][: min(top_k, 38)] == left[: min(top_k, 38)]              # the copies, row ascending


# ---- 3. update / upsert -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,refine,devices", [("fp16", True, 1), ("fp16", True, 2), ("int8", True, 1), ("fp16", False, 1)])
def test_update_and_upsert_equal_a_store_built_with_the_new_values(cuda, dtype, refine, devices):
    import torch
    from rag.chunking import Chunk
    from rag.indexing import VectorStore
    n = 6000
    emb = scan_ref.synth_corpus(n, D_E, seed=4)
    q = scan_ref.synth_queries(emb, 32, seed=5)
    chunks = _chunks(n, 6)
    rng = np.random.default_rng(8)
    rows = rng.choice(n, 500, replace=False)
    fresh = scan_ref.synth_corpus(500, D_E, seed=77) * 3.0              # not unit length: the kernel normalises like the append
    a = VectorStore(_cfg(dtype, refine, devices))
    a.create_index(chunks[:2500], emb[:2500]); a.create_index(chunks[2500:], emb[2500:])
    a.search_batch(q, top_k=5, where={"page_number": 2})                  # fills the filter cache with the OLD rows
    ptrs = [sh.slab.data_ptr() for sh in a.collection.shards]
    err0 = [sh.row_err_max() for sh in a.collection.shards]
    a.update([chunks[r].chunk_id for r in rows], embeddings=fresh, documents=[f"new text {r}" for r in rows],
             metadatas=[{"page_number": 2 if r % 2 else 77, "fresh": int(r)} for r in rows])
    assert a.mutation_epoch == 1 and ptrs == [sh.slab.data_ptr() for sh in a.collection.shards]
    assert all(sh.row_err_max() >= e for sh, e in zip(a.collection.shards, err0))
    emb_b = emb.copy(); emb_b[rows] = fresh
    b = VectorStore(_cfg(dtype, refine, devices))
    b.create_index(chunks[:2500], emb_b[:2500]); b.create_index(chunks[2500:], emb_b[2500:])
    col = b.collection
    for r in rows:
        col.documents[r], col.metadatas[r] = f"new text {r}", {"page_number": 2 if r % 2 else 77, "fresh": int(r)}
    qq = np.concatenate([q, fresh[:8]])
    for top_k in (1, 10, 64, 100):
        _same(a.search_batch(qq, top_k=top_k), b.search_batch(qq, top_k=top_k))
    hit = a.search(fresh[3], top_k=1)
    assert hit["ids"][0] == [chunks[rows[3]].chunk_id] and hit["documents"][0] == [f"new text {rows[3]}"]
    # filters: a value that only exists after the update, and a cached filter whose rows changed
    got = a.search_batch(qq, top_k=6, where={"page_number": 77})
    assert all(m["page_number"] == 77 for row in got["metadatas"] for m in row) and len(got["ids"][0]) == 6
    _same(got, b.search_batch(qq, top_k=6, where={"page_number": 77}))
    _same(a.search_batch(qq, top_k=5, where={"page_number": 2}), b.search_batch(qq, top_k=5, where={"page_number": 2}))
    # embeddings as a device tensor, one id, text untouched
    a.update(chunks[11].chunk_id, embeddings=torch.from_numpy(fresh[:1]).to(cuda))
    assert a.search(fresh[0], top_k=2)["ids"][0][0] in (chunks[11].chunk_id, chunks[rows[0]].chunk_id) and a.mutation_epoch == 2

    # every ValueError leaves the store as it was
    before, epoch = a.search_batch(qq, top_k=10), a.mutation_epoch
    bad = [dict(ids=["nobody"], documents=["x"]), dict(ids=[chunks[1].chunk_id] * 2, documents=["x", "y"]),
           dict(ids=[chunks[1].chunk_id], documents=["x", "y"]), dict(ids=[chunks[1].chunk_id], embeddings=np.zeros((1, 100), np.float32)),
           dict(ids=[chunks[1].chunk_id, "nobody"], embeddings=fresh[:2], documents=["x", "y"])]
    for kw in bad:
        with pytest.raises(ValueError):
            a.update(**kw)
    with pytest.raises(ValueError):
        a.upsert(chunks[:2], fresh[:3])
    with pytest.raises(ValueError):
        a.upsert(chunks[:2], np.zeros((2, 100), np.float32))
    with pytest.raises(ValueError):
        a.delete()
    _same(a.search_batch(qq, top_k=10), before)
    assert a.mutation_epoch == epoch

    # upsert: half known ids, half new, interleaved
    a2 = VectorStore(_cfg(dtype, refine, devices))
    a2.create_index(chunks, emb)
    known = rng.choice(n, 200, replace=False)
    up_emb = scan_ref.synth_corpus(400, D_E, seed=99)
    batch = []
    for t in range(200):
        r = int(known[t])
        batch.append(Chunk(text=f"upserted {r}", chunk_id=chunks[r].chunk_id, start_char=0, end_char=5, page_number=9, section=None, tokens=2))
        batch.append(Chunk(text=f"brand new {t}", chunk_id=f"new_{t}", start_char=0, end_char=5, page_number=8, section=None, tokens=3))
    a2.upsert(batch, up_emb)
    assert a2.collection.count() == n + 200 and a2.mutation_epoch == 1
    emb_b2 = emb.copy(); emb_b2[known] = up_emb[0::2]
    ch_b2 = list(chunks)
    for t in range(200):
        ch_b2[int(known[t])] = batch[2 * t]
    b2 = VectorStore(_cfg(dtype, refine, devices))
    b2.create_index(ch_b2, emb_b2)
    b2.create_index(batch[1::2], up_emb[1::2])
    qq2 = np.concatenate([q, up_emb[:16]])
    for top_k in (5, 64):
        _same(a2.search_batch(qq2, top_k=top_k), b2.search_batch(qq2, top_k=top_k))
    _same(a2.search_batch(qq2, top_k=5, where={"page_number": 9}), b2.search_batch(qq2, top_k=5, where={"page_number": 9}))
    # upsert into an empty store is create_index
    a3 = VectorStore(_cfg(dtype, refine, devices))
    a3.upsert(chunks[:50], emb[:50])
    assert a3.collection.count() == 50


# ---- 4. filters and caches --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [1, 2])
def test_filter_caches_do_not_outlive_a_mutation(cuda, devices):
    from rag.indexing import VectorStore
    n = 4000
    emb = scan_ref.synth_corpus(n + 300, D_E, seed=12)
    q = scan_ref.synth_queries(emb, 16, seed=13)
    chunks = _chunks(n, 14) + _chunks(300, 15, first=n, pages=1)          # the 300 later rows are all page 1
    a = VectorStore(_cfg("fp16", True, devices))
    a.create_index(chunks[:n], emb[:n])
    where = {"page_number": 3}
    first = a.search_batch(q, top_k=8, where=where)
    match = a.collection.rows_matching(where, None)
    gone = match[::3]
    assert a.delete(ids=[chunks[r].chunk_id for r in gone]) == len(gone)
    a.create_index(chunks[n: n + len(gone)], emb[n: n + len(gone)])       # the row count is back to the old value
    assert a.collection.count() == n
    keep = np.concatenate([np.setdiff1d(np.arange(n), gone), np.arange(n, n + len(gone))])
    b = VectorStore(_cfg("fp16", True, devices))
    b.create_index([chunks[r] for r in keep[: n - len(gone)]], emb[keep[: n - len(gone)]])
    b.create_index([chunks[r] for r in keep[n - len(gone):]], emb[keep[n - len(gone):]])
    second = a.search_batch(q, top_k=8, where=where)
    _same(second, b.search_batch(q, top_k=8, where=where))
    assert second != first and not ({chunks[r].chunk_id for r in gone} & {i for row in second["ids"] for i in row})
    _same(a.search_batch(q, top_k=20), b.search_batch(q, top_k=20))
    # delete(where=...) / delete(where_document=...) remove exactly rows_matching
    for kw in (dict(where={"page_number": {"$in": [2, 4]}}), dict(where_document={"$contains": "omicron"}),
               dict(ids=[c.chunk_id for c in chunks[:2000]], where={"page_number": 5}, where_document={"$not_contains": "pi"})):
        rows = a.collection.rows_matching(kw.get("where"), kw.get("where_document"))
        if "ids" in kw:
            rows = np.intersect1d(rows, [r for r, i in enumerate(a.collection.ids) if i in set(kw["ids"])])
        want_ids = [i for r, i in enumerate(a.collection.ids) if r not in set(rows.tolist())]
        assert len(rows) > 0 and a.delete(**kw) == len(rows)
        assert a.collection.ids == want_ids
        assert b.delete(ids=[i for i in b.collection.ids if i not in set(want_ids)]) == len(rows)
        _same(a.search_batch(q, top_k=10), b.search_batch(q, top_k=10))
        if "where" in kw and "ids" not in kw:
            assert a.search_batch(q, top_k=3, **kw)["ids"] == [[] for _ in range(16)]
    # the collection delegates as a ChromaDB collection would; deleting everything leaves an empty, usable store
    assert a.collection.delete(ids=list(a.collection.ids)) == len(want_ids)
    assert a.collection.count() == 0 and a.get_stats()["count"] == 0
    assert a.search(q[0], top_k=3) == {"ids": [[]], "documents": [[]], "metadatas": [[]], "distances": [[]]}
    a.create_index(chunks[:100], emb[:100])
    c = VectorStore(_cfg("fp16", True, devices))
    c.create_index(chunks[:100], emb[:100])
    _same(a.search_batch(q, top_k=10), c.search_batch(q, top_k=10))


# ---- 5. the engine ----------------------------------------------------------------------------------------------------------------
def test_engine_is_rebuilt_after_an_update_and_sees_deletes(cuda):
    """retrieve_batch with >= batch_queries questions runs the throughput engine, whose captured graphs hold the shard's
    row-error bound and row count.  (The pipeline is the one tests/test_exactness_contract_gpu.py drives through the engine:
    the synthetic MiniLM encoder.)"""
    from rag import RAGPipeline

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    p = RAGPipeline({"embedding": {"model_name": "synthetic:minilm", "device": "cuda", "batch_size": 64, "normalize": True},
                     "retrieval": {"top_k": 5, "similarity_threshold": 0.0, "rerank": False, "diversity_penalty": 0.0, "batch_queries": 64},
                     "vector_store": {"collection_name": "engine_mut"}})
    p.setup(Stub())
    n = 5000
    chunks = _chunks(n, 21)
    p.vector_store.create_index(chunks, scan_ref.synth_corpus(n, 384, seed=22))
    words = "retrieval generation quantization encoder attention relevance chunks model memory evidence passages index".split()
    questions = [f"what about {words[i % 12]} and {words[(5 * i + 1) % 12]} number {i}" for i in range(80)]
    first = p.retrieve_batch(questions)
    eng0 = p.retriever._engine
    assert eng0 is not None and len(first) == 80
    target = chunks[4321].chunk_id
    assert first[7][0]["chunk_id"] != target
    q_emb = p.embedding_model.embed([questions[7]])
    p.vector_store.update([target], embeddings=np.asarray(q_emb, dtype=np.float32).reshape(1, -1))
    second = p.retrieve_batch(questions)
    assert second[7][0]["chunk_id"] == target and second[7][0]["score"] > 0.999
    assert p.retriever._engine is not None and p.retriever._engine is not eng0
    assert p.remove_documents(ids=[target]) == 1
    third = p.retrieve_batch(questions)
    assert all(c["chunk_id"] != target for hits in third for c in hits)
    assert [c["chunk_id"] for c in third[7]] == [c["chunk_id"] for c in first[7]]
    assert p.remove_documents(where={"page_number": 4}) == sum(1 for r in range(n) if r % 5 == 3 and r != 4321)


# ---- 6. persistence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,devices", [("fp16", 1), ("int8", 2)])
def test_generations_on_disk(cuda, tmp_path, monkeypatch, dtype, devices):
    from rag.indexing import VectorStore
    n = 3000
    emb = scan_ref.synth_corpus(n + 200, D_E, seed=31)
    q = scan_ref.synth_queries(emb, 16, seed=32)
    chunks = _chunks(n + 200, 33)
    cfg = _cfg(dtype, True, devices, persist_directory=str(tmp_path), collection_name="p")
    a = VectorStore(dict(cfg))
    a.create_index(chunks[:n], emb[:n])
    files = lambda: sorted(os.listdir(tmp_path))                                    # noqa: E731
    assert "p.slab.bin" in files() and not any(".g" in f for f in files())
    dead = np.random.default_rng(1).choice(n, 300, replace=False)
    assert a.delete(ids=[chunks[r].chunk_id for r in dead]) == 300
    assert "p.g1.slab.bin" in files() and "p.slab.bin" not in files() and "p.docs.jsonl" not in files()
    assert json.load(open(tmp_path / "p.meta.json"))["gen"] == 1
    keep = np.setdiff1d(np.arange(n), dead)
    b = VectorStore(_cfg(dtype, True, devices))
    b.create_index([chunks[r] for r in keep], emb[keep])
    live = a.search_batch(q, top_k=10)
    re_opened = VectorStore(dict(cfg))
    assert re_opened.get_stats()["count"] == n - 300
    _same(re_opened.search_batch(q, top_k=10), live)
    _same(live, b.search_batch(q, top_k=10))
    # an append continues the current generation's files: they grow by exactly the batch
    pd = a.collection.pdim * (1 if dtype == "int8" else 2)
    size0 = {f: os.path.getsize(tmp_path / f) for f in files()}
    a.create_index(chunks[n: n + 200], emb[n: n + 200])
    assert set(files()) == set(size0)
    assert os.path.getsize(tmp_path / "p.g1.slab.bin") == size0["p.g1.slab.bin"] + 200 * pd
    assert os.path.getsize(tmp_path / "p.g1.shadow.bin") == size0["p.g1.shadow.bin"] + 200 * 4 * D_E
    assert os.path.getsize(tmp_path / "p.g1.docs.jsonl") > size0["p.g1.docs.jsonl"]
    if dtype == "int8":
        assert os.path.getsize(tmp_path / "p.g1.scales.bin") == size0["p.g1.scales.bin"] + 200 * 4
    b.create_index(chunks[n: n + 200], emb[n: n + 200])
    _same(VectorStore(dict(cfg)).search_batch(q, top_k=10), b.search_batch(q, top_k=10))
    # update likewise: a new generation, the old one removed
    new = scan_ref.synth_corpus(20, D_E, seed=34)
    ids = [chunks[r].chunk_id for r in keep[:20]]
    a.update(ids, embeddings=new, documents=[f"t{i}" for i in range(20)])
    b.update(ids, embeddings=new, documents=[f"t{i}" for i in range(20)])
    assert "p.g2.slab.bin" in files() and not any(".g1." in f for f in files())
    live = a.search_batch(np.concatenate([q, new]), top_k=10)
    _same(VectorStore(dict(cfg)).search_batch(np.concatenate([q, new]), top_k=10), live)
    _same(live, b.search_batch(np.concatenate([q, new]), top_k=10))

    # crash safety: the header's rename fails during a delete -> the OLD store re-opens, all rows, same results
    real = os.replace

    def torn(src, dst, *args, **kw):
        if str(dst).endswith("p.meta.json"):
            raise OSError("simulated crash before the header's rename")
        return real(src, dst, *args, **kw)

    monkeypatch.setattr(os, "replace", torn)
    with pytest.raises(OSError):
        a.delete(ids=[chunks[r].chunk_id for r in keep[100:400]])
    monkeypatch.setattr(os, "replace", real)
    assert "p.g3.slab.bin" in files() and "p.g2.slab.bin" in files()                 # the orphan, beside the intact generation
    old = VectorStore(dict(cfg))
    assert old.get_stats()["count"] == n - 300 + 200
    _same(old.search_batch(np.concatenate([q, new]), top_k=10), live)
    # a subsequent successful delete (on the re-opened store) cleans up the orphaned generation
    assert old.delete(ids=[chunks[r].chunk_id for r in keep[100:400]]) == 300
    assert not any(".g2." in f for f in files()) and "p.g3.slab.bin" in files()
    assert sum(f.endswith(".slab.bin") for f in files()) == 1
    b.delete(ids=[chunks[r].chunk_id for r in keep[100:400]])
    _same(VectorStore(dict(cfg)).search_batch(q, top_k=10), b.search_batch(q, top_k=10))
    # the store whose rewrite failed is ahead of the files: its next persist writes a generation of its own
    a.create_index(chunks[:1], emb[:1])
    assert VectorStore(dict(cfg)).get_stats()["count"] == a.collection.count()
    old.delete_collection()
    assert files() == [] or all(not f.startswith("p.") for f in files())


# ---- 7. memory --------------------------------------------------------------------------------------------------------------------
def test_delete_allocates_no_more_than_the_bounce_buffer(cuda):
    """2 000 000 x 384 fp16 + fp32 shadow (4.6 GB of arrays): a delete of a random 1 % may raise the peak by the bounce buffer
    (256 MB) + 64 MB for index tensors and allocator rounding.  Derived, not measured: nothing else in the design is
    proportional to N."""
    import torch
    from rag.indexing import VectorStore
    n = 2_000_000
    store = VectorStore({})
    g = torch.Generator(device=cuda).manual_seed(1)
    for lo in range(0, n, 500_000):
        emb = torch.randn((500_000, D_E), device=cuda, generator=g)
        store.create_index([_FakeChunk(i) for i in range(lo, lo + 500_000)], emb)
        del emb
    sh = store.collection.shards[0]
    ptrs = (sh.slab.data_ptr(), sh.shadow.data_ptr(), sh.rows_global.data_ptr(), sh.capacity)
    dead = np.sort(np.random.default_rng(2).choice(n, n // 100, replace=False))
    probe = torch.from_numpy(dead[:1000].copy()).to(cuda)
    survivors = np.setdiff1d(np.arange(n), dead)
    want = sh.shadow[torch.from_numpy(survivors[-2000:]).to(cuda)].clone()
    ids = [f"c{r}" for r in dead]
    store.collection._id_rows()
    torch.cuda.synchronize(); torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    assert store.delete(ids=ids) == len(dead)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak rise across the delete: {rise / 2**20:.1f} MiB")
    assert rise <= (256 << 20) + (64 << 20)
    assert ptrs == (sh.slab.data_ptr(), sh.shadow.data_ptr(), sh.rows_global.data_ptr(), sh.capacity) and sh.n == n - len(dead)
    assert torch.equal(sh.shadow[sh.n - 2000: sh.n], want)
    del probe


class _FakeChunk:
    __slots__ = ("chunk_id", "text", "page_number", "section", "tokens")

    def __init__(self, i):
        self.chunk_id, self.text, self.page_number, self.section, self.tokens = f"c{i}", "t", 1, None, 1


# ---- 8. SPMD ----------------------------------------------------------------------------------------------------------------------
def test_spmd_two_ranks_delete_and_update(cuda, tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", os.path.join(ROOT, "tests", "_mutate_sharded_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for rank in range(2):
        v = json.load(open(tmp_path / f"verdict_{rank}.json"))
        assert v["world"] == 2 and len(v["checks"]) >= 12
        bad = [name for name, ok in v["checks"] if not ok]
        assert not bad, (rank, bad)
