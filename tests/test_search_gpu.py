"""GPU: the one search of a device's rows (rag/_search.py) through both calling styles -- allocating (the store's) and on the
caller's buffers (the engine's) -- and the status-2 retry above the kernel level: through VectorStore, and for the engine's
overflow queries through the store's private entry.  (The kernels' own overflow behaviour: test_exact_gpu.py; the engine path end
to end on a 200 k-row index: test_exactness_contract_gpu.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D = 384


def _chunks(n):
    from rag.chunking import Chunk
    return [Chunk(text=f"t{r}", chunk_id=f"c_{r}", start_char=0, end_char=1) for r in range(n)]


@pytest.fixture(scope="module")
def planted_5k(cuda):
    """5 000 x 384 fp16 rows with the fp32 shadow, as one view; 64 unit queries, half planted near a row, and their fp16 block"""
    import torch
    from rag import _native as nat
    from rag.indexing import VectorStore
    g = torch.Generator(device=cuda); g.manual_seed(5000)
    n, nq = 5000, 64
    store = VectorStore({"collection_name": "search5k"})
    store.create_index(_chunks(n), torch.randn((n, D), generator=g, device=cuda))
    view = store.engine_view()
    q = torch.randn((nq, D), generator=g, device=cuda)
    j = torch.randint(0, n, (nq,), generator=g, device=cuda)
    q[0::2] = view.shadow[j[0::2]] + 0.1 * q[0::2]
    q32 = torch.nn.functional.normalize(q, dim=1).contiguous()
    return store, view, q32, nat.queries_to_f16(q32, view.slab_type)


@pytest.mark.parametrize("top_k", [10, 100])
def test_allocating_and_on_the_callers_buffers_give_the_same_bits(planted_5k, cuda, top_k):
    import torch
    from rag import _native as nat
    from rag import _search
    store, view, q32, q16 = planted_5k
    nq = q32.shape[0]
    k_scan = nat.overfetch(nq, top_k, store.refine_overfetch, view.n, view.slab_type)
    cap = _search.first_cap(store.exact_cap, top_k)
    s0, i0, st0 = _search.search_certified(view, q32, q16, k_scan, top_k, cap, True)
    junk = lambda shape, dtype: torch.full(shape, 0x5A if dtype == torch.uint8 else -7, dtype=dtype, device=cuda)    # noqa: E731
    b = _search.SearchBuffers()
    ws_bytes = (nat.scan_workspace_bytes(nq, D, k_scan, view.n) if top_k <= nat.MAX_K else
                nat.large_cert_workspace_bytes(nq, D, top_k, view.n))
    b.ws = junk((ws_bytes,), torch.uint8)
    b.exact_ws = junk((nat.exact_workspace_bytes(nq, cap),), torch.uint8)
    b.cand_s, b.cand_i = junk((nq, k_scan), torch.float32), junk((nq, k_scan), torch.int64)
    b.out_s, b.out_i = junk((nq, top_k), torch.float32), junk((nq, top_k), torch.int64)
    b.status = junk((nq,), torch.int32)
    s1, i1, st1 = _search.search_certified(view, q32, q16, k_scan, top_k, cap, True, b)
    torch.cuda.synchronize()
    assert s1 is b.out_s and i1 is b.out_i and st1 is b.status, "the caller's buffers were not the ones written"
    assert torch.equal(s0.view(torch.int32), s1.view(torch.int32)), "scores differ in their bits"
    assert torch.equal(i0, i1) and torch.equal(st0, st1)
    assert set(st0.cpu().numpy().tolist()) <= {0, 1} and int(i0.min()) >= 0 and int(i0.max()) < view.n


@pytest.fixture(scope="module")
def band_2k(cuda):
    """2 000 x 384 rows, 200 of them one vector v, in a store whose first escalation list holds 64 rows; 16 unit queries, the
    first equal to v"""
    import torch
    from rag.indexing import VectorStore
    g = torch.Generator(device=cuda); g.manual_seed(2000)
    n, ndup = 2000, 200
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    v = torch.nn.functional.normalize(torch.randn((1, D), generator=g, device=cuda), dim=1)
    pos = torch.randperm(n, generator=g, device=cuda)[:ndup]
    rows[pos] = v
    store = VectorStore({"collection_name": "band2k", "exact_cap": 64})
    store.create_index(_chunks(n), rows)
    q = torch.cat([v, torch.nn.functional.normalize(torch.randn((15, D), generator=g, device=cuda), dim=1)]).contiguous()
    return store, q, np.sort(pos.cpu().numpy())


def test_store_retries_an_overflowing_list_with_a_longer_one(band_2k):
    """a list of 64 cannot hold the band of 200 (status 2, as test_exact_gpu.py pins for the kernels): the store's retry must
    reach a length that does"""
    store, q, pos = band_2k
    s, i = store.search_rows(q[:4].cpu().numpy(), 10)
    ex = dict(store.last_exactness)
    print("last_exactness:", ex)
    assert np.array_equal(i[0], pos[:10]), "exact ties: the ten lowest duplicate rows"
    assert ex["queries"] == 4 and ex["unproven"] == 0 and ex["escalated"] >= 1 and ex["mode"] == "certificate", ex
    assert ex["certified"] + ex["escalated"] == 4, ex


def test_engine_overflow_queries_are_resolved_through_the_store(band_2k, cuda):
    import torch
    from rag import _search
    from rag._engine import RetrievalEngine
    store, q, pos = band_2k
    eng = RetrievalEngine(None, store.engine_view(), 16, 16, 10, k_scan=store.refine_overfetch, exact=store.refine_exact,
                          exact_cap=64, encode=False)
    for grp in eng.groups:              # encode=False: the caller writes the embeddings (every buffer set: warm_up runs them all)
        grp.q_out.copy_(q.repeat(grp.q_out.shape[0] // 16, 1))
    eng.warm_up()
    eng.submit(0)
    eng.wait(0)
    s, r, st = (t.cpu().numpy() for t in eng.outputs(0))
    torch.cuda.synchronize()
    print("engine status:", st.tolist())
    assert st[0] == 2, f"the band of 200 must overflow the engine's list of 64: {st.tolist()}"
    s2, r2, again = store._search_rows(q[:1].cpu().numpy(), 10)
    assert np.array_equal(r2[0], pos[:10])
    assert again["queries"] == 1 and again["unproven"] == 0, again
    over = int((st == 2).sum())
    s2, r2, again = store._search_rows(q[torch.as_tensor(np.nonzero(st == 2)[0], device=cuda)].cpu().numpy(), 10)
    both = _search.retried_tally(_search.tally(st, 16, 10, eng.refine, eng.exact), again)
    print("combined tally:", both)
    assert again["queries"] == over
    assert both["queries"] == 16 and both["certified"] + both["escalated"] + both["unproven"] == 16, both
    assert both["unproven"] == 0, both
