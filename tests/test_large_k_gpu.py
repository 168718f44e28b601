"""GPU: certified exact fp32 search for top_k 65 .. 1024 (crs::cosine_topk_large_cert, csrc/large_k.hip).

Above one scan's 64 candidates the store over-fetches by partition (64 from each of up to 64 row chunks), re-ranks every
candidate in fp32 against the shadow and proves the list per query, escalating unproven queries on the device as the
top_k <= 64 path does.  Held here against the oracle fed the fp32 shadow rows: the ids of every claimed list, the tally
(mode 'certificate', nothing unproven on fp16), the certified share of random queries, and the kernel's refusal of candidate
blocks that do not cover their chunks."""
import numpy as np
import pytest

from topk_check import assert_topk, topk_errors

pytestmark = pytest.mark.gpu

D = 384
TOL = 3e-7          # random corpora
BAND_TOL = 2e-6     # near-duplicate bands
KS = (65, 100, 256, 1000, 1024)


def _chunks(n, pages=False):
    from rag.chunking import Chunk
    return [Chunk(text=f"t{r}", chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=(r % 10) if pages else None)
            for r in range(n)]


def _store(cfg, emb, pages=False):
    from rag.indexing import VectorStore
    store = VectorStore(cfg)
    n = emb.shape[0]
    chunks = _chunks(n, pages)
    for lo in range(0, n, 250_000):
        store.create_index(chunks[lo:lo + 250_000], emb[lo:lo + 250_000].contiguous(),
                           metadata_fields=["page_number"] if pages else None)
    return store


def _tally_ok(ex, nq, what, escalates=True):
    assert ex["mode"] == "certificate", f"{what}: {ex}"
    assert ex["queries"] == nq and ex["certified"] + ex["escalated"] + ex["unproven"] == nq, f"{what}: {ex}"
    if escalates:
        assert ex["unproven"] == 0, f"{what}: {ex}"


@pytest.fixture(scope="module")
def band_300k(cuda):
    """300 k x 384 unit rows (page_number = row % 10) with a band of 6000 near-identical rows -- more than the 4096 candidates
    of the deepest partition, so no over-fetch holds it.  64 queries: 0 and 1 on the band, the other even ones planted near a
    row, the odd ones random."""
    import torch
    from types import SimpleNamespace
    g = torch.Generator(device=cuda); g.manual_seed(1024)
    n, nq, nb = 300_000, 64, 6000
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    centre = torch.nn.functional.normalize(torch.randn((1, D), generator=g, device=cuda), dim=1)
    band = torch.randperm(n, generator=g, device=cuda)[:nb]
    rows[band] = centre + 2e-4 * torch.randn((nb, D), generator=g, device=cuda)
    store = _store({"collection_name": "large-k"}, rows, pages=True)
    sh_rows = store.collection.shadow[:n]
    q = torch.randn((nq, D), generator=g, device=cuda)
    j = torch.randint(0, n, (nq,), generator=g, device=cuda)
    q[0::2] = sh_rows[j[0::2]] + 0.1 * q[0::2]
    q[:2] = centre + 1e-5 * torch.randn((2, D), generator=g, device=cuda)
    q = torch.nn.functional.normalize(q, dim=1).contiguous()
    q_h, rows_h = q.cpu().numpy(), sh_rows.cpu().numpy()
    from oracle import scan_ref
    return SimpleNamespace(store=store, n=n, q=q, q_h=q_h, rows=rows_h, ref=scan_ref.cosine_topk_ref(q_h, rows_h, 1024),
                           band_q=np.array([0, 1]), random_q=np.arange(3, nq, 2))


@pytest.mark.parametrize("k", KS)
def test_fp16_store_is_certified_and_exact_at_large_top_k(band_300k, cuda, k):
    """ids equal the oracle's; the tally is a certificate with nothing unproven; >= 95 % of the random queries are proven by the
    partitioned over-fetch alone; the band queries are escalated and exact."""
    import torch
    from rag import _native as nat
    st = band_300k
    store, q_h, rows_h = st.store, st.q_h, st.rows
    nq = q_h.shape[0]
    s, i = store.search_rows(q_h, k)
    ex = dict(store.last_exactness)
    _tally_ok(ex, nq, f"top_k {k}")
    rs, ri = st.ref[0][:, :k], st.ref[1][:, :k]
    wrong = topk_errors(i, q_h, rows_h, ri, k, BAND_TOL)
    assert not wrong, f"top_k {k}: {len(wrong)} lists differ from the oracle: {list(wrong.items())[:3]}"
    assert np.abs(s - rs).max() < 1e-5
    # per query, straight from the kernels: which queries the certificate proves before any escalation
    sh = store.collection.shards[0]
    cap = store._cap(k)
    ws = sh.exact_workspace(nq, cap)
    q16 = nat.queries_to_f16(st.q, nat.SLAB_F16)
    _, _, status = nat.cosine_topk_large_cert(st.q, q16, sh.slab, sh.shadow, st.n, D, k, sh.row_err_max(), ws, cap)
    status = status.cpu().numpy()
    torch.cuda.synchronize()
    frac = float((status[st.random_q] == 0).mean())
    assert frac >= 0.95, f"top_k {k}: only {frac:.3f} of the random queries certified: {status[st.random_q].tolist()}"
    assert (status[st.band_q] == 1).all(), f"top_k {k}: band queries must need the escalation: {status[st.band_q]}"
    assert ex["escalated"] >= len(st.band_q), f"top_k {k}: {ex}"
    assert_topk(s[st.band_q], i[st.band_q], q_h[st.band_q], rows_h, k, f"band top_k {k}", tol=BAND_TOL,
                ref=(rs[st.band_q], ri[st.band_q]))


def test_top_k_100_starts_with_the_top_k_64_list_bit_for_bit(band_300k):
    st = band_300k
    s64, i64 = st.store.search_rows(st.q_h, 64)
    s100, i100 = st.store.search_rows(st.q_h, 100)
    assert np.array_equal(i100[:, :64], i64)
    assert np.array_equal(s100[:, :64].view(np.int32), s64.view(np.int32)), "fp32 scores differ between the two paths"


def test_search_and_search_batch_agree_with_search_rows(band_300k):
    st = band_300k
    k = 128
    _, ri = st.store.search_rows(st.q_h[:8], k)
    res = st.store.search_batch(st.q_h[:8], top_k=k)
    assert [[int(x[2:]) for x in ids] for ids in res["ids"]] == ri.tolist()
    one = st.store.search(st.q_h[3], top_k=k)
    assert [int(x[2:]) for x in one["ids"][0]] == ri[3].tolist()
    _tally_ok(st.store.last_exactness, 1, "search")


def test_filtered_search_at_top_k_128(band_300k):
    """a `where` filter scans the compacted rows of page 3 (30 k rows): the oracle on those rows"""
    from oracle import scan_ref
    st = band_300k
    k = 128
    allowed = np.arange(3, st.n, 10)
    res = st.store.search_batch(st.q_h, top_k=k, where={"page_number": 3})
    _tally_ok(st.store.last_exactness, len(st.q_h), "filtered")
    got = np.array([[int(x[2:]) for x in ids] for ids in res["ids"]])
    local = np.searchsorted(allowed, got)
    assert (allowed[local] == got).all(), "a filtered search returned a row outside the filter"
    sub = st.rows[allowed]
    rs, ri = scan_ref.cosine_topk_ref(st.q_h, sub, k)
    got_s = (1.0 - np.asarray(res["distances"], dtype=np.float64)).astype(np.float32)
    wrong = topk_errors(local, st.q_h, sub, ri, k, BAND_TOL)
    assert not wrong, f"filtered top_k {k}: {list(wrong.items())[:3]}"
    assert np.abs(got_s - rs).max() < 1e-5


@pytest.mark.parametrize("n, k", [(700, 256), (3001, 1000), (4000, 65), (20_011, 1024)])
def test_shards_near_the_partition_sizes(cuda, n, k):
    """single shards between k and P x 64 rows, and n_rows not a multiple of 16"""
    import torch
    from oracle import scan_ref
    g = torch.Generator(device=cuda); g.manual_seed(n)
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    store = _store({"collection_name": f"edge{n}"}, rows)
    rows_h = store.collection.shadow[:n].cpu().numpy()
    q_h = torch.nn.functional.normalize(torch.randn((16, D), generator=g, device=cuda), dim=1).cpu().numpy()
    s, i = store.search_rows(q_h, k)
    _tally_ok(store.last_exactness, 16, f"n {n} top_k {k}")
    assert_topk(s, i, q_h, rows_h, k, f"n {n} top_k {k}", tol=TOL)


@pytest.mark.parametrize("n, k", [(150, 100), (1000, 1000), (40_001, 300)])
def test_two_shards_on_one_device(cuda, n, k):
    """devices ["cuda:0", "cuda:0"]: two shards (the second with a row map), each possibly smaller than top_k, merged by
    (score desc, row asc)"""
    import torch
    from oracle import scan_ref
    g = torch.Generator(device=cuda); g.manual_seed(7 * n)
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    store = _store({"collection_name": f"two{n}", "devices": ["cuda:0", "cuda:0"]}, rows)
    assert len(store.collection.shards) == 2 and not store.collection.shards[1].identity
    rows_h = rows.cpu().numpy()
    q_h = torch.nn.functional.normalize(torch.randn((8, D), generator=g, device=cuda), dim=1).cpu().numpy()
    s, i = store.search_rows(q_h, k)
    _tally_ok(store.last_exactness, 8, f"two shards n {n} top_k {k}")
    assert_topk(s, i, q_h, rows_h, k, f"two shards n {n} top_k {k}", tol=TOL)


def test_768_dim_rows_at_top_k_128(cuda):
    import torch
    g = torch.Generator(device=cuda); g.manual_seed(768)
    n, d, k = 60_000, 768, 128
    rows = torch.nn.functional.normalize(torch.randn((n, d), generator=g, device=cuda), dim=1)
    store = _store({"collection_name": "wide"}, rows)
    rows_h = store.collection.shadow[:n].cpu().numpy()
    q = torch.randn((32, d), generator=g, device=cuda)
    q[0::2] = rows[:16] + 0.1 * q[0::2]
    q_h = torch.nn.functional.normalize(q, dim=1).cpu().numpy()
    s, i = store.search_rows(q_h, k)
    _tally_ok(store.last_exactness, 32, "768-d top_k 128")
    assert_topk(s, i, q_h, rows_h, k, "768-d top_k 128", tol=TOL)


def test_int8_768_dim_claims_hold(cuda):
    """int8 under 'auto' stays empirical (no escalation): the lists that differ from the oracle number at most `unproven`.  With
    refine_exact=True every list is the oracle's."""
    import torch
    from oracle import scan_ref
    g = torch.Generator(device=cuda); g.manual_seed(8)
    n, d, nq = 100_000, 768, 32
    rows = torch.nn.functional.normalize(torch.randn((n, d), generator=g, device=cuda), dim=1)
    q = torch.randn((nq, d), generator=g, device=cuda)
    q[0::2] = rows[:nq // 2] + 0.1 * q[0::2]
    q_h = torch.nn.functional.normalize(q, dim=1).cpu().numpy()
    auto = _store({"collection_name": "i8auto-large", "index_dtype": "int8"}, rows)
    rows_h = auto.collection.shadow[:n].cpu().numpy()
    ref = scan_ref.cosine_topk_ref(q_h, rows_h, 300)
    for k in (128, 300):
        _, i = auto.search_rows(q_h, k)
        ex = dict(auto.last_exactness)
        _tally_ok(ex, nq, f"int8 auto top_k {k}", escalates=False)
        assert ex["escalated"] == 0, ex
        wrong = topk_errors(i, q_h, rows_h, ref[1][:, :k], k, TOL)
        assert len(wrong) <= ex["unproven"], f"int8 auto top_k {k}: {len(wrong)} wrong lists, {ex}"
    del auto
    exact = _store({"collection_name": "i8exact-large", "index_dtype": "int8", "refine_exact": True}, rows)
    for k in (128, 300):
        s, i = exact.search_rows(q_h, k)
        _tally_ok(exact.last_exactness, nq, f"int8 exact top_k {k}")
        assert_topk(s, i, q_h, rows_h, k, f"int8 exact top_k {k}", tol=TOL, ref=(ref[0][:, :k], ref[1][:, :k]))


def test_kernel_refuses_candidate_blocks_that_do_not_cover_their_chunks(cuda):
    """refine_large_cert on candidate blocks the test builds from per-chunk scans (id_base 1000): a -1 slot on a full chunk and
    an id outside its chunk give status 1; a small shard listed whole gives status 0; after escalate_exact every list is the
    oracle's."""
    import torch
    from oracle import scan_ref
    from rag import _native as nat
    g = torch.Generator(device=cuda); g.manual_seed(55)
    base, k, nq = 1000, 100, 6
    for n, case in ((3000, "intact"), (3000, "hole"), (3000, "outside"), (40, "whole-small")):
        rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
        slab = torch.zeros((n, nat.padded_dim(D)), dtype=torch.float16, device=cuda)
        shadow = torch.empty((n, D), dtype=torch.float32, device=cuda)
        err = torch.zeros(1, dtype=torch.float32, device=cuda)
        nat.slab_append_f32(rows, slab, 0, nat.SLAB_F16, shadow=shadow, row_err=err)
        q = torch.nn.functional.normalize(torch.randn((nq, D), generator=g, device=cuda), dim=1).contiguous()
        q16 = nat.queries_to_f16(q)
        parts, chunk = nat.large_k_plan(k, n)
        cs = torch.empty((parts, nq, 64), dtype=torch.float32, device=cuda)
        ci = torch.empty((parts, nq, 64), dtype=torch.int64, device=cuda)
        for p in range(parts):
            lo, hi = p * chunk, min(n, (p + 1) * chunk)
            cs[p], ci[p] = nat.cosine_topk(q16, slab[lo:hi].contiguous(), hi - lo, D, 64, id_base=base + lo)
        if case == "hole":
            ci[0, 0, 63], cs[0, 0, 63] = -1, float("-inf")
        elif case == "outside":
            ci[1, 0, 5] = base + 0            # a row of chunk 0 listed in chunk 1
        cap = 4 * k
        ws = torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=cuda)
        s, i, st = nat.refine_large_cert(q, q16, shadow, n, base, ci, cs, chunk, k, float(err.item()), nat.SLAB_F16, ws, cap)
        st_h = st.cpu().numpy()
        if case in ("hole", "outside"):
            assert st_h[0] == 1, f"{case}: status {st_h}"
        if case == "whole-small":
            assert (st_h == 0).all(), f"{case}: status {st_h}"
            assert (i[:, n:].cpu().numpy() == -1).all() and np.isneginf(s[:, n:].cpu().numpy()).all()
        nat.escalate_exact(q, q16, slab, shadow, n, base, k, s, i, st, ws, cap)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() != 2).all()
        q_h, rows_h = q.cpu().numpy(), shadow.cpu().numpy()
        rs, ri = scan_ref.cosine_topk_ref(q_h, rows_h, k)
        got = i.cpu().numpy()
        kk = min(k, n)
        got_l = np.where(got[:, :kk] >= 0, got[:, :kk] - base, -1)
        wrong = topk_errors(got_l, q_h, rows_h, ri[:, :kk], kk, TOL)
        assert not wrong, f"{case}: {wrong}"
        assert np.abs(s.cpu().numpy()[:, :kk] - rs[:, :kk]).max() < 1e-5, case


WORDS = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine "
         "similarity vector index chunk context answer question compression memory latency throughput").split()


def test_retrieve_batch_with_rerank_fetches_80_certified(cuda):
    """rerank on, top_k 40: retrieve_batch fetches 80 rows per question through the certified path; each question's chunks are
    what _post_process builds from the oracle's 80 rows."""
    import torch
    from oracle import scan_ref
    from rag import RAGPipeline

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    cfg = {"embedding": {"model_name": "synthetic:minilm", "device": "cuda", "batch_size": 64, "normalize": True},
           "retrieval": {"top_k": 40, "similarity_threshold": 0.0, "rerank": True, "diversity_penalty": 0.0, "batch_queries": 64},
           "vector_store": {"collection_name": "retr-large"}}
    p = RAGPipeline(cfg)
    p.setup(Stub())
    n = 200_000
    g = torch.Generator(device=cuda); g.manual_seed(40)
    p.vector_store.create_index(_chunks(n), torch.randn((n, D), generator=g, device=cuda))
    rng = np.random.default_rng(40)
    questions = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 9)))) + f" {q}" for q in range(256)]
    got = p.retrieve_batch(questions)
    store = p.vector_store
    _tally_ok(store.last_exactness, len(questions), "retrieve_batch top_k 40")
    r = p.retriever
    model = p.embedding_model
    emb = model.embed_device(list(questions)) if hasattr(model, "embed_device") else model.embed(list(questions))
    q = torch.as_tensor(emb, device=cuda, dtype=torch.float32)
    q_h = torch.nn.functional.normalize(q, dim=1).cpu().numpy()
    rows_h = store.collection.shadow[:n].cpu().numpy()
    rs, ri = scan_ref.cosine_topk_ref(q_h, rows_h, 80)
    col = store.collection
    for a, question in enumerate(questions):
        dist = (np.float32(1.0) - rs[a].astype(np.float32)).astype(np.float64)
        chunks = r._hits_to_chunks([col.ids[x] for x in ri[a]], [col.documents[x] for x in ri[a]],
                                   [col.metadatas[x] for x in ri[a]], dist.tolist())
        want = r._post_process(question, chunks, 40)
        assert [c["chunk_id"] for c in got[a]] == [c["chunk_id"] for c in want], f"question {a}"
        assert max(abs(x["score"] - y["score"]) for x, y in zip(got[a], want)) < 1e-5
