"""GPU: the exactness claim at every top_k and on every search path.

The store fetches k' candidates from the fp16 / int8 slab, re-ranks them in fp32 against the shadow rows, and then either
proves the list (crs::refine_f32_cert) or escalates the query (crs::escalate_exact).  ``VectorStore.last_exactness`` says
how many queries of the LAST search were certified, escalated or left unproven.  The invariant held here, on the kernels
(per query, by the status array) and through the store (by the counts):

    a claim is true -- every query counted certified or escalated (status 0 / 1 after escalation) has exactly the ids of
    the oracle fed the fp32 shadow rows, up to swaps between rows whose fp64 scores differ by less than fp32 summation can
    resolve; the counts describe this search and add up to its query count.

Through the store only counts exist: the queries whose ids differ from the oracle number at most ``unproven``.
Also held: the over-fetch keeps a margin at the sizes callers use (``rerank: true`` asks for 2 x top_k rows), so that
random queries are certified instead of paying an escalation sweep each."""
import numpy as np
import pytest

from topk_check import assert_topk, topk_errors

pytestmark = pytest.mark.gpu

D = 384
TOL = 3e-7          # random corpora (|score| ~ 0.3)
BAND_TOL = 2e-6     # near-duplicate bands (|score| ~ 1)
SWEEP = (1, 10, 16, 20, 24, 32, 40, 48, 64)


def _chunks(n, pages=False):
    from rag.chunking import Chunk
    return [Chunk(text=f"t{r}", chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=(r % 10) if pages else None)
            for r in range(n)]


def _store(cfg, emb, pages=False):
    """VectorStore(cfg) over emb (cuda fp32 [n, d]), appended in pieces like an index build."""
    from rag.indexing import VectorStore
    store = VectorStore(cfg)
    n = emb.shape[0]
    chunks = _chunks(n, pages)
    for lo in range(0, n, 250_000):
        store.create_index(chunks[lo:lo + 250_000], emb[lo:lo + 250_000].contiguous(),
                           metadata_fields=["page_number"] if pages else None)
    return store


def _planted_queries(cuda, g, rows, nq):
    """half the queries planted near a row, half random (as test_refine_gpu.py), unit length"""
    import torch
    q = torch.randn((nq, rows.shape[1]), generator=g, device=cuda)
    j = torch.randint(0, rows.shape[0], (nq,), generator=g, device=cuda)
    q[0::2] = rows[j[0::2]] + 0.1 * q[0::2]
    return torch.nn.functional.normalize(q, dim=1).contiguous()


def _check_tally(ex, nq, what):
    counts = (ex["certified"], ex["escalated"], ex["unproven"])
    assert min(counts) >= 0 and sum(counts) == ex["queries"], f"{what}: counts do not add up: {ex}"
    if ex.get("mode", "certificate") == "certificate":
        assert ex["queries"] == nq, f"{what}: the tally does not describe this search of {nq} queries: {ex}"


def _check_claim(ex, wrong, nq, what):
    """store level: the queries whose ids differ from the oracle number at most `unproven` (none when all are claimed)"""
    _check_tally(ex, nq, what)
    if ex.get("mode", "certificate") == "certificate":
        assert len(wrong) <= ex["unproven"], f"{what}: {len(wrong)} lists differ from the oracle, {ex} -- e.g. {list(wrong.items())[:3]}"


# ---- 1. the certificate kernel, direct ----------------------------------------------------------------------------------------
def test_certificate_kernel_refuses_lists_that_do_not_cover_the_shard(cuda):
    """A candidate list proves nothing about the rows it does not hold: a -1 hole while the shard has more rows than the
    list, an id outside [id_base, id_base + n_rows), a small shard with a row missing -- status 1, and the escalation then
    returns the oracle's ids.  A small shard with every row in the list: status 0."""
    import torch
    from oracle import scan_ref
    from rag import _native as nat
    g = torch.Generator(device=cuda); g.manual_seed(41)
    base, k_in, k_out, nq = 1000, 16, 10, 6
    for n, case in ((40, "hole"), (40, "outside-high"), (40, "outside-low"), (12, "all-rows"), (12, "row-missing")):
        rows = torch.randn((n, D), generator=g, device=cuda)
        slab = torch.empty((n, nat.padded_dim(D)), dtype=torch.float16, device=cuda)
        shadow = torch.empty((n, D), dtype=torch.float32, device=cuda)
        row_err = torch.zeros(1, dtype=torch.float32, device=cuda)
        nat.slab_append_f32(rows, slab, 0, nat.SLAB_F16, shadow=shadow, row_err=row_err)
        q = torch.nn.functional.normalize(torch.randn((nq, D), generator=g, device=cuda), dim=1).contiguous()
        q16 = nat.queries_to_f16(q)
        cs, ci = nat.cosine_topk(q16, slab, n, D, k_in, id_base=base)
        torch.cuda.synchronize()
        if case == "hole":                   # one slot of each list emptied (its candidate left out)
            ci[:, 3] = -1; cs[:, 3] = float("-inf")
        elif case == "outside-high":         # one slot names a row past this shard
            ci[:, 5] = base + n + 7
        elif case == "outside-low":          # ... or before it (a row of the shard below)
            ci[:, k_in - 1] = base - 1
        elif case == "row-missing":          # n_rows <= k_in, but one of the n rows is not in the list
            ci[:, 2] = -1; cs[:, 2] = float("-inf")
            assert int((ci[0] >= 0).sum()) == n - 1
        else:
            assert int((ci[0] >= 0).sum()) == n          # every row of the shard fetched
        ci, cs = ci.contiguous(), cs.contiguous()
        ws = torch.empty(nat.exact_workspace_bytes(nq), dtype=torch.uint8, device=cuda)
        s, i, st = nat.refine_f32_cert(q, q16, shadow, n, base, ci, cs, k_out, float(row_err.item()), nat.SLAB_F16, ws)
        st0 = st.cpu().numpy().copy()
        nat.escalate_exact(q, q16, slab, shadow, n, base, k_out, s, i, st, ws)
        torch.cuda.synchronize()
        want = 0 if case == "all-rows" else 1
        assert (st0 == want).all(), f"{case}: certificate status {st0.tolist()}, expected {want} for every query"
        assert set(np.unique(st.cpu().numpy())) <= {0, 1}, case
        q_h, rows_h = q.cpu().numpy(), shadow.cpu().numpy()
        ref = scan_ref.cosine_topk_ref(q_h, rows_h, k_out)
        assert_topk(s.cpu().numpy(), i.cpu().numpy() - base, q_h, rows_h, k_out, f"{case} after escalation", ref=ref)


# ---- 2. the store over every top_k, fp16 ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def f16_1m(cuda):
    """1 M x 384 random rows in a default-config store, 64 queries (half planted), the oracle's top-64 over the shadow."""
    import torch
    from types import SimpleNamespace
    from oracle import scan_ref
    g = torch.Generator(device=cuda); g.manual_seed(2024)
    n, nq = 1_000_000, 64
    store = _store({"collection_name": "sweep"}, torch.randn((n, D), generator=g, device=cuda))
    rows = store.collection.shadow[:n]
    q = _planted_queries(cuda, g, rows, nq)
    q_h, rows_h = q.cpu().numpy(), rows.cpu().numpy()
    return SimpleNamespace(store=store, n=n, q=q_h, rows=rows_h, ref=scan_ref.cosine_topk_ref(q_h, rows_h, max(SWEEP)))


def test_store_sweep_over_top_k_fp16(f16_1m):
    from rag import _native as nat
    st = f16_1m
    nq = st.q.shape[0]
    frac = {}
    for k in SWEEP:
        s, i = st.store.search_rows(st.q, k)
        ex = dict(st.store.last_exactness)
        rs, ri = st.ref[0][:, :k], st.ref[1][:, :k]
        wrong = topk_errors(i, st.q, st.rows, ri, k, TOL)
        _check_claim(ex, wrong, nq, f"top_k {k}")
        assert ex["unproven"] == 0, f"top_k {k}: {ex}"
        assert_topk(s, i, st.q, st.rows, k, f"top_k {k}", ref=(rs, ri))
        frac[k] = ex["certified"] / nq
        print(f"top_k {k}: k' {nat.overfetch(nq, k, st.store.refine_overfetch, st.n)} certified {frac[k]:.3f} "
              f"escalated {ex['escalated']}")
    low = {k: f for k, f in frac.items() if k <= 32 and f < 0.9}
    assert not low, f"certified fraction per top_k (>= 0.9 wanted up to 32): {frac}"


# ---- 3. near-tie bands at large top_k ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "int8"])
def test_near_tie_bands_at_large_top_k_are_escalated(cuda, dtype):
    """2 x top_k rows within ~1e-4 cosine of a centre (near-duplicate chunks) for top_k 20 and 40: no over-fetch holds the
    band, so the certificate must refuse every such query and the escalation must return the oracle's fp32 ids."""
    import torch
    from oracle import scan_ref
    g = torch.Generator(device=cuda); g.manual_seed(5 if dtype == "fp16" else 6)
    n, per = 200_000, 4
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    centres = torch.nn.functional.normalize(torch.randn((2 * per, D), generator=g, device=cuda), dim=1)
    pos = torch.randperm(n, generator=g, device=cuda)
    at = 0
    for c, k in enumerate([20] * per + [40] * per):
        rows[pos[at:at + 2 * k]] = centres[c] + 1e-4 * torch.randn((2 * k, D), generator=g, device=cuda)
        at += 2 * k
    cfg = {"collection_name": f"band-{dtype}"} if dtype == "fp16" else {"collection_name": "band-int8", "index_dtype": "int8",
                                                                        "refine_exact": True}
    store = _store(cfg, rows)
    rows_h = store.collection.shadow[:n].cpu().numpy()
    q = torch.nn.functional.normalize(centres + 1e-5 * torch.randn(centres.shape, generator=g, device=cuda), dim=1)
    q_h = q.cpu().numpy()
    for lo, k in ((0, 20), (per, 40)):
        qk = q_h[lo:lo + per]
        s, i = store.search_rows(qk, k)
        ex = dict(store.last_exactness)
        _check_tally(ex, per, f"{dtype} top_k {k}")
        assert ex["escalated"] == per and ex["certified"] == 0 and ex["unproven"] == 0, f"{dtype} top_k {k}: {ex}"
        ref = scan_ref.cosine_topk_ref(qk, rows_h, k)
        assert_topk(s, i, qk, rows_h, k, f"{dtype} band top_k {k}", tol=BAND_TOL, ref=ref)


# ---- 4. int8 under refine_exact 'auto' -----------------------------------------------------------------------------------------
def test_int8_auto_claims_hold_and_the_rerank_has_a_margin(cuda):
    """int8 slabs stay empirical under 'auto' (no escalation): a query left unproven may differ from the oracle, a
    certified one may not -- per query through the kernels (status array), by the counts through the store.  And the
    re-rank must have candidates to re-rank: k' > top_k."""
    import torch
    from oracle import scan_ref
    from rag import _native as nat
    g = torch.Generator(device=cuda); g.manual_seed(88)
    n, nq = 500_000, 64
    store = _store({"collection_name": "i8auto", "index_dtype": "int8"}, torch.randn((n, D), generator=g, device=cuda))
    assert store.refine_exact == "auto"
    sh = store.collection.shards[0]
    rows = sh.shadow[:n]
    q = _planted_queries(cuda, g, rows, nq)
    q_h, rows_h = q.cpu().numpy(), rows.cpu().numpy()
    ref = scan_ref.cosine_topk_ref(q_h, rows_h, 20)
    kps = {}
    for k in (10, 20):
        ri = ref[1][:, :k]
        _, i = store.search_rows(q_h, k)
        ex = dict(store.last_exactness)
        _check_claim(ex, topk_errors(i, q_h, rows_h, ri, k, TOL), nq, f"int8 store top_k {k}")
        kp = kps[k] = nat.overfetch(nq, k, store.refine_overfetch, n, nat.SLAB_I8)
        q16 = nat.queries_to_f16(q, nat.SLAB_I8)
        cs, ci = nat.cosine_topk(q16, sh.slab, n, D, kp, slab_type=nat.SLAB_I8, scales=sh.scales)
        ws = torch.empty(nat.exact_workspace_bytes(nq), dtype=torch.uint8, device=cuda)
        s, i, st = nat.refine_f32_cert(q, q16, sh.shadow, n, 0, ci, cs, k, sh.row_err_max(), nat.SLAB_I8, ws)
        torch.cuda.synchronize()
        st, i = st.cpu().numpy(), i.cpu().numpy()
        proven = np.nonzero(st == 0)[0]
        wrong = topk_errors(i[proven], q_h[proven], rows_h, ri[proven], k, TOL)
        assert not wrong, f"int8 top_k {k}: certified queries differ from the oracle: {wrong}"
    assert all(kp > k for k, kp in kps.items()), f"int8 over-fetch per top_k: {kps} (k' == top_k only reorders the slab's list)"


# ---- 5 / 6. top_k above the scan kernels, filtered search ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def f16_300k(cuda):
    """300 k x 384 rows (metadata page_number = row % 10) with a band of 300 near-identical rows; queries 0 and 1 sit on it."""
    import torch
    from types import SimpleNamespace
    g = torch.Generator(device=cuda); g.manual_seed(300)
    n, nq = 300_000, 16
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    centre = torch.nn.functional.normalize(torch.randn((1, D), generator=g, device=cuda), dim=1)
    band = torch.randperm(n, generator=g, device=cuda)[:300]
    rows[band] = centre + 2e-4 * torch.randn((300, D), generator=g, device=cuda)
    store = _store({"collection_name": "large"}, rows, pages=True)
    sh_rows = store.collection.shadow[:n]
    q = _planted_queries(cuda, g, sh_rows, nq)
    q[:2] = torch.nn.functional.normalize(centre + 1e-5 * torch.randn((2, D), generator=g, device=cuda), dim=1)
    return SimpleNamespace(store=store, n=n, q=q.cpu().numpy(), rows=sh_rows.cpu().numpy(), band=band.cpu().numpy())


def test_top_k_above_64_reports_what_it_proves(f16_300k, cuda):
    from oracle import scan_ref
    from rag.indexing import VectorStore
    st = f16_300k
    store, q_h, rows_h = st.store, st.q, st.rows
    nq = q_h.shape[0]
    ref = scan_ref.cosine_topk_ref(q_h, rows_h, 200)
    for k in (65, 100, 200):
        store.search_rows(q_h[:5], 10)                 # a certified search first: its counts must not survive the next one
        assert store.last_exactness["queries"] == 5
        _, i = store.search_rows(q_h, k)
        ex = dict(store.last_exactness)
        assert ex["queries"] in (0, nq), f"top_k {k}: last_exactness still describes the previous search: {ex}"
        _check_tally(ex, nq, f"top_k {k}")
        wrong = topk_errors(i, q_h, rows_h, ref[1][:, :k], k, BAND_TOL)
        assert len(wrong) <= ex["unproven"] or ex.get("mode", "certificate") != "certificate", \
            f"top_k {k}: {len(wrong)} lists differ from the oracle, tally {ex}: {list(wrong.items())[:3]}"
    # a store without the fp32 shadow certifies nothing, and says so after each of its searches
    plain = VectorStore({"collection_name": "plain", "refine_fp32": False})
    plain.create_index(_chunks(5000), rows_h[:5000])
    store.search_rows(q_h, 10)
    plain.last_exactness = dict(store.last_exactness)    # the refined search's tally, as a caller holding one dict would see it
    plain.search_rows(q_h, 10)
    ex = plain.last_exactness
    assert ex["certified"] == 0 and ex["escalated"] == 0, f"a store without fp32 rows claims exactness: {ex}"
    _check_tally(ex, nq, "refine_fp32=False")


def test_filtered_search_keeps_the_claim(f16_300k):
    """where = page_number < 3 (30 % of the rows, a third of the band): the oracle runs on the allowed fp32 rows only."""
    from oracle import scan_ref
    st = f16_300k
    store, q_h, rows_h = st.store, st.q, st.rows
    nq, k = q_h.shape[0], 20
    allowed = np.nonzero(np.arange(st.n) % 10 < 3)[0]
    res = store.search_batch(q_h, top_k=k, where={"page_number": {"$lt": 3}})
    ex = dict(store.last_exactness)
    got = np.array([[int(c.split("_")[1]) for c in row] for row in res["ids"]])
    got_s = np.array([[1.0 - x for x in row] for row in res["distances"]], dtype=np.float32)
    assert np.isin(got, allowed).all(), "a filtered search returned a row the filter excludes"
    sub = rows_h[allowed]
    rs, ri = scan_ref.cosine_topk_ref(q_h, sub, k)
    local = np.searchsorted(allowed, got)
    wrong = topk_errors(local, q_h, sub, ri, k, BAND_TOL)
    _check_claim(ex, wrong, nq, "filtered top_k 20")
    assert ex["unproven"] == 0 and ex["escalated"] >= 2, f"the band queries must be escalated: {ex}"
    assert_topk(got_s, local, q_h, sub, k, "filtered", tol=BAND_TOL, ref=(rs, ri))


# ---- 7. the engine path (retrieve_batch with >= batch_queries questions) -------------------------------------------------------
WORDS = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine "
         "similarity vector index chunk context answer question compression memory latency throughput").split()


def _pipeline(seed, dtype="fp16"):
    """RAGPipeline on the synthetic MiniLM encoder with the reference's retrieval defaults (rerank on: top_k 10 -> fetch 20),
    nothing indexed yet."""
    from rag import RAGPipeline

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    cfg = {"embedding": {"model_name": "synthetic:minilm", "device": "cuda", "batch_size": 64, "normalize": True},
           "retrieval": {"top_k": 10, "similarity_threshold": 0.0, "rerank": True, "diversity_penalty": 0.0, "batch_queries": 64},
           "vector_store": {"collection_name": f"engine{seed}", "index_dtype": dtype}}
    p = RAGPipeline(cfg)
    p.setup(Stub())
    return p


def _index(cuda, p, n, seed, plant=None):
    """n random rows into p's store; plant = (vector, copies): that many copies of one vector at random rows (returned, sorted)."""
    import torch
    g = torch.Generator(device=cuda); g.manual_seed(seed)
    emb = torch.randn((n, D), generator=g, device=cuda)
    pos = None
    if plant is not None:
        vec, copies = plant
        pos = torch.randperm(n, generator=g, device=cuda)[:copies]
        emb[pos] = torch.as_tensor(vec, device=cuda)
        pos = np.sort(pos.cpu().numpy())
    p.vector_store.create_index(_chunks(n), emb)
    return pos


def _questions(n, seed):
    rng = np.random.default_rng(seed)
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 9)))) + f" {q}" for q in range(n)]


def _engine_lists(p, questions, fetch):
    r = p.retriever
    hits = [h for piece in r._search_many(questions, fetch) for h in piece]
    assert r._engine is not None, "this store / encoder pair should take the engine"
    assert len(hits) == len(questions)
    return np.stack([h[0] for h in hits]), np.stack([h[1] for h in hits])


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
def test_engine_path_lists_match_the_oracle(cuda, dtype):
    """fp16: every list proven (escalated where needed); int8 under 'auto': no escalation, an unproven list may differ."""
    from oracle import scan_ref
    p = _pipeline(71, dtype)
    _index(cuda, p, 200_000, 71)
    store = p.vector_store
    questions = _questions(160, 3)
    fetch = 20
    s, i = _engine_lists(p, questions, fetch)
    ex = dict(store.last_exactness)
    q_h = p.embedding_model.embed(questions)
    rows_h = store.collection.shadow[:200_000].cpu().numpy()
    rs, ri = scan_ref.cosine_topk_ref(q_h, rows_h, fetch)
    wrong = topk_errors(i, q_h, rows_h, ri, fetch, 1e-3)     # the batched encoder rounds the questions differently
    _check_claim(ex, wrong, len(questions), f"engine {dtype}, fetch 20")
    if dtype == "fp16":
        assert ex["unproven"] == 0, ex
        assert np.abs(s - rs).max() < 1e-3


def test_engine_path_retries_an_escalation_list_overflow(cuda):
    """More than EXACT_CAP copies of one question's own embedding: the engine's escalation list overflows (status 2); the
    question must come back proven, with search_batch's list (the lowest rows of the copies: exact ties)."""
    from rag import _native as nat
    questions = _questions(96, 5)
    p = _pipeline(73)
    e0 = p.embedding_model.embed([questions[0]])[0]
    pos = _index(cuda, p, 200_000, 73, plant=(e0, nat.EXACT_CAP + 100))
    store = p.vector_store
    fetch = 20
    s, i = _engine_lists(p, questions, fetch)
    ex = dict(store.last_exactness)
    _check_tally(ex, len(questions), "engine with an overflowing band")
    assert ex["unproven"] == 0, f"an escalation-list overflow was left unproven on the engine path: {ex}"
    assert np.array_equal(i[0], pos[:fetch]), "the overflowing query's list is not the lowest rows of the copies"
    _, ref_i = store.search_rows(p.embedding_model.embed([questions[0]]), fetch)
    assert np.array_equal(i[0], ref_i[0])
