"""GPU: the lexical re-rank kernel (csrc/rerank.hip, crs::rerank_lexical) against the pure-Python restatement of the host rule in
tests/_rerank_ref.py, and the retriever's opt-in lexical_rerank: 'device' path end to end.

The rule is fp64 arithmetic on integers and fp32 scores, each operation rounded on its own, so there is no tolerance: order, count
and reranked must be equal and sim / rr bit-equal (compared as int64 words)."""
import numpy as np
import pytest

import _rerank_ref as ref

pytestmark = pytest.mark.gpu

N_ROWS, NQ = 2048, 128
SHAPES = [(2, 1), (7, 3), (20, 10), (40, 20), (64, 32), (64, 64), (20, 20)]


@pytest.fixture(scope="module")
def corpus():
    """The 2048 documents, and their token CSR as the product builds it."""
    from rag.indexing import _TokenCSR
    docs = ref.make_documents(N_ROWS, seed=3)
    csr = _TokenCSR()
    csr.extend(docs)
    return docs, csr


def _run(cuda, csr, n_rows, scores, rows, queries, k, threshold, doc_off=None, doc_tok=None):
    """The lists as numpy -> the kernel's five outputs as numpy.  doc_off / doc_tok: cuda tensors the caller holds (views)."""
    import torch
    from rag import _native as nat
    if doc_off is None:
        doc_off, doc_tok = torch.from_numpy(csr.offsets.copy()).to(cuda), torch.from_numpy(csr.token_ids.copy()).to(cuda)
    q_ids, q_norm = zip(*(csr.query_ids(q) for q in queries))
    q_off = np.zeros(len(queries) + 1, dtype=np.int64)
    np.cumsum([len(i) for i in q_ids], out=q_off[1:])
    q_tok = np.array([t for ids in q_ids for t in ids], dtype=np.int32)
    out = nat.rerank_lexical(torch.from_numpy(scores).to(cuda), torch.from_numpy(rows).to(cuda), doc_off, doc_tok, n_rows,
                             torch.from_numpy(q_off).to(cuda), torch.from_numpy(q_tok).to(cuda),
                             torch.from_numpy(np.asarray(q_norm, dtype=np.int32)).to(cuda), k, threshold)
    torch.cuda.synchronize()
    return dict(zip(("order", "count", "sim", "rr", "reranked"), (t.cpu().numpy() for t in out)))


def _assert_equal(got, want, what):
    for name in ("order", "count", "reranked"):
        assert got[name].dtype == np.int32 and got[name].shape == want[name].shape, (what, name)
        bad = np.argwhere(got[name] != want[name])
        assert bad.size == 0, f"{what}: {name} differs first at {bad[0].tolist()}: {got[name][tuple(bad[0])]} != {want[name][tuple(bad[0])]}"
    for name in ("sim", "rr"):
        assert got[name].dtype == np.float64 and got[name].shape == want[name].shape, (what, name)
        bad = np.argwhere(got[name].view(np.int64) != want[name].view(np.int64))
        assert bad.size == 0, (f"{what}: {name} differs in its bits first at {bad[0].tolist()}: {got[name][tuple(bad[0])]!r} != "
                               f"{want[name][tuple(bad[0])]!r}")


def _check(cuda, corpus, scores, rows, queries, k, threshold, what, n_rows=N_ROWS, texts=None, **views):
    docs, csr = corpus
    got = _run(cuda, csr, n_rows, scores, rows, queries, k, threshold, **views)
    want = ref.rerank_ref_batch(scores, rows, docs[:n_rows] if texts is None else texts, queries, k, threshold)
    _assert_equal(got, want, what)
    return got, want


@pytest.mark.parametrize("m_max,k", SHAPES, ids=lambda v: str(v))
def test_op_equals_the_host_rule(cuda, corpus, m_max, k):
    scores, rows, queries = ref.make_lists(NQ, m_max, k, N_ROWS, seed=100 * m_max + k)
    lengths = (rows >= 0).sum(1)
    assert {0, 1, min(k, m_max), min(k + 1, m_max), m_max} <= set(lengths.tolist())
    got, want = _check(cuda, corpus, scores, rows, queries, k, 0.0, f"m_max {m_max} k {k}")
    if m_max > k:
        assert want["reranked"].sum() >= NQ // 8 and (want["reranked"] == 0).sum() >= 3
        moved = sum(want["order"][i, :k].tolist() != sorted(want["order"][i, :k].tolist()) for i in np.flatnonzero(want["reranked"]))
        assert moved >= 1 or m_max == 2, "no list was re-ordered by the lexical term"
    else:
        assert want["reranked"].sum() == 0


def test_exact_ties_keep_list_order_and_runs_repeat(cuda, corpus):
    docs, csr = corpus
    m_max, k = 20, 10
    scores, rows, queries = ref.make_lists(NQ, m_max, k, N_ROWS, seed=5)
    rng = np.random.default_rng(6)
    for i in range(NQ):
        n = int((rows[i] >= 0).sum())
        if n:
            # two score values only, and the candidates are ONE row repeated in runs: equal scores and equal hits, over and over
            scores[i, :n] = np.sort(rng.choice(np.array([0.75, 0.5], dtype=np.float32), size=n))[::-1]
            rows[i, :n] = np.repeat(rows[i, :(n + 3) // 4], 4)[:n]
    got, want = _check(cuda, corpus, scores, rows, queries, k, 0.0, "ties")
    tied = 0
    for i in np.flatnonzero(want["reranked"]):
        rr = want["rr"][i][want["order"][i, :k]]
        tied += int((np.diff(rr) == 0).any())
    assert tied >= NQ // 8, "the case holds no exact ties"
    again = _run(cuda, csr, N_ROWS, scores, rows, queries, k, 0.0)
    for name in got:
        assert got[name].tobytes() == again[name].tobytes(), name


def test_threshold_leaves_k_and_k_plus_one_survivors(cuda, corpus):
    m_max, k = 20, 10
    scores, rows, queries = ref.make_lists(NQ, m_max, k, N_ROWS, seed=8)
    rng = np.random.default_rng(9)
    threshold = ref.similarity(float(np.float32(1.0) - np.float32(0.5)))          # the score of cosine 0.5: 0.875
    for i in range(NQ):
        above = (k, k + 1, k - 1, m_max)[i % 4]
        scores[i] = np.sort(np.concatenate([rng.uniform(0.5, 0.9, size=above), rng.uniform(0.1, 0.49, size=m_max - above)]).astype(np.float32))[::-1]
        scores[i, above - 1] = 0.5                                                # sim == threshold exactly: kept
        rows[i] = rng.choice(N_ROWS, size=m_max, replace=False)
    got, want = _check(cuda, corpus, scores, rows, queries, k, threshold, "threshold")
    assert set(want["count"].tolist()) == {k - 1, k}
    assert want["reranked"].tolist() == [int(i % 4 in (1, 3)) for i in range(NQ)]


def test_clamps_nan_and_odd_queries(cuda, corpus):
    docs, csr = corpus
    m_max, k = 20, 10
    scores, rows, queries = ref.make_lists(NQ, m_max, k, N_ROWS, seed=12)
    full = np.flatnonzero((rows >= 0).sum(1) == m_max)
    assert full.size >= 4
    a, b, c, d = full[:4].tolist()
    scores[a, :4] = (1.5, 1.0000001, 1.0, 0.99999994)                   # above 1: distance below 0, clamped; sim 1
    scores[a, -3:] = (-0.99999994, -1.0000001, -1.5)                    # below -1: distance above 2, clamped; sim 0
    scores[b, 2], scores[b, 7] = np.nan, np.nan                         # a NaN score drops, whatever the threshold
    queries[c] = "   "                                                  # no words: norm 1, no hits
    queries[d] = "nothing known here"                                   # only words no document holds: norm 3, no hits
    for threshold in (0.0, -1.0):
        got, want = _check(cuda, corpus, scores, rows, queries, k, threshold, f"edge cases, threshold {threshold}")
        assert np.isnan(want["sim"][b, 2]) and 2 not in want["order"][b].tolist() and 7 not in want["order"][b].tolist()
        assert want["sim"][a, 0] == 1.0 and want["sim"][a, -1] == 0.0
        assert want["reranked"][c] == 1 and want["order"][c, :k].tolist() == list(range(k))     # no lexical term: the score order stays
        assert want["reranked"][d] == 1 and want["order"][d, :k].tolist() == list(range(k))
    # every candidate of a list under the threshold
    got, want = _check(cuda, corpus, scores, rows, queries, k, 2.0, "nothing passes")
    assert want["count"].sum() == 0 and (want["order"] == -1).all()


def test_long_queries_and_long_documents(cuda):
    """A query of 200 distinct words (more than one staged round of query ids) and a document of 5000 tokens (searched, not
    walked), against short ones: both counting strategies, on both sides of the choice between them."""
    from rag.indexing import _TokenCSR
    rng = np.random.default_rng(15)
    vocab = [f"t{j}" for j in range(6000)]
    docs = ref.make_documents(256, seed=16)
    docs[10] = " ".join(vocab[:5000])                                   # 5000 distinct tokens
    docs[11] = " ".join(rng.permutation(vocab)[:700])
    docs[12] = " ".join(vocab[4990:5100]) + " " + docs[12]
    csr = _TokenCSR()
    csr.extend(docs)
    assert csr.row(10).size == 5000
    m_max, k, nq = 12, 4, 16
    rows = np.stack([np.concatenate([[10, 11, 12], rng.choice(np.arange(13, 256), size=m_max - 3, replace=False)]) for _ in range(nq)]).astype(np.int64)
    for i in range(nq):
        rng.shuffle(rows[i])
    scores = np.sort(rng.uniform(0.3, 0.9, size=(nq, m_max)).astype(np.float32), axis=1)[:, ::-1].copy()
    queries = []
    for i in range(nq):
        if i % 4 == 0:      # 200 distinct words: tokens of the long documents, pool words, unknown words
            words = list(rng.permutation(vocab[:5200])[:150]) + ref.POOL + [f"unknown{j}" for j in range(26)]
            assert len(set(words)) == 200
        elif i % 4 == 1:    # 129 known ids: one past a staged round
            words = list(rng.permutation(vocab[:5000])[:129])
        elif i % 4 == 2:
            words = [vocab[4995], vocab[5050], "retrieval", vocab[3]]
        else:
            words = list(rng.choice(ref.POOL, size=5))
        queries.append(" ".join(rng.permutation(words)))
    got = _run(cuda, csr, len(docs), scores, rows, queries, k, 0.0)
    want = ref.rerank_ref_batch(scores, rows, docs, queries, k, 0.0)
    _assert_equal(got, want, "long query / long document")
    assert want["reranked"].all()


def test_rows_outside_the_collection_are_never_dereferenced(cuda):
    """The CSR handed to the kernel is a view into a larger allocation that goes on with 16 more rows' offsets and tokens (rows
    holding every query word), and n_rows stops short of them: a row id the kernel failed to refuse reads those -- more hits, a
    wrong answer here, not a fault."""
    import torch
    from rag.indexing import _TokenCSR
    n_rows, extra = 500, 16
    m_max, k = 20, 10
    scores, rows, queries = ref.make_lists(NQ, m_max, k, n_rows, seed=20)
    docs = ref.make_documents(n_rows, seed=21) + [" ".join(ref.POOL + [f"u{r}" for r in range(0, n_rows, 9)])] * extra
    csr = _TokenCSR()
    csr.extend(docs)
    rng = np.random.default_rng(22)
    poisoned = 0
    for i in range(NQ):
        n = int((rows[i] >= 0).sum())
        if n >= 4:
            at = rng.choice(n, size=3, replace=False)
            for p, bad in zip(at, (-1, n_rows, n_rows + 3)):
                rows[i, p] = bad
            poisoned += 1
    assert poisoned >= NQ // 2
    off_all, tok_all = torch.from_numpy(csr.offsets.copy()).to(cuda), torch.from_numpy(csr.token_ids.copy()).to(cuda)
    off, tok = off_all[: n_rows + 1], tok_all            # the offsets stop at n_rows; the 16 rows' tokens stay reachable
    got = _run(cuda, csr, n_rows, scores, rows, queries, k, 0.0, doc_off=off, doc_tok=tok)
    want = ref.rerank_ref_batch(scores, rows, docs[:n_rows], queries, k, 0.0)      # rows >= n_rows: candidates without text
    _assert_equal(got, want, "poisoned rows")
    would = ref.rerank_ref_batch(scores, rows, docs, queries, k, 0.0)              # what a missed check would compute
    assert (would["rr"] != want["rr"]).any()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
WORDS = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine "
         "similarity vector index chunk context answer question compression memory latency throughput").split()
E2E_ROWS, E2E_DIM, E2E_Q = 4096, 384, 128


def _pipeline(cuda, name, store_cfg=None):
    import torch
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    cfg = {"embedding": {"model_name": "synthetic:minilm", "device": "cuda", "batch_size": 64, "normalize": True},
           "retrieval": {"top_k": 10, "similarity_threshold": 0.0, "rerank": True, "diversity_penalty": 0.0, "batch_queries": 64,
                         "lexical_rerank": "device"},
           "vector_store": dict({"collection_name": name}, **(store_cfg or {}))}
    p = RAGPipeline(cfg)
    p.setup(Stub())
    rng = np.random.default_rng(21)
    chunks = [Chunk(text=" ".join(rng.choice(WORDS, size=6)) + f" {r}", chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=None)
              for r in range(E2E_ROWS)]
    g = torch.Generator(device=cuda); g.manual_seed(22)
    centres = torch.randn((E2E_ROWS // 8, E2E_DIM), generator=g, device=cuda).repeat_interleave(8, dim=0)
    emb = centres + 0.3 * torch.randn((E2E_ROWS, E2E_DIM), generator=g, device=cuda)
    p.vector_store.create_index(chunks[:3000], emb[:3000])
    p.vector_store.create_index(chunks[3000:], emb[3000:])
    questions = [" ".join(rng.choice(WORDS, size=int(rng.integers(4, 9)))) + f" {q}" for q in range(E2E_Q)]
    return p, questions


@pytest.fixture(scope="module")
def e2e(cuda):
    return _pipeline(cuda, "rerank-e2e")


def _both(p, questions, top_k=None):
    r = p.retriever
    out = {}
    for mode in ("host", "device"):
        r.lexical_rerank = mode
        out[mode] = (p.retrieve_batch(questions, top_k=top_k), dict(r.last_rerank))
    r.lexical_rerank = "device"
    return out


def _assert_device_equals_host(both, lists=E2E_Q):
    (host, host_info), (dev, dev_info) = both["host"], both["device"]
    assert host_info == {"mode": "host", "lists": lists}, host_info
    assert dev_info == {"mode": "device", "lists": lists}, dev_info
    for a in range(len(host)):
        assert dev[a] == host[a], f"query {a}: {[c['chunk_id'] for c in dev[a]]} != {[c['chunk_id'] for c in host[a]]}"
    assert dev == host
    return host


@pytest.mark.parametrize("top_k", [10, 32])
def test_retrieve_batch_on_device_equals_host(cuda, e2e, top_k):
    p, questions = e2e
    host = _assert_device_equals_host(_both(p, questions, top_k=top_k))
    assert all(len(c) == top_k and "rerank_score" in c[0] for c in host)
    assert sum([c["score"] for c in chunks] != sorted((c["score"] for c in chunks), reverse=True) for chunks in host) >= E2E_Q // 4, \
        "the lexical term re-ordered hardly any list"


def test_retrieve_batch_with_a_threshold_at_the_median_score(cuda, e2e):
    p, questions = e2e
    r = p.retriever
    r.lexical_rerank = "host"
    first = p.retrieve_batch(questions)
    r.lexical_rerank = "device"
    r.similarity_threshold = float(np.median([c["score"] for chunks in first for c in chunks]))
    try:
        host = _assert_device_equals_host(_both(p, questions))
        sizes = [len(c) for c in host]
        assert min(sizes) < 10 and sum("rerank_score" not in c[0] for c in host if c) >= 8, sizes
    finally:
        r.similarity_threshold = 0.0


def test_retrieve_batch_with_the_mmr_step_on_the_device_behind_it(cuda, e2e):
    p, questions = e2e
    r = p.retriever
    r.diversity_penalty, r.mmr_vectors = 0.1, "device"
    try:
        _assert_device_equals_host(_both(p, questions))
        assert r.last_mmr["mode"] == "device"
    finally:
        r.diversity_penalty, r.mmr_vectors = 0.0, "auto"


def test_lists_of_80_take_the_host_path(cuda, e2e):
    p, questions = e2e
    both = _both(p, questions[:64], top_k=40)
    assert both["device"][1] == {"mode": "host", "lists": 64}
    assert both["device"][0] == both["host"][0] and all(len(c) == 40 for c in both["host"][0])


def test_retrieve_equals_retrieve_batch_of_one(cuda, e2e):
    p, questions = e2e
    for q in (questions[3], questions[77]):
        assert p.retrieve(q) == p.retrieve_batch([q])[0]
        assert p.retriever.last_rerank == {"mode": "device", "lists": 1}


def test_device_follows_update_and_delete(cuda):
    p, questions = _pipeline(cuda, "rerank-mutate")
    store = p.vector_store
    before = _assert_device_equals_host(_both(p, questions))
    # one chunk gains every word of question 0: its lexical term becomes 1
    target = before[0][-1]["chunk_id"]
    store.update(ids=[target], documents=[questions[0] + " and more"])
    after = _assert_device_equals_host(_both(p, questions))
    hit = [c for c in after[0] if c["chunk_id"] == target]
    assert hit and hit[0]["text"] == questions[0] + " and more"
    assert hit[0]["rerank_score"] == hit[0]["score"] * 0.7 + 1.0 * 0.3
    assert after[0][0]["chunk_id"] == target or after[0][0]["rerank_score"] >= hit[0]["rerank_score"]
    # rows renumbered by a delete
    gone = [after[5][0]["chunk_id"], "c_7", "c_2000"]
    assert store.delete(ids=gone) == len(set(gone))
    last = _assert_device_equals_host(_both(p, questions))
    assert all(c["chunk_id"] not in gone for chunks in last for c in chunks)


def test_two_shards_on_one_card(cuda):
    """A layout whose rows are not the sidecar rows: two shards (the second with a row map), lists merged across them."""
    p, questions = _pipeline(cuda, "rerank-two", {"devices": ["cuda:0", "cuda:0"]})
    assert len(p.vector_store.collection.shards) == 2 and not p.vector_store.collection.shards[1].identity
    _assert_device_equals_host(_both(p, questions))
