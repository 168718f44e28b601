"""CPU: hybrid retrieval without a device.  The token CSR's BM25 statistics (tfs, doc_len, df, total_len) equal collections.Counter
on the raw documents, are extended and dropped with the CSR, and leave its offsets / ids / vocabulary as they were; the three C
entry points (crs_bm25_topk, crs_bm25_workspace_bytes, crs_fuse_rrf) are declared, exported and bound with the ABI version
unmoved, their argument checks answer CRS_EINVAL before any HIP call and their kernels use no scratch; VectorStore.bm25_rows cuts
a batch at 64 queries and at the pair cap and refuses one query over the cap; the fp32 reference of the GPU tests
(tests/_bm25_ref.py) agrees with an independent fp64 textbook BM25 within the rounding bound; the retriever validates `hybrid`,
builds the documented dicts from a hybrid retrieve_batch, and never calls bm25_rows with hybrid off."""
import ctypes
import os
import random
import re
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import _bm25_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the statistics beside the token CSR ---------------------------------------------------------------------------------------------
def _random_docs(n, seed=3):
    rng = random.Random(seed)
    words = [f"tok{i}" for i in range(300)] + ["Mixed", "mixed", "MIXED", "Straße", "tab\tbed"]
    docs = []
    for r in range(n):
        if r % 17 == 5:
            docs.append("" if r % 2 else "  \n ")
            continue
        picked = [rng.choice(words) for _ in range(rng.randint(1, 40))]
        picked += [picked[0]] * rng.randint(0, 4)                      # repeated words: tf > 1
        docs.append(" ".join(w.upper() if rng.random() < 0.2 else w for w in picked))
    docs[n // 2] = " ".join(rng.choice(words) for _ in range(5000))    # one long document
    return docs


def _collection(docs):
    from rag.indexing import SlabCollection
    col = SlabCollection("bm25", "fp16", False, ["cpu"])
    _add(col, docs)
    return col


def _add(col, docs):
    start = len(col.ids)
    col.ids.extend(f"c{start + i}" for i in range(len(docs)))
    col.documents.extend(docs)
    col.metadatas.extend({} for _ in docs)


def _assert_stats_are(csr, docs):
    word_of = {i: w for w, i in csr.vocab.items()}
    counts = [Counter(d.lower().split()) for d in docs]
    assert csr.rows == len(docs)
    assert csr.tfs.dtype == np.int32 and csr.tfs.shape == csr.token_ids.shape
    assert csr.doc_len.dtype == np.int32 and csr.doc_len.shape == (len(docs),)
    assert csr.df.dtype == np.int64 and csr.df.shape == (len(csr.vocab),)
    for r, c in enumerate(counts):
        lo, hi = csr.offsets[r], csr.offsets[r + 1]
        assert {word_of[t]: tf for t, tf in zip(csr.token_ids[lo:hi].tolist(), csr.tfs[lo:hi].tolist())} == dict(c), f"row {r}"
        assert csr.doc_len[r] == sum(c.values()) == len(docs[r].lower().split())
    df = Counter(w for c in counts for w in c)
    assert {word_of[t]: int(n) for t, n in enumerate(csr.df.tolist())} == dict(df)
    assert csr.total_len == sum(sum(c.values()) for c in counts) == int(csr.doc_len.sum())


def test_statistics_equal_counter_on_the_raw_documents():
    docs = _random_docs(300)
    col = _collection(docs)
    csr = col._token_csr()
    _assert_stats_are(csr, docs)
    assert csr.tfs.max() > 1 and csr.doc_len.max() >= 5000 and (csr.doc_len == 0).sum() >= 10
    tf, dl = csr.device_stats("cpu")
    assert (tf.numpy() == csr.tfs).all() and (dl.numpy() == csr.doc_len).all()


def test_statistics_are_extended_by_a_second_extend_and_the_mirror_gets_the_tail():
    docs = _random_docs(300)
    col = _collection(docs[:120])
    csr = col._token_csr()
    _assert_stats_are(csr, docs[:120])
    csr.device_stats("cpu")
    first_rows, first_total = csr._dev_st_rows, csr._dev_st_total
    assert (first_rows, first_total) == (120, csr.total)
    _add(col, docs[120:])
    assert col._token_csr() is csr
    _assert_stats_are(csr, docs)
    tf, dl = csr.device_stats("cpu")
    assert csr._dev_st_rows == 300 and csr._dev_st_total == csr.total > first_total
    assert (tf.numpy() == csr.tfs).all() and (dl.numpy() == csr.doc_len).all()
    _add(col, ["one more row row"])                                    # fits the capacity the growth left: the same allocation
    mirror = csr._dev_st
    tf, dl = col._token_csr().device_stats("cpu")
    assert csr._dev_st is mirror and (tf.numpy() == csr.tfs).all() and (dl.numpy() == csr.doc_len).all()


def test_statistics_are_dropped_with_the_csr():
    docs = _random_docs(60)
    col = _collection(docs)
    csr = col._token_csr()
    col._drop_derived(ids_changed=False, metadata_changed=True, documents_changed=False)
    assert col._token_csr() is csr
    col.documents[3] = "entirely new words words"
    col._drop_derived(ids_changed=False, documents_changed=True)
    assert "_tok" not in col.__dict__
    fresh = col._token_csr()
    assert fresh is not csr
    docs[3] = "entirely new words words"
    _assert_stats_are(fresh, docs)


def test_offsets_ids_and_vocabulary_are_what_they_were():
    docs = _random_docs(200)
    vocab, rows = {}, []                                               # the construction before the statistics arrived
    for doc in docs:
        rows.append(sorted({vocab.setdefault(w, len(vocab)) for w in doc.lower().split()}))
    csr = _collection(docs)._token_csr()
    assert csr.vocab == vocab and list(csr.vocab) == list(vocab)
    assert csr.offsets.tolist() == np.r_[0, np.cumsum([len(r) for r in rows])].tolist()
    assert csr.token_ids.tolist() == [t for r in rows for t in r]
    assert csr.offsets.dtype == np.int64 and csr.token_ids.dtype == np.int32


# ---- boundary --------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ("crs_bm25_topk", "crs_bm25_workspace_bytes", "crs_fuse_rrf"):
        assert re.search(r"\bint %s\s*\(" % name, header), f"{name} not declared in include/crs_hip.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in nat.exported_symbols()
    import rag._encoder  # noqa: F401  (registers the encoder header's entry points in the binding table)
    encoder = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_encoder.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(crs_[a-z0-9_]+)\s*\(", header + encoder))
    assert declared == set(nat.exported_symbols()), "binding table and headers disagree"
    assert lib.crs_abi_version() == 3
    assert nat.has_bm25() and callable(nat.bm25_topk) and callable(nat.fuse_rrf)
    assert re.search(r"#define CRS_BM25_MAX_PAIRS (\d+)", header).group(1) == str(nat.BM25_MAX_PAIRS)
    assert str(torch.ops.crs.bm25_topk.default._schema) == \
        ("crs::bm25_topk(Tensor doc_offsets, Tensor doc_tokens, Tensor doc_tf, Tensor doc_len, int n_rows, Tensor q_offsets, "
         "Tensor q_tokens, Tensor q_weights, float c0, float c1, float k1p1, int k, Tensor(a!) workspace, Tensor(b!) out_scores, "
         "Tensor(c!) out_rows) -> ()")
    assert str(torch.ops.crs.fuse_rrf.default._schema) == \
        ("crs::fuse_rrf(Tensor dense_rows, Tensor lex_rows, float c, float w_dense, float w_lex, Tensor(a!) rows, Tensor(b!) fused, "
         "Tensor(c!) dense_pos, Tensor(d!) lex_pos, Tensor(e!) count) -> ()")
    makefile = open(os.path.join(ROOT, "compressed-rag-suite_amd", "csrc", "Makefile")).read()
    assert "bm25.hip" in makefile and "fuse.hip" in makefile


def test_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 8192)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    EINVAL, ENOSPC = -1, -2
    need = nat.bm25_workspace_bytes(4, 10, 1000)
    assert need > 0 and need % 256 == 0 and nat.bm25_workspace_bytes(64, 64, 1_000_000) > need
    names = ("doc_off", "doc_tok", "doc_tf", "doc_len", "n_rows", "n_doc_tok", "q_off", "q_tok", "q_w", "nq", "n_q_tok", "c0", "c1", "k1p1",
             "k", "ws", "ws_bytes", "out_s", "out_r")
    good = dict(doc_off=p, doc_tok=p, doc_tf=p, doc_len=p, n_rows=1000, n_doc_tok=9000, q_off=p, q_tok=p, q_w=p, nq=4, n_q_tok=12, c0=0.4,
                c1=0.01, k1p1=2.5, k=10, ws=p, ws_bytes=need, out_s=p, out_r=p)

    def call(**change):
        args = dict(good, **change)
        return lib.crs_bm25_topk(*[args[n] for n in names], None)

    for bad, word in (({"nq": 0}, b"nq"), ({"nq": 65}, b"nq"), ({"k": 0}, b"k"), ({"k": 65}, b"k"), ({"n_rows": -1}, b"n_rows"),
                      ({"n_rows": 2 ** 31}, b"n_rows"), ({"n_doc_tok": -1}, b"n_doc_tokens"), ({"n_q_tok": -1}, b"n_q_tokens"),
                      ({"n_q_tok": nat.BM25_MAX_PAIRS + 1}, b"CRS_BM25_MAX_PAIRS"), ({"doc_off": None}, b"null pointer"),
                      ({"doc_tok": None}, b"null pointer"), ({"doc_tf": None}, b"null pointer"), ({"doc_len": None}, b"null pointer"),
                      ({"q_off": None}, b"null pointer"), ({"q_tok": None}, b"null pointer"), ({"q_w": None}, b"null pointer"),
                      ({"out_s": None}, b"null pointer"), ({"out_r": None}, b"null pointer"), ({"ws": None}, b"workspace"),
                      ({"ws": ctypes.c_void_p(p.value + 8)}, b"workspace")):
        assert call(**bad) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    assert call(ws_bytes=need - 1) == ENOSPC
    size = ctypes.c_size_t(0)
    assert lib.crs_bm25_workspace_bytes(0, 10, 1000, ctypes.byref(size)) == EINVAL
    assert lib.crs_bm25_workspace_bytes(4, 10, 1000, None) == EINVAL

    f_names = ("dense", "m_dense", "lex", "m_lex", "nq", "c", "w_dense", "w_lex", "k_out", "rows", "fused", "dpos", "lpos", "count")
    f_good = dict(dense=p, m_dense=20, lex=p, m_lex=20, nq=3, c=60.0, w_dense=1.0, w_lex=1.0, k_out=20, rows=p, fused=p, dpos=p, lpos=p, count=p)

    def fuse(**change):
        args = dict(f_good, **change)
        return lib.crs_fuse_rrf(*[args[n] for n in f_names], None)

    for bad, word in (({"nq": -1}, b"nq"), ({"m_dense": 0}, b"m_dense"), ({"m_dense": 65}, b"m_dense"), ({"m_lex": 0}, b"m_lex"),
                      ({"m_lex": 65}, b"m_lex"), ({"k_out": 0}, b"k_out"), ({"k_out": 129}, b"k_out"), ({"c": -1.0}, b"c must"),
                      ({"c": float("nan")}, b"c must"), ({"w_dense": -1.0}, b"weights"), ({"w_lex": float("inf")}, b"weights"),
                      ({"dense": None}, b"null pointer"), ({"lex": None}, b"null pointer"), ({"rows": None}, b"null pointer"),
                      ({"fused": None}, b"null pointer"), ({"dpos": None}, b"null pointer"), ({"lpos": None}, b"null pointer"),
                      ({"count": None}, b"null pointer")):
        assert fuse(**bad) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    assert fuse(nq=0) == 0                                               # nothing to do: no launch


@pytest.mark.parametrize("source,kernels", [("bm25.hip", 2), ("fuse.hip", 1)])
def test_kernels_use_no_scratch(source, kernels):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), source], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout and f"{kernels} kernels in 1 files" in r.stdout, r.stdout


# ---- the references -----------------------------------------------------------------------------------------------------------------
def _csr_of(docs):
    return _collection(docs)._token_csr()


def _query_block(csr, queries):
    """q_offsets, q_tokens, q_weights of a query batch, as VectorStore.bm25_rows builds them."""
    ids = [csr.query_ids(q)[0] for q in queries]
    q_off = np.r_[0, np.cumsum([len(t) for t in ids])].astype(np.int64)
    q_tok = np.array([t for ts in ids for t in ts], dtype=np.int32)
    q_w = np.array([ref.weight(csr.rows, int(csr.df[t])) for t in q_tok.tolist()], dtype=np.float32)
    return q_off, q_tok, q_w


def test_vectorised_reference_has_the_scalar_loops_bits():
    docs = ref.corpus(200, seed=2)
    csr = _csr_of(docs)
    q_off, q_tok, q_w = _query_block(csr, ref.queries(8))
    c0, c1, k1p1 = ref.constants(csr.rows, csr.total_len)
    for q in range(8):
        lo, hi = q_off[q], q_off[q + 1]
        args = (csr.offsets, csr.token_ids, csr.tfs, csr.doc_len, csr.rows, q_tok[lo:hi], q_w[lo:hi], c0, c1, k1p1)
        s_v, h_v = ref.bm25_scores_ref(*args)
        s_s, h_s = ref.bm25_scores_scalar(*args)
        assert (h_v == h_s).all() and (s_v.view(np.int32) == s_s.view(np.int32)).all(), q


def test_fp32_reference_agrees_with_the_fp64_textbook():
    """|fp32 - fp64| <= (m + 6) 2^-24 score for a row with m matching terms: every term is positive (no cancellation), takes four
    roundings, and the sum takes m.  Also the cap the GPU test relies on: of the seeded plain queries at most 2 % have a k-th /
    (k+1)-th fp64 score closer than that bound, at k = 1 and k = 10 (tests/test_bm25_gpu.py drops those before it compares row sets),
    and on the others the fp32 reference's row set IS the textbook's."""
    docs = ref.corpus(1000)
    special, plain = ref.queries(64), ref.plain_queries(100)
    queries = special + plain
    csr = _csr_of(docs)
    book = ref.Textbook(docs)
    q_off, q_tok, q_w = _query_block(csr, queries)
    c0, c1, k1p1 = ref.constants(csr.rows, csr.total_len)
    worst, checked, close = 0.0, 0, {1: 0, 10: 0}
    for q, query in enumerate(queries):
        lo, hi = q_off[q], q_off[q + 1]
        s32, hit = ref.bm25_scores_ref(csr.offsets, csr.token_ids, csr.tfs, csr.doc_len, csr.rows, q_tok[lo:hi], q_w[lo:hi], c0, c1, k1p1)
        want = book.scores(query)
        assert set(np.nonzero(hit)[0].tolist()) == set(want)
        for r, (s64, m) in want.items():
            err, bound = abs(float(s32[r]) - s64), (m + 6) * ref.EPS32 * s64
            worst = max(worst, err / bound)
            checked += 1
            assert err <= bound, (q, r, float(s32[r]), s64, m, err / bound)
        for k in close:
            if q < len(special):
                continue
            if ambiguous_topk(want, k):
                close[k] += 1
            else:
                assert set(ref.topk_of(s32, hit, k)[1].tolist()) - {-1} == textbook_topk(want, k), (q, k)
    print(f"fp32 vs fp64 over {checked} (query, row) scores: worst error / bound = {worst:.3f}; plain queries ambiguous at k: {close} of {len(plain)}")
    assert checked > 10000
    assert all(n <= 0.02 * len(plain) for n in close.values()), close


def textbook_topk(want, k):
    """The rows of the fp64 top-k (score descending, ties by lower row)."""
    return {r for r, _ in sorted(want.items(), key=lambda rs: (-rs[1][0], rs[0]))[:k]}


def ambiguous_topk(want, k):
    """1 when the fp64 k-th and (k+1)-th scores lie closer than the fp32 rounding bound (the top-k SET is then not decided)."""
    ranked = sorted(want.values(), key=lambda sm: -sm[0])
    if len(ranked) <= k:
        return 0
    (a, ma), (b, mb) = ranked[k - 1], ranked[k]
    return int(a - b <= (ma + 6) * ref.EPS32 * a + (mb + 6) * ref.EPS32 * b)


def test_fusion_reference_on_hand_cases():
    rows, fused, dpos, lpos, n = ref.fuse_rrf_ref([7, 3, -1], [3, 9], 4)
    assert rows.tolist() == [3, 7, 9, -1] and n == 3
    assert fused.tolist() == [1.0 / 62.0 + 1.0 / 61.0, 1.0 / 61.0, 1.0 / 62.0, 0.0]
    assert dpos.tolist() == [1, 0, -1, -1] and lpos.tolist() == [0, -1, 1, -1]
    rows, fused, dpos, lpos, n = ref.fuse_rrf_ref([5], [6], 2)            # the exact tie: the dense entry first
    assert rows.tolist() == [5, 6] and fused[0] == fused[1]


# ---- the store: launch cutting -------------------------------------------------------------------------------------------------------
def _store(docs):
    from rag.indexing import VectorStore
    store = VectorStore({"collection_name": "bm25"})
    store.collection = store._adopt(_collection(docs))
    return store


def _patch_natives(monkeypatch):
    """nat.bm25_topk / nat.fuse_rrf replaced by the references, on CPU tensors; returns the list of bm25 launches (nq, pairs)."""
    import torch
    from rag import _native as nat
    launches = []

    def bm25(doc_off, doc_tok, doc_tf, doc_len, n_rows, q_off, q_tok, q_w, c0, c1, k1p1, k, workspace=None, out_scores=None, out_rows=None):
        assert q_off.dtype == torch.int64 and q_tok.dtype == torch.int32 and q_w.dtype == torch.float32 and doc_tf.dtype == torch.int32
        assert c0 == float(np.float32(c0)) and c1 == float(np.float32(c1)) and k1p1 == float(np.float32(k1p1))   # rounded once, by the caller
        launches.append((q_off.shape[0] - 1, int(q_tok.shape[0])))
        s, r = ref.bm25_topk_ref(doc_off.numpy(), doc_tok.numpy(), doc_tf.numpy(), doc_len.numpy(), n_rows, q_off.numpy(), q_tok.numpy(),
                                 q_w.numpy(), c0, c1, k1p1, k)
        out_scores.copy_(torch.from_numpy(s))
        out_rows.copy_(torch.from_numpy(r))
        return out_scores, out_rows

    def fuse(dense_rows, lex_rows, k_out, c=60.0, w_dense=1.0, w_lex=1.0, out=None):
        for i in range(dense_rows.shape[0]):
            got = ref.fuse_rrf_ref(dense_rows[i].tolist(), lex_rows[i].tolist(), k_out, c, w_dense, w_lex)
            for t, v in zip(out[:4], got[:4]):
                t[i].copy_(torch.from_numpy(v))
            out[4][i] = got[4]
        return out

    monkeypatch.setattr(nat, "bm25_topk", bm25)
    monkeypatch.setattr(nat, "fuse_rrf", fuse)
    return launches


def test_bm25_rows_cuts_a_batch_at_64_queries_and_at_the_pair_cap(monkeypatch):
    from rag import _native as nat
    docs = ref.corpus(300, seed=4)
    store = _store(docs)
    csr = store.collection._token_csr()
    launches = _patch_natives(monkeypatch)
    queries = ref.queries(65)
    scores, rows = store.bm25_rows(queries, 10)
    assert [n for n, _ in launches] == [64, 1] and scores.shape == rows.shape == (65, 10)
    q_off, q_tok, q_w = _query_block(csr, queries)
    c0, c1, k1p1 = ref.constants(csr.rows, csr.total_len)
    want_s, want_r = ref.bm25_topk_ref(csr.offsets, csr.token_ids, csr.tfs, csr.doc_len, csr.rows, q_off, q_tok, q_w, c0, c1, k1p1, 10)
    assert (rows == want_r).all() and (scores.view(np.int32) == want_s.view(np.int32)).all()
    assert (rows[1] == -1).all() and np.isneginf(scores[1]).all()         # the query that knows no word
    # the pair cap: 30 queries of 200 known words each = 6000 pairs -> 20 queries (4000 pairs) + 10
    wide = [" ".join(f"w{t}" for t in range(s, s + 200)) for s in range(30)]
    known = [len(csr.query_ids(q)[0]) for q in wide]
    del launches[:]
    store.bm25_rows(wide, 5)
    assert sum(n for n, _ in launches) == 30 and len(launches) >= 2
    assert all(pairs <= nat.BM25_MAX_PAIRS for _, pairs in launches)
    assert [pairs for _, pairs in launches] == [sum(known[lo:hi]) for lo, hi in store._bm25_launches(known)]
    assert store._bm25_launches([4000, 96, 1]) == [(0, 2), (2, 3)] and store._bm25_launches([0] * 130) == [(0, 64), (64, 128), (128, 130)]
    # dict form
    got = store.search_lexical_batch(queries[:3], top_k=4)
    assert set(got) == {"ids", "documents", "metadatas", "scores"} and [len(x) for x in got["ids"]] == [4, 0, 4]
    assert got["ids"][0] == [f"c{r}" for r in want_r[0, :4]] and got["scores"][0] == want_s[0, :4].astype(np.float64).tolist()


def test_bm25_rows_refuses_bad_arguments(monkeypatch):
    from rag import _native as nat
    store = _store([" ".join(f"u{t}" for t in range(nat.BM25_MAX_PAIRS + 1)), "short one"])
    launches = _patch_natives(monkeypatch)
    with pytest.raises(ValueError, match="distinct known tokens"):
        store.bm25_rows(["fine", " ".join(f"u{t}" for t in range(nat.BM25_MAX_PAIRS + 1))], 5)
    assert launches == []                                                # refused before anything ran
    for bad in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="top_k"):
            store.bm25_rows(["short"], bad)
    with pytest.raises(ValueError, match="k1"):
        store.bm25_rows(["short"], 5, k1=-1.0)
    with pytest.raises(ValueError, match="b"):
        store.bm25_rows(["short"], 5, b=1.5)
    scores, rows = store.bm25_rows([], 5)
    assert scores.shape == rows.shape == (0, 5)


# ---- the retriever -------------------------------------------------------------------------------------------------------------------
class _NoStore:
    collection = None


def test_retriever_validates_the_hybrid_key():
    from rag.retrieval import ContextRetriever
    assert ContextRetriever(_NoStore(), None, {}).hybrid is None
    assert ContextRetriever(_NoStore(), None, {"hybrid": False}).hybrid is None
    r = ContextRetriever(_NoStore(), None, {"hybrid": True})
    assert r.hybrid == {"rrf_k": 60.0, "weights": (1.0, 1.0), "k1": 1.5, "b": 0.75} and r.last_hybrid == {"lists": 0, "lexical_only_hits": 0}
    r = ContextRetriever(_NoStore(), None, {"hybrid": {"rrf_k": 10, "weights": [2, 1], "k1": 1.2, "b": 0.5}})
    assert r.hybrid == {"rrf_k": 10.0, "weights": (2.0, 1.0), "k1": 1.2, "b": 0.5}
    assert ContextRetriever(_NoStore(), None, {"hybrid": {}}).hybrid["rrf_k"] == 60.0
    for bad in ("yes", 1, {"rrf": 60}, {"rrf_k": -1}, {"rrf_k": "60"}, {"rrf_k": True}, {"weights": [1]}, {"weights": [0, 0]},
                {"weights": [-1, 1]}, {"weights": "11"}, {"k1": -0.1}, {"k1": float("nan")}, {"b": 1.5}, {"b": None}):
        with pytest.raises(ValueError, match="hybrid"):
            ContextRetriever(_NoStore(), None, {"hybrid": bad})


class _Model:
    def embed(self, texts):
        return np.zeros((len(texts), 8), dtype=np.float32) if isinstance(texts, list) else np.zeros(8, dtype=np.float32)


def _hybrid_retriever(monkeypatch, config, dense):
    """A retriever over a CPU collection whose natives are the references and whose dense search returns `dense`
    (per query: (cosine scores, rows))."""
    from rag.retrieval import ContextRetriever
    docs = [f"filler text number {r} about nothing" for r in range(40)]
    docs[31] = "the part number ZX-4471-Q is listed here"
    docs[7] = "filler text mentioning zx-4471-q twice: ZX-4471-Q"
    store = _store(docs)
    _patch_natives(monkeypatch)
    calls = {"bm25_rows": 0}
    inner = store.bm25_rows

    def counted(*a, **kw):
        calls["bm25_rows"] += 1
        return inner(*a, **kw)

    def search_rows(emb, top_k):
        n = len(emb)
        s = np.full((n, top_k), -np.inf, dtype=np.float32)
        r = np.full((n, top_k), -1, dtype=np.int64)
        for i in range(n):
            sc, rw = dense[i]
            s[i, :len(sc)], r[i, :len(rw)] = sc[:top_k], rw[:top_k]
        return s, r

    monkeypatch.setattr(store, "bm25_rows", counted)
    monkeypatch.setattr(store, "search_rows", search_rows)
    return ContextRetriever(store, _Model(), config), store, calls


def test_hybrid_retrieve_batch_builds_the_documented_dicts(monkeypatch):
    dense = [(np.array([0.9, 0.8, 0.7, 0.1], dtype=np.float32), np.array([2, 7, 3, 4])),
             (np.array([0.95], dtype=np.float32), np.array([5]))]
    r, store, calls = _hybrid_retriever(monkeypatch, {"top_k": 4, "hybrid": True, "similarity_threshold": 0.7}, dense)
    out = r.retrieve_batch(["ZX-4471-Q", "unknownword"])
    assert calls["bm25_rows"] == 1 and r.last_hybrid == {"lists": 2, "lexical_only_hits": 1}
    first, second = out
    keys = {"text", "score", "distance", "metadata", "chunk_id", "dense_score", "bm25_score", "dense_rank", "lexical_rank"}
    assert all(set(c) == keys for c in first + second)
    # dense list after the threshold: rows 2, 7, 3 (0.1 maps below 0.7); lexical list: rows 7 (tf 2) and 31
    lex_s, lex_r = store.bm25_rows(["ZX-4471-Q"], 4)
    assert lex_r[0].tolist()[:2] == [7, 31] and lex_r[0, 2] == -1
    assert [c["chunk_id"] for c in first] == ["c7", "c2", "c31", "c3"]
    top = first[0]
    assert top["dense_rank"] == 1 and top["lexical_rank"] == 0 and top["bm25_score"] == float(lex_s[0, 0])
    assert top["score"] == (1.0 / 62.0 + 1.0 / 61.0) / (2.0 / 61.0) and 0.0 < top["score"] <= 1.0
    dist = float(np.float32(1.0) - np.float32(0.8))
    assert top["distance"] == dist and top["dense_score"] == 1.0 - dist * dist / 2.0
    only_lex = first[2]
    assert only_lex["distance"] is None and only_lex["dense_score"] is None and only_lex["dense_rank"] is None
    assert only_lex["lexical_rank"] == 1 and only_lex["bm25_score"] == float(lex_s[0, 1]) and only_lex["score"] == (1.0 / 62.0) / (2.0 / 61.0)
    only_dense = first[1]
    assert only_dense["lexical_rank"] is None and only_dense["bm25_score"] == 0.0 and only_dense["dense_rank"] == 0
    assert only_dense["score"] == 0.5                                       # (1 / 61) / (2 / 61)
    assert [c["chunk_id"] for c in second] == ["c5"] and second[0]["lexical_rank"] is None
    # retrieve() goes through retrieve_batch, and refuses filters
    assert [c["chunk_id"] for c in r.retrieve("ZX-4471-Q")] == ["c7", "c2", "c31", "c3"]
    with pytest.raises(ValueError, match="filters"):
        r.retrieve("ZX-4471-Q", filters={"page": 1})
    with pytest.raises(ValueError, match="64"):
        r.retrieve_batch(["x"], top_k=65)


def test_hybrid_lists_go_through_the_rerank_and_the_cut(monkeypatch):
    dense = [(np.array([0.9, 0.8, 0.7, 0.6], dtype=np.float32), np.array([2, 7, 3, 4]))]
    r, store, calls = _hybrid_retriever(monkeypatch, {"top_k": 2, "rerank": True, "hybrid": {"weights": [1, 3]}, "lexical_rerank": "device"}, dense)
    out = r.retrieve_batch(["ZX-4471-Q"])[0]
    assert len(out) == 2 and all("rerank_score" in c for c in out) and r.last_rerank["mode"] == "host"
    assert out[0]["chunk_id"] == "c7" and out[0]["rerank_score"] == out[0]["score"] * 0.7 + 1.0 * 0.3


def test_without_hybrid_the_retriever_never_calls_bm25_rows(monkeypatch):
    dense = [(np.array([0.9, 0.8], dtype=np.float32), np.array([2, 7]))]
    for config in ({"top_k": 2}, {"top_k": 2, "hybrid": False}, {"top_k": 1, "rerank": True}):
        r, store, calls = _hybrid_retriever(monkeypatch, config, dense)
        out = r.retrieve_batch(["ZX-4471-Q"])[0]
        assert calls["bm25_rows"] == 0 and r.last_hybrid == {"lists": 0, "lexical_only_hits": 0}
        assert set(out[0]) - {"rerank_score"} == {"text", "score", "distance", "metadata", "chunk_id"}
