"""GPU: the 2-bit residual token index -- crs::token_compress against the numpy restatement, crs::maxsim_rc against
fp64 MaxSim over the numpy-decoded tokens (tests/_rc_ref.py), crs::maxsim_topk_rc bit for bit against crs::maxsim_rc, and the
format through a store."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import _rc_ref as rc

pytestmark = pytest.mark.gpu

Q_LENS = (1, 16, 17, 64)
DOC_LENS = (1, 16, 0, 17, 300)      # one empty row; 300 tokens: longer than a window
# the sweep: windows are 256 tokens and items 64 rows; 255 / 256 / 257 sit on a window's edge, 600 is longer than two windows
SCAN_LENS = tuple([255, 1, 256, 0, 257, 600, 0, 33] + [(11 * i) % 47 for i in range(192)])
GROUP_Q = 8      # kMsRcGroupQ
WEIGHTS = np.asarray([-0.07, -0.02, 0.015, 0.06], np.float32)
CUTOFFS = np.asarray([-0.04, 0.0, 0.035], np.float32)


def _unit16(rng, n, dimp, dim):
    x = np.zeros((n, dimp))
    x[:, :dim] = rng.standard_normal((n, dim))
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float16)


@functools.lru_cache(maxsize=None)
def _case(dimp, nq, lens, k_cent=64):
    """A codec of random unit centroids, an index of random fields over documents of `lens` tokens, fp16 unit queries (poisoned
    past q_len); the last 3 coordinates are padding when dimp > 32."""
    rng = np.random.default_rng(dimp + 1000 * nq + len(lens))
    dim = dimp - 3 if dimp > 32 else dimp
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offsets[-1])
    q16 = _unit16(rng, nq * 64, dimp, dim).reshape(nq, 64, dimp)
    q_len = np.asarray([Q_LENS[i % 4] for i in range(nq)], dtype=np.int32)
    for a in range(nq):
        q16[a, q_len[a]:] = 300.0
    case = {"q16": q16, "q_len": q_len, "offsets": offsets, "centroids": _unit16(rng, k_cent, dimp, dim), "weights": WEIGHTS,
            "cid": rng.integers(0, k_cent, n).astype(np.int32), "codes": rng.integers(0, 256, (n, dimp // 4)).astype(np.uint8),
            "scale": rng.uniform(0.8, 1.2, n).astype(np.float16)}
    case["dec"] = rc.decode(case["centroids"], WEIGHTS, case["cid"], case["codes"], case["scale"])
    return case


def _dev(cuda, case):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    index = SimpleNamespace(cid=t(case["cid"]), codes=t(case["codes"]), scale=t(case["scale"]), n_tokens=len(case["cid"]),
                            offsets_dev=t(case["offsets"]), n_rows=len(case["offsets"]) - 1,
                            codec=SimpleNamespace(centroids=t(case["centroids"]), weights=t(case["weights"])))
    return t(case["q16"]), t(case["q_len"]), index


@pytest.mark.parametrize("n_tok", [1, 257])
@pytest.mark.parametrize("k_cent", [16, 272])      # one centroid tile; several with a ragged last one
@pytest.mark.parametrize("dimp", [32, 64, 96, 128])
def test_compression_against_the_reference(cuda, dimp, k_cent, n_tok):
    import torch
    from rag import _native as nat
    rng = np.random.default_rng(dimp + k_cent + n_tok)
    dim = dimp - 3 if dimp > 32 else dimp
    cent = _unit16(rng, k_cent, dimp, dim)
    cent[9] = cent[4]                                         # two identical centroids: the lower id wins
    planted = np.resize(np.asarray([4, 0, k_cent - 1] + list(rng.integers(0, k_cent, 61))), n_tok)
    x = cent[planted].astype(np.float64)
    x[:, :dim] += 0.25 / np.sqrt(dim) * rng.standard_normal((n_tok, dim))
    x16 = (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float16)
    cid, codes, scale, margin = rc.compress(x16, cent, CUTOFFS, WEIGHTS, dim)
    # the kernel's dot is an fp32 accumulation of exact products: off by at most dimp 2^-23 |x| |c| <= dimp 2^-22 per centroid
    assert margin.min() > 2 * dimp * 2.0 ** -22, "the planted tokens must leave no doubt about the nearest centroid"
    assert 4 in cid and 9 not in cid
    t = lambda a: torch.from_numpy(a).to(cuda)
    got_codes = torch.full((n_tok + 1, dimp // 4), 0x55, dtype=torch.uint8, device=cuda)
    got_scale = torch.full((n_tok + 1,), 7.0, dtype=torch.float16, device=cuda)
    got_cid = nat.token_compress(t(x16), dim, t(cent), t(CUTOFFS), t(WEIGHTS), first=1, codes=got_codes, scale=got_scale)
    assert got_cid[1:].cpu().numpy().tolist() == cid.tolist()
    assert nat.token_compress(t(x16), dim, t(cent)).cpu().numpy().tolist() == cid.tolist()      # the assignment stage alone
    assert np.array_equal(got_codes[1:].cpu().numpy(), codes)
    assert np.all(got_codes[0].cpu().numpy() == 0x55) and float(got_scale[0]) == 7.0            # slot 0 was not the call's
    err = np.abs(got_scale[1:].cpu().numpy().astype(np.float64) - scale)
    ulp = 2.0 ** (np.floor(np.log2(scale)) - 10)
    print(f"token_compress dimp {dimp} K {k_cent} T {n_tok}: largest scale error {np.max(err / ulp):.3f} ulp")
    assert np.all(err <= ulp)


@pytest.mark.parametrize("dimp", [32, 64, 96, 128])
def test_maxsim_rc_against_fp64(cuda, dimp):
    import torch
    from rag import _native as nat
    case = _case(dimp, 4, DOC_LENS)
    rows = np.tile(np.arange(len(DOC_LENS), dtype=np.int64), (4, 1))
    rows = np.concatenate([rows, np.full((4, 1), -1, np.int64)], axis=1)      # a negative candidate slot
    want, tol = rc.maxsim(case["q16"], case["q_len"], case["dec"], case["offsets"], rows)
    q16, q_len, index = _dev(cuda, case)
    got = nat.maxsim_rc(q16, q_len, index, torch.from_numpy(rows).to(cuda)).cpu().numpy().astype(np.float64)
    live = tol > 0
    err = np.abs(got[live] - want[live])
    print(f"maxsim_rc dimp {dimp}: largest |error| / tolerance {np.max(err / tol[live]):.3f}")
    assert np.all(got[~live] == want[~live])                  # 0 for the empty row, -inf for the negative slot
    assert np.all(err <= tol[live])


def _check_topk(cuda, case, k, first=0, count=None):
    import torch
    from rag import _native as nat
    q16, q_len, index = _dev(cuda, case)
    n_rows, nq = index.n_rows, len(case["q_len"])
    count = n_rows - first if count is None else count
    full = nat.maxsim_rc(q16, q_len, index, torch.arange(n_rows, device=cuda).repeat(nq, 1)).cpu().numpy()
    s, r = nat.maxsim_topk_rc(q16, q_len, index, k, row_first=first, row_count=count)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    nonempty = np.diff(case["offsets"]) > 0
    rows = [x for x in range(first, first + count) if nonempty[x]]
    for q in range(nq):
        best = sorted(rows, key=lambda x: (-full[q, x], x))[:k]
        assert r[q].tolist() == best + [-1] * (k - len(best)), (q, r[q], best)
        assert s[q, :len(best)].view(np.uint32).tolist() == full[q, best].view(np.uint32).tolist(), q
        assert np.all(np.isneginf(s[q, len(best):]))


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("nq", [1, GROUP_Q, GROUP_Q + 1])
@pytest.mark.parametrize("dimp", [32, 64, 96, 128])
def test_topk_rc_is_maxsim_rc_bit_for_bit(cuda, dimp, nq, k):
    _check_topk(cuda, _case(dimp, nq, SCAN_LENS), k)


@pytest.mark.parametrize("first, count, k", [(3, 130, 10), (6, 20, 64)])      # row_first > 0; fewer than k rows that hold tokens
def test_topk_rc_row_range(cuda, first, count, k):
    _check_topk(cuda, _case(128, GROUP_Q + 1, SCAN_LENS), k, first=first, count=count)


def test_a_cid_outside_the_table_decodes_to_zeros(cuda):
    """The C ABI cannot refuse device data without a host sync: such a token is never used as an index and scores as a zero vector,
    in both kernels (tests/_rc_ref.py decodes it the same way)."""
    case = dict(_case(64, 2, (3, 20, 5)))
    case["cid"] = case["cid"].copy()
    case["cid"][[1, 4, 22]] = [-1, 64, 2 ** 31 - 1]
    case["dec"] = rc.decode(case["centroids"], WEIGHTS, case["cid"], case["codes"], case["scale"])
    assert np.all(case["dec"][[1, 4, 22]] == 0)
    import torch
    from rag import _native as nat
    rows = np.tile(np.arange(3, dtype=np.int64), (2, 1))
    want, tol = rc.maxsim(case["q16"], case["q_len"], case["dec"], case["offsets"], rows)
    got = nat.maxsim_rc(*_dev(cuda, case), torch.from_numpy(rows).to(cuda)).cpu().numpy()
    assert np.all(np.abs(got - want) <= tol)
    _check_topk(cuda, case, 3)


@pytest.mark.parametrize("bad, word", [(dict(lq_max=65), "lq_max"), (dict(dimp=48), "dimp"), (dict(k=65), "k must"), (dict(K=15), "n_centroids"),
                                       (dict(K=(1 << 20) + 1), "n_centroids"), (dict(row_first=1), "row range"),
                                       (dict(ws_bytes=16), "workspace too small")])
def test_refusals(cuda, bad, word):
    """CRS_EINVAL with a message naming the argument, through the C ABI (the torch ops check the same limits ahead of it)."""
    import torch
    from rag import _native as nat
    lib, buf = nat.load(), torch.zeros(4096, dtype=torch.uint8, device=cuda)
    p = buf.data_ptr()
    a = dict(nq=2, lq_max=4, dimp=32, k=4, K=16, row_first=0, ws_bytes=nat.maxsim_topk_rc_workspace_bytes(2, 4, 2))
    assert a["ws_bytes"] <= 4096 - 1024
    a.update(bad)
    rc_ = lib.crs_maxsim_topk_rc(p, p, a["nq"], a["lq_max"], p, p, p, p, a["K"], p, p, 2, 8, a["row_first"], 2, a["dimp"], a["k"], p + 1024,
                                 a["ws_bytes"], p, p, None)
    assert rc_ != 0 and word in lib.crs_last_error().decode()
    if word in ("lq_max", "dimp", "n_centroids"):
        assert lib.crs_maxsim_rc(p, p, a["nq"], a["lq_max"], p, p, p, p, a["K"], p, p, 2, 8, p, 1, a["dimp"], p, None) != 0
        assert word in lib.crs_last_error().decode()
    if word in ("dimp", "n_centroids"):
        assert lib.crs_token_compress(p, 4, a["dimp"], 16, p, a["K"], p, p, p, p, p, None) != 0 and word in lib.crs_last_error().decode()


def _check_retriever(p, questions, n):
    """retrieve_batch returns the best rows by the store's (reference-checked) score_rows, in that order, with that score."""
    li, store = p.retriever.late_interaction, p.vector_store
    p.retriever.similarity_threshold = -1.0
    full = li.score_rows(questions, np.tile(np.arange(n, dtype=np.int64), (len(questions), 1)), store).cpu().numpy()
    for a, chunks in enumerate(p.retriever.retrieve_batch(questions)):
        rows = [int(c["chunk_id"].split("_")[1]) for c in chunks]
        assert rows and rows == sorted(range(n), key=lambda r: (-full[a, r], r))[:len(rows)]
        assert [np.float32(c["rerank_score"]) for c in chunks] == [full[a, r] for r in rows]


@pytest.mark.parametrize("stage", ["dense", "scan"])
def test_rerank_score_is_the_kernels_sum(cuda, stage):
    """Both first stages: 40 chunks, top_k 20, so the dense stage's candidates (2 top_k) are every row."""
    import _late_cases as lc
    from test_late_interaction_gpu import LI_CFG, _pipeline
    docs = [t or "an empty chunk" for t in lc.corpus(40)]
    p = _pipeline("rc-" + stage, docs, {"late_interaction": dict(LI_CFG, token_dtype="res2", centroids=64, first_stage=stage), "top_k": 20})
    chunks = p.retriever.retrieve_batch(lc.queries(5))
    assert all(len(c) == 20 for c in chunks)
    _check_retriever(p, lc.queries(5), 40)


def test_through_the_store(cuda):
    """synthetic:tiny-colbert with token_dtype 'res2' and 64 centroids: the store's scores are the reference's over its own planes
    and codec, search_late_batch is the ranking by them, an append keeps the codec and the old bytes, and the size guard counts
    tokens x (dimp / 4 + 6) + centroids x dimp x 2 before any forward."""
    import _late_cases as lc
    from test_late_interaction_gpu import LI_CFG, _chunks, _pipeline
    texts, questions = lc.corpus(150), lc.queries(9)
    cfg = dict(LI_CFG, token_dtype="res2", centroids=64, first_stage="scan")
    p = _pipeline("rc-store", texts[:100], {"late_interaction": cfg})
    store, li = p.vector_store, p.retriever.late_interaction

    def check(k):
        index, n = store.token_index(), store.collection.count()
        assert index.tok16 is None and index.codes.dtype.itemsize == 1 and index.codec.n_centroids == 64
        host = lambda x: x.cpu().numpy()
        dec = rc.decode(host(index.codec.centroids), host(index.codec.weights), host(index.cid)[:index.n_tokens],
                        host(index.codes)[:index.n_tokens], host(index.scale)[:index.n_tokens])
        q16, q_len = li.encode_queries_device(questions)
        rows = np.tile(np.arange(n, dtype=np.int64), (len(questions), 1))
        want, tol = rc.maxsim(host(q16), host(q_len), dec, index.offsets, rows)
        full = host(li.score_rows(questions, rows, store))
        assert np.all(np.abs(full - want) <= tol)
        got = store.search_late_batch(questions, top_k=k)
        for a in range(len(questions)):
            order = sorted(range(n), key=lambda r: (-full[a, r], r))[:k]
            assert got["rows"][a] == order
            assert np.asarray(got["scores"][a], np.float32).tobytes() == full[a, order].tobytes()
        return index

    index = check(10)
    codec, before = index.codec, (index.n_tokens, index.codes[:index.n_tokens].clone(), index.codec.centroids.clone())
    new = _chunks(texts[100:], first=100)
    store.create_index(new, p.embedding_model.embed_chunks_device(new), metadata_fields=["page_number"])
    again = check(32)
    assert again is index and again.codec is codec and again.n_tokens > before[0]
    assert bool((again.codes[:before[0]] == before[1]).all()) and bool((codec.centroids == before[2]).all())
    _check_retriever(p, questions, 150)
    assert store.delete(ids=["c_3"]) == 1
    assert check(7) is not index and store.token_index().codec is codec      # rebuilt after a document change: the codec stays
    # the guard: a fresh store, one byte short
    q = _pipeline("rc-guard", texts[:100], {"late_interaction": cfg})
    need = before[0] * (li.dimp // 4 + 6) + 64 * li.dimp * 2
    q.vector_store.max_index_bytes = need - 1
    li2 = q.retriever.late_interaction
    with pytest.raises(ValueError, match="max_index_bytes"):
        q.vector_store.token_index()
    assert li2.doc_forwards == 0
    q.vector_store.max_index_bytes = need
    assert q.vector_store.token_index().n_tokens == before[0]
