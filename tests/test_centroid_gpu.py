"""GPU: the pruned centroid-interaction first stage over a res2 index -- crs::centroid_scores against fp64 and its
bitmap against its own stored scores, crs::centroid_maxsim_topk bit for bit against a numpy restatement of A and of the tie rule,
the refusals, and first_stage 'centroid' through a store."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROW_LENS = tuple([300, 0, 1, 63, 64, 65, 0] + [(7 * i) % 23 for i in range(123)])      # 130 rows: three items, the last ragged


def _unit16(rng, n, dimp):
    x = rng.standard_normal((n, dimp), dtype=np.float32)
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float16)


def _q_lens(nq, lq_max):
    q_len = np.asarray([(lq_max, 1, max(1, lq_max // 2), max(1, lq_max - 1))[i % 4] for i in range(nq)], dtype=np.int32)
    q_len[nq // 2] = 0 if nq > 1 else q_len[0]
    return q_len


def _bit(keep, cid):
    """keep int32 [nq, words] -> bool [nq, len(cid)] for cids inside the table"""
    return ((keep.view(np.uint32)[:, cid >> 5] >> (cid & 31).astype(np.uint32)) & 1).astype(bool)


@pytest.mark.parametrize("nq", [1, 9])
@pytest.mark.parametrize("lq_max", [1, 17, 64])
@pytest.mark.parametrize("k_cent", [16, 272])      # one bitmap word; nine with a ragged last one
@pytest.mark.parametrize("dimp", [32, 64, 96, 128])
def test_scores_against_fp64_and_the_bitmap_against_the_scores(cuda, dimp, k_cent, lq_max, nq):
    import torch
    from rag import _native as nat
    rng = np.random.default_rng(dimp + k_cent + 7 * lq_max + nq)
    q16, cent, q_len = _unit16(rng, nq * lq_max, dimp).reshape(nq, lq_max, dimp), _unit16(rng, k_cent, dimp), _q_lens(nq, lq_max)
    q16[0, 0] *= np.float16(2.0 ** -12)                        # scores in fp16's subnormal range
    t = lambda a: torch.from_numpy(a).to(cuda)
    lqp = -(-lq_max // 8) * 8
    ref = np.einsum("qid,cd->qci", q16.astype(np.float64), cent.astype(np.float64))
    tol = 2.0 ** -11 * np.abs(ref) + dimp * 2.0 ** -23 * float(np.abs(q16).max()) * float(np.abs(cent).max()) + 2.0 ** -25
    live = np.arange(lqp)[None, :] < q_len[:, None]            # [nq, lqp]
    rowmax = None
    for thr in (-np.inf, None):
        thr = float(np.median(rowmax[q_len > 0])) if thr is None else thr      # the second pass splits the centroids
        s16, keep = nat.centroid_scores(t(q16), t(q_len), t(cent), thr)
        s16, keep = s16.cpu().numpy(), keep.cpu().numpy()
        assert s16.shape == (nq, k_cent, lqp) and keep.shape == (nq, -(-k_cent // 32))
        err = np.abs(s16[:, :, :lq_max].astype(np.float64) - ref)
        ok = live[:, None, :lq_max]
        print(f"centroid_scores dimp {dimp} K {k_cent} lq {lq_max} nq {nq}: largest |error| / tolerance {np.max((err / tol)[np.broadcast_to(ok, err.shape)]):.3f}")
        assert np.all((err <= tol) | ~ok)
        dead = np.broadcast_to(~live[:, None, :], s16.shape)
        assert np.all(s16.view(np.uint16)[dead] == 0)          # +0 past a query's length and in the padding columns
        rowmax = np.where(live[:, None, :], s16.astype(np.float32), -np.inf).max(2)      # [nq, K], -inf for an empty query
        want = (rowmax >= np.float32(thr)) & (q_len[:, None] > 0)
        assert np.array_equal(_bit(keep, np.arange(k_cent)), want)
        assert not _bit(keep, np.arange(k_cent, keep.shape[1] * 32)).any()      # bits past K
    assert 0 < want[q_len > 0].mean() < 1


def _expected(s_rows, keep, q_len, cid, offsets, k_cent, first, count, k):
    """The header's A in numpy -- fp16 maximum from +0, fp32 sums of 8 ascending, then of the chunks ascending -- and the tie rule.
    s_rows fp16 [nq, n_tokens, lqp]: the stored score rows of each token's centroid (anything where the cid is outside the table)."""
    nq, _, lqp = s_rows.shape
    inside = (cid >= 0) & (cid < k_cent)
    kept = _bit(keep, np.where(inside, cid, 0)) & inside[None, :]
    out_s, out_r = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        if q_len[q] == 0:
            continue
        found = []
        for r in range(first, first + count):
            lo, hi = offsets[r], offsets[r + 1]
            if hi <= lo:
                continue
            m = np.zeros(lqp, np.float16)
            for j in range(lo, hi):
                if kept[q, j]:
                    m = np.maximum(m, s_rows[q, j])
            m = np.where(np.arange(lqp) < q_len[q], m, 0).astype(np.float32).reshape(-1, 8)
            part = np.zeros(lqp // 8, np.float32)
            for i in range(8):
                part = part + m[:, i]
            total = np.float32(0)
            for c in range(lqp // 8):
                total = np.float32(total + part[c])
            found.append((-total, r))
        found.sort()
        for slot, (neg, r) in enumerate(found[:k]):
            out_s[q, slot], out_r[q, slot] = -neg, r
    return out_s, out_r


@functools.lru_cache(maxsize=None)
def _sweep_case(k_cent, dimp, lq_max, nq, lens):
    rng = np.random.default_rng(k_cent % 1000 + nq)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cid = rng.integers(0, k_cent, int(offsets[-1])).astype(np.int32)
    cid[-5:] = k_cent - 1 - np.arange(5)                       # the last words of the bitmap
    cid[[5, 301]] = [-1, k_cent]                               # outside the table: skipped
    return SimpleNamespace(q16=_unit16(rng, nq * lq_max, dimp).reshape(nq, lq_max, dimp), q_len=_q_lens(nq, lq_max),
                           cent=_unit16(rng, k_cent, dimp), cid=cid, offsets=offsets)


def _check_sweep(cuda, case, thr, k, first=0, count=None, split=False):
    import torch
    from rag import _native as nat
    t = lambda a: torch.from_numpy(a).to(cuda)
    k_cent, lq_max, n_rows = len(case.cent), case.q16.shape[1], len(case.offsets) - 1
    count = n_rows - first if count is None else count
    q16, q_len, cent, cid = t(case.q16), t(case.q_len), t(case.cent), t(case.cid)
    s16, keep = nat.centroid_scores(q16, q_len, cent, thr)
    if split:                                                  # the median of the largest scores: about half the centroids stay
        thr = float(s16.float().amax(2)[t(case.q_len > 0)].median())
        s16, keep = nat.centroid_scores(q16, q_len, cent, thr)
    index = SimpleNamespace(cid=cid, n_tokens=len(case.cid), offsets_dev=t(case.offsets), n_rows=n_rows)
    got_s, got_r = nat.centroid_maxsim_topk(s16, keep, q_len, lq_max, index, k, row_first=first, row_count=count)
    s_rows = s16[:, cid.clamp(0, k_cent - 1).long(), :].cpu().numpy()
    want_s, want_r = _expected(s_rows, keep.cpu().numpy(), case.q_len, case.cid, case.offsets, k_cent, first, count, k)
    assert np.array_equal(got_r.cpu().numpy(), want_r)
    assert got_s.cpu().numpy().tobytes() == want_s.tobytes()
    return want_s, want_r


@pytest.mark.parametrize("thr", [-np.inf, "split", 2.0])
@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("nq", [1, 8, 9])
def test_sweep_is_the_formula_bit_for_bit(cuda, nq, k, thr):
    case = _sweep_case(272, 32, 17, nq, ROW_LENS)              # lqp 24: three chunks in slots of four lanes
    want_s, want_r = _check_sweep(cuda, case, -np.inf if thr == "split" else thr, k, split=thr == "split")
    if thr == 2.0:                                             # nothing is kept: every score is 0 and the order is the tie rule
        nonempty = np.flatnonzero(np.diff(case.offsets) > 0)[:k]
        assert np.all(want_s[case.q_len > 0][:, :len(nonempty)] == 0) and np.all(want_r[case.q_len > 0][:, :len(nonempty)] == nonempty)


@pytest.mark.parametrize("lq_max", [1, 9, 64])                 # one, two and eight chunks a score row
def test_sweep_at_every_chunk_count(cuda, lq_max):
    _check_sweep(cuda, _sweep_case(64, 64, lq_max, 3, ROW_LENS), -np.inf, 10, split=True)


def test_sweep_row_range_with_fewer_rows_than_k(cuda):
    want_s, want_r = _check_sweep(cuda, _sweep_case(272, 32, 17, 9, ROW_LENS), -np.inf, 64, first=3, count=40)
    assert np.all(want_r[0] < 43) and (want_r[0] >= 0).sum() == (np.diff(_sweep_case(272, 32, 17, 9, ROW_LENS).offsets)[3:43] > 0).sum() < 64


def test_sweep_with_one_query_per_workgroup(cuda):
    """2^20 centroids: a query's bitmap is 128 KB, so the plan serves one query per workgroup (a 64 MB table, 32 MB of scores)."""
    from rag import _native as nat
    assert " Qg=1 " in nat.centroid_maxsim_topk_plan_describe(2, 8, 1 << 20, 10, 130)
    _check_sweep(cuda, _sweep_case(1 << 20, 32, 8, 2, ROW_LENS), -np.inf, 10, split=True)


@pytest.mark.parametrize("bad, word", [(dict(lq_max=65), "lq_max"), (dict(dimp=48), "dimp"), (dict(k=65), "k must"), (dict(K=15), "n_centroids"),
                                       (dict(s16=2), "aligned"), (dict(ws_bytes=16), "workspace too small")])
def test_refusals(cuda, bad, word):
    """CRS_EINVAL with a message naming the argument, through the C ABI (the torch ops check the same limits ahead of it)."""
    import torch
    from rag import _native as nat
    lib, buf = nat.load(), torch.zeros(8192, dtype=torch.uint8, device=cuda)
    p = buf.data_ptr()
    a = dict(lq_max=4, dimp=32, k=4, K=16, s16=0, ws_bytes=nat.centroid_maxsim_topk_workspace_bytes(2, 4, 2))
    assert a["ws_bytes"] <= 8192 - 1024
    a.update(bad)
    if word != "dimp":                                         # the sweep never sees the vectors
        rc_ = lib.crs_centroid_maxsim_topk(p + a["s16"], p, p, 2, a["lq_max"], a["K"], p, p, 2, 8, 0, 2, a["k"], p + 1024, a["ws_bytes"], p, p, None)
        assert rc_ != 0 and word in lib.crs_last_error().decode()
    if word in ("lq_max", "dimp", "n_centroids", "aligned"):
        assert lib.crs_centroid_scores(p, p, 2, a["lq_max"], p, a["K"], a["dimp"], 0.5, p + a["s16"], p, None) != 0
        assert word in lib.crs_last_error().decode()


def test_every_document_a_candidate_gives_the_scan_lists(cuda):
    """60 documents and 64 candidates: whatever the centroid scores say every document is scored exactly, so 'centroid' returns
    what 'scan' returns -- ids, score and rerank_score."""
    import _late_cases as lc
    from test_late_interaction_gpu import LI_CFG, _pipeline
    docs, questions, lists = lc.corpus(60), lc.queries(9), {}
    for stage in ("scan", "centroid"):
        p = _pipeline("cs-" + stage, docs, {"late_interaction": dict(LI_CFG, token_dtype="res2", centroids=64, first_stage=stage),
                                            "similarity_threshold": -1.0})
        lists[stage] = [[(c["chunk_id"], c["score"], c["rerank_score"]) for c in chunks] for chunks in p.retriever.retrieve_batch(questions)]
    assert all(len(x) == 5 for x in lists["scan"]) and lists["centroid"] == lists["scan"]


def test_scores_through_the_store_are_exact(cuda):
    """300 documents: every returned score is score_rows' for its row bit for bit, best first, and the rows are among the sweep's 64."""
    import _late_cases as lc
    from rag import _native as nat
    from test_late_interaction_gpu import LI_CFG, _pipeline
    questions = lc.queries(9)
    p = _pipeline("cs-store", lc.corpus(300), {"late_interaction": dict(LI_CFG, token_dtype="res2", centroids=64, first_stage="centroid")})
    store, li = p.vector_store, p.retriever.late_interaction
    s, r, q_len = store.late_rows(questions, 10, candidates=64, threshold=0.5)
    assert r.shape == (9, 10) and np.all(r >= 0) and np.all(np.diff(s.astype(np.float64), axis=1) <= 0)
    assert s.tobytes() == li.score_rows(questions, r, store).cpu().numpy().tobytes()
    index = store.token_index()
    q16, ql = li.encode_queries_device(questions)
    s16, keep = nat.centroid_scores(q16, ql, index.codec.centroids, 0.5)
    cand = nat.centroid_maxsim_topk(s16, keep, ql, q16.shape[1], index, 64)[1].cpu().numpy()
    assert all(set(r[a]) <= set(cand[a]) for a in range(9))
    assert store.search_late_batch(questions, top_k=10, candidates=64)["rows"] == r.tolist()
    with pytest.raises(ValueError, match="candidates"):
        store.late_rows(questions, 10, candidates=9)
    q = _pipeline("cs-fp16", lc.corpus(8), {"late_interaction": dict(LI_CFG, first_stage="scan")})
    with pytest.raises(ValueError, match="token_dtype"):
        q.vector_store.late_rows(questions, 5, candidates=64)
