"""GPU: VectorStore in the spaces 'ip' and 'l2' (csrc/space.hip, rag/indexing.py, rag/_search.py) against fp64.

Shapes: d in {100, 128, 384} (fp16 rows pad to 128 / 128 / 384 under ip and, one coordinate longer, to 128 / 256 / 512 under l2), 4096 + 37 rows
(several tiles, a ragged tail), 1 / 5 / 70 queries (70 leaves the 64-query kernels), top_k 1 / 10 / 40 / 100 (100: the partitioned
over-fetch), fp16 and int8 slabs, row norms spread over 8 x.

Ids follow the near-tie rule of tests/topk_check.py::topk_errors on the metric (tests/_space_ref.py::topk_errors): rows may change
places only where their fp64 metric values differ by less than a bound DERIVED from the arithmetic (_space_ref.swap_tol):
2 (d' + 4) 2^-24 |q| R for ip, 2 (d' + 4) 2^-24 4 R^2 |(q / R, -1)| for l2.  The queries are chosen so that the fp64 gap at every
tested k exceeds that bound, and the test asserts so before it looks at a result.  Distances: within (d + 2) 2^-24 sum |q_i x_i|
(ip) / (d + 2) 2^-24 sum (q_i - x_i)^2 (l2) of fp64.  int8 stores run with refine_exact: True ('auto' leaves int8 empirical)."""
import functools
import json
import os

import numpy as np
import pytest

import _space_ref as sr

pytestmark = pytest.mark.gpu

N = 4096 + 37
DIMS = (100, 128, 384)
NQS = (1, 5, 70)
KS = (1, 10, 40, 100)


@functools.lru_cache(maxsize=None)
def _chunks(n, first=0):
    from rag.chunking import Chunk
    return [Chunk(text=f"chunk text {i}", chunk_id=f"c_{i}", start_char=0, end_char=1, page_number=int(i % 2) + 1, section=None, tokens=3)
            for i in range(first, first + n)]


def _rows_of(res):
    return [[int(i[2:]) for i in ids] for ids in res["ids"]]


@functools.lru_cache(maxsize=None)
def _rows(d):
    x = sr.make_rows(N, d, seed=7 + d)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _case(d, space):
    """(rows, R, 70 queries, fp64 metric [70, N], swap bound [70]): computed once, shared, read-only."""
    x = _rows(d)
    R = sr.norm_scale_for(sr.row_norm_max(x))
    q = sr.pick_queries(x, space, R, max(NQS), KS, seed=11 + d)
    metric, tol = sr.metric64(q, x, space), sr.swap_tol(q, d, space, R)
    for a in (q, metric, tol):
        a.setflags(write=False)
    return x, R, q, metric, tol


def _store(space, dtype, **cfg):
    from rag.indexing import VectorStore
    return VectorStore({"space": space, "index_dtype": dtype, "refine_exact": True if dtype == "int8" else "auto", **cfg})


def _check_lists(res, q, x, space, k, metric, tol, tag):
    """ids by the near-tie rule, distances against fp64, list order (distance asc, row asc)."""
    rows = np.asarray(_rows_of(res), dtype=np.int64)
    assert rows.shape == (len(q), k), tag
    assert sr.topk_errors(rows, metric, k, tol) == {}, tag
    for r in range(len(q)):
        got = np.asarray(res["distances"][r], dtype=np.float64)
        ref = sr.metric64_rows(q[r], x[rows[r]], space)
        bound = sr.distance_tol(q[r], x[rows[r]], space)
        assert (np.abs(got - ref) <= bound).all(), (tag, r, np.abs(got - ref).max(), bound.min())
        assert all(got[a] < got[a + 1] or (got[a] == got[a + 1] and rows[r, a] < rows[r, a + 1]) for a in range(k - 1)), (tag, r)


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("space", sr.SPACES)
def test_ids_distances_and_exactness(cuda, space, d, dtype):
    from rag import _native as nat
    x, R, q, metric, tol = _case(d, space)
    assert sr.row_norm_max(x) / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).min() >= 8.0
    # the tolerance must not be what makes the test pass: at every k the fp64 gap exceeds the bound, for every query
    assert (sr.kth_gaps(metric, KS) > tol[:, None]).all()
    store = _store(space, dtype)
    store.create_index(_chunks(N), x.copy())           # (the shared arrays are read-only; the store takes a copy)
    col = store.collection
    sdim = d + (space == "l2")
    assert col.metadata == {"hnsw:space": space} and store.get_stats()["metadata"] == {"hnsw:space": space}
    assert col.dim == d and col.sdim == sdim and col.pdim == nat.padded_dim(sdim, col.slab_type) and col.shadow.shape[1] == sdim
    assert col.shards[0].norm_scale_host == R == float(col.shards[0].norm_scale.item())
    if dtype == "fp16":
        assert col.pdim == {("ip", 100): 128, ("ip", 128): 128, ("ip", 384): 384, ("l2", 100): 128, ("l2", 128): 256, ("l2", 384): 512}[space, d]
    some = np.array([0, 1, 2, 63, 64, 4095, 4096, N - 1])
    assert np.array_equal(store.rows_f32(some).view(np.uint32), x[some].view(np.uint32))      # the caller's vectors, bit for bit
    for nq in NQS:
        for k in KS:
            res = store.search_batch(q[:nq].copy(), top_k=k)
            tag = (space, d, dtype, nq, k)
            _check_lists(res, q[:nq], x, space, k, metric[:nq], tol[:nq], tag)
            ex = store.last_exactness
            assert ex["mode"] == "certificate" and ex["queries"] == nq and ex["unproven"] == 0, (tag, ex)
            assert ex["certified"] + ex["escalated"] == nq
    one = store.search(q[3].copy(), top_k=10)
    assert one["ids"] == [store.search_batch(q[3:4].copy(), top_k=10)["ids"][0]]
    with pytest.raises(ValueError, match="top_k"):
        store.search_batch(q[:1].copy(), top_k=2000)
    with pytest.raises(ValueError, match="dimension"):
        store.search_batch(np.zeros((1, d + 1), dtype=np.float32), top_k=1)


@pytest.mark.parametrize("d", [100, 384])
def test_planted_long_row_outranks_short_row_under_ip(cuda, d):
    """Per query a SHORT row at cosine 0.95 and a LONG row at cosine 0.6: cosine returns the short one, ip must return the long one
    (its inner product is 4 x the short one's).  On a store that normalises every row the ip list cannot hold the long row first."""
    from rag.indexing import VectorStore
    rng = np.random.default_rng(5)
    base = _rows(d)
    nq = 5
    q = rng.standard_normal((nq, d))
    q /= np.sqrt((q * q).sum(axis=1, keepdims=True))
    planted = []
    for r in range(nq):
        for cos, norm in ((0.95, 0.3), (0.6, 1.9)):
            w = rng.standard_normal(d)
            w -= (w @ q[r]) * q[r]
            w /= np.sqrt(w @ w)
            planted.append(norm * (cos * q[r] + np.sqrt(1 - cos * cos) * w))
    x = np.concatenate([base, np.asarray(planted)]).astype(np.float32)
    q = q.astype(np.float32)
    short, long_ = N + 2 * np.arange(nq), N + 2 * np.arange(nq) + 1
    ip64, cos64 = sr.metric64(q, x, "ip"), None
    xn = x.astype(np.float64) / np.sqrt((x.astype(np.float64) ** 2).sum(axis=1, keepdims=True))
    cos64 = q.astype(np.float64) @ xn.T
    assert (np.argmin(ip64, axis=1) == long_).all() and (np.argmax(cos64, axis=1) == short).all()       # the fp64 truth, first
    assert (cos64[np.arange(nq), long_] < cos64[np.arange(nq), short]).all()
    chunks = _chunks(len(x))
    ip = VectorStore({"space": "ip"})
    ip.create_index(chunks, x)
    cosine = VectorStore({})
    cosine.create_index(chunks, x)
    for k in (1, 10):
        got_ip, got_cos = _rows_of(ip.search_batch(q, top_k=k)), _rows_of(cosine.search_batch(q, top_k=k))
        for r in range(nq):
            assert got_ip[r][0] == long_[r] and long_[r] in got_ip[r], (k, r, got_ip[r])
            assert got_cos[r][0] == short[r], (k, r, got_cos[r])
    assert cosine.collection.metadata == {"hnsw:space": "cosine"}


@pytest.mark.parametrize("space", sr.SPACES)
def test_equal_distances_come_lower_row_first(cuda, space):
    rng = np.random.default_rng(2)
    x = rng.standard_normal((60, 100)).astype(np.float32)
    x[7], x[41], x[40] = x[3], x[3], x[12]
    store = _store(space, "fp16")
    store.create_index(_chunks(60), x)
    q = (x[3] * 0.9 + 0.01).astype(np.float32)[None, :]
    for k in (5, 60):
        res = store.search_batch(q, top_k=k)
        rows, dist = _rows_of(res)[0], res["distances"][0]
        assert rows[:3] == [3, 7, 41] and dist[0] == dist[1] == dist[2]
        at = rows.index(12) if 12 in rows else None
        assert at is None or k < 60 or (rows[at + 1] == 40 and dist[at] == dist[at + 1])
        assert sorted(dist) == dist


def _state(store):
    import torch
    sh = store.collection.shards[0]
    torch.cuda.synchronize()
    out = {"slab": sh.slab[: sh.n].cpu(), "shadow": sh.shadow[: sh.n].cpu(), "norm_scale": sh.norm_scale.cpu(), "R": sh.norm_scale_host}
    if sh.scales is not None:
        out["scales"] = sh.scales[: sh.n].cpu()
    return out


def _same_state(a, b, tag):
    import torch
    assert a.keys() == b.keys(), tag
    for key in a:
        if key == "R":
            assert a[key] == b[key], (tag, key)
        else:        # byte for byte (views as integers: -0.0 and NaN would not hide)
            ia = a[key].view(torch.int32 if a[key].dtype == torch.float32 else torch.int16 if a[key].dtype == torch.float16 else torch.int8)
            ib = b[key].view(ia.dtype)
            assert torch.equal(ia, ib), (tag, key)


def _norms_to(x, top):
    """x with its norms scaled into (0, top]"""
    n = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    return (x * (top / n.max())).astype(np.float32)


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
@pytest.mark.parametrize("space", sr.SPACES)
def test_rescale_equals_a_fresh_store(cuda, space, dtype):
    d, na, nb = 100, 1500 + 13, 37
    full = _rows(d)
    a = _norms_to(full[:na], 1.5)
    b = _norms_to(full[na:na + nb], 1.2)
    b[5] = (b[5].astype(np.float64) * (5.0 / np.sqrt((b[5].astype(np.float64) ** 2).sum()))).astype(np.float32)      # one row of norm 5
    ab = np.concatenate([a, b])
    rng = np.random.default_rng(17)
    q = (rng.standard_normal((9, d)) * 0.1).astype(np.float32)
    evens = {"page_number": 1}

    grown = _store(space, dtype)
    grown.create_index(_chunks(na), a)
    assert grown.collection.shards[0].norm_scale_host == 2.0
    before = grown.search_batch(q, top_k=10, where=evens)              # fills the filter cache under R = 2
    grown.create_index(_chunks(nb, first=na), b)
    fresh = _store(space, dtype)
    fresh.create_index(_chunks(na + nb), ab)
    assert fresh.collection.shards[0].norm_scale_host == 8.0
    _same_state(_state(grown), _state(fresh), "add")
    for where in (None, evens):
        assert grown.search_batch(q, top_k=10, where=where) == fresh.search_batch(q, top_k=10, where=where)
    assert before["ids"] != [[]] * len(q)

    # the same through update: the largest norm arrives in place
    calm = ab.copy()
    calm[na + 5] = b[4]
    upd = _store(space, dtype)
    upd.create_index(_chunks(na + nb), calm)
    assert upd.collection.shards[0].norm_scale_host == 2.0
    upd.search_batch(q, top_k=10, where=evens)
    upd.update([f"c_{na + 5}"], embeddings=ab[na + 5][None, :])
    _same_state(_state(upd), _state(fresh), "update")
    assert upd.search_batch(q, top_k=10) == fresh.search_batch(q, top_k=10)
    assert upd.search_batch(q, top_k=10, where=evens) == fresh.search_batch(q, top_k=10, where=evens)

    # delete leaves R alone; the results stay those of the fp64 metric over the survivors
    assert upd.delete(ids=[f"c_{na + 5}"]) == 1
    assert upd.collection.shards[0].norm_scale_host == 8.0 == float(upd.collection.shards[0].norm_scale.item())
    keep = np.delete(np.arange(na + nb), na + 5)
    metric = sr.metric64(q, ab[keep], space)
    res = upd.search_batch(q, top_k=10)
    got = np.asarray([[int(np.searchsorted(keep, r)) for r in rows] for rows in _rows_of(res)])
    assert sr.topk_errors(got, metric, 10, sr.swap_tol(q, d, space, 8.0)) == {}
    for r in range(len(q)):
        ref = sr.metric64_rows(q[r], ab[keep][got[r]], space)
        assert (np.abs(np.asarray(res["distances"][r]) - ref) <= sr.distance_tol(q[r], ab[keep][got[r]], space)).all()
    if dtype == "fp16":
        assert upd.last_exactness["unproven"] == 0

    # a vector without a finite norm is refused before anything is written
    bad = ab[:3].copy()
    bad[1, 7] = np.inf
    state = _state(fresh)
    with pytest.raises(ValueError, match="non-finite"):
        fresh.create_index(_chunks(3, first=na + nb), bad)
    with pytest.raises(ValueError, match="non-finite"):
        fresh.update(["c_0"], embeddings=bad[1:2])
    assert fresh.collection.count() == na + nb
    _same_state(_state(fresh), state, "refused")


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
@pytest.mark.parametrize("space", sr.SPACES)
def test_where_filter(cuda, space, dtype):
    d, k = 128, 10
    x, R, q, _, _ = _case(d, space)
    q = q[:5].copy()
    store = _store(space, dtype)
    store.create_index(_chunks(N), x.copy())
    allowed = np.arange(0, N, 2)                                       # page_number 1: the even rows
    res = store.search_batch(q, top_k=k, where={"page_number": 1})
    rows = np.asarray(_rows_of(res))
    assert (rows % 2 == 0).all()
    metric = sr.metric64(q, x[allowed], space)
    assert sr.topk_errors(rows // 2, metric, k, sr.swap_tol(q, d, space, R)) == {}
    for r in range(len(q)):
        got = np.asarray(res["distances"][r])
        assert (np.abs(got - sr.metric64_rows(q[r], x[rows[r]], space)) <= sr.distance_tol(q[r], x[rows[r]], space)).all()
        assert (np.diff(got) >= 0).all()
    assert store.last_exactness["unproven"] == 0
    assert store.search_batch(q, top_k=k, where={"page_number": 3})["ids"] == [[] for _ in range(len(q))]


@pytest.mark.parametrize("space", sr.SPACES)
def test_persistence_round_trip(cuda, space, tmp_path):
    from rag.indexing import VectorStore
    d = 100
    x = _rows(d)[:900]
    a, b = _norms_to(x[:600], 1.5), _norms_to(x[600:], 5.0)
    q = (np.random.default_rng(3).standard_normal((6, d)) * 0.2).astype(np.float32)
    cfg = {"space": space, "persist_directory": str(tmp_path), "collection_name": "spaces"}
    store = VectorStore(cfg)
    store.create_index(_chunks(600), a)
    store.create_index(_chunks(300, first=600), b)                     # grows R from 2 to 8: the files are rewritten under the new scale
    meta = json.load(open(os.path.join(str(tmp_path), "spaces.meta.json")))
    assert meta["space"] == space and meta["norm_scale"] == 8.0 and meta["dim"] == d and meta["n"] == 900
    want = store.search_batch(q, top_k=10)
    again = VectorStore(cfg)
    assert again.collection.count() == 900 and again.collection.metadata == {"hnsw:space": space}
    assert again.collection.shards[0].norm_scale_host == 8.0
    _same_state(_state(again), _state(store), "reopened")
    assert again.search_batch(q, top_k=10) == want
    again.create_index(_chunks(5, first=900), _norms_to(x[:5], 1.0))   # appends continue the files
    assert VectorStore(cfg).search_batch(q, top_k=10) == again.search_batch(q, top_k=10)
    for other in ({"ip", "l2", "cosine"} - {space}):
        with pytest.raises(ValueError, match="space"):
            VectorStore({**cfg, "space": other})
    # a cosine store's header is what it was
    plain = VectorStore({"persist_directory": str(tmp_path), "collection_name": "plain"})
    plain.create_index(_chunks(600), a)
    header = json.load(open(os.path.join(str(tmp_path), "plain.meta.json")))
    assert sorted(header) == ["dim", "docs_bytes", "format", "index_dtype", "n", "pdim", "row_err_max", "shadow"]
    with pytest.raises(ValueError, match="space"):
        VectorStore({"persist_directory": str(tmp_path), "collection_name": "plain", "space": "ip"})


def test_kernels_against_numpy(cuda):
    import torch
    from rag import _native as nat
    d = 100
    x = _rows(d)
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    top = nat.rows_norm_max(xd)
    assert abs(top - sr.row_norm_max(x)) <= 1e-6 * top
    bad = xd[:70].clone()
    bad[69, 3] = float("nan")
    assert nat.rows_norm_max(bad) == float("inf")
    R = torch.full((1,), 2.0, device=cuda)
    q = _case(d, "l2")[2][:7]
    qd = torch.from_numpy(np.ascontiguousarray(q)).to(cuda)
    for space, code in (("ip", nat.SPACE_IP), ("l2", nat.SPACE_L2)):
        for st in (nat.SLAB_F16, nat.SLAB_I8):
            q32, q16 = nat.queries_to_space(qd, code, st, R)
            sdim = d + (space == "l2")
            assert q32.shape == (7, sdim) and q16.shape == (7, nat.padded_dim(sdim, st))
            # |coordinate| <= 1; the sum of squares (two fmas and six butterfly adds per lane), its root, the division: < 8 roundings
            assert np.abs(q32.cpu().numpy().astype(np.float64) - sr.queries(q, space, 2.0)).max() <= 8 * sr.U
            assert torch.equal(q16[:, :sdim], q32.half()) and not q16[:, sdim:].any()


LARGE_N = 1100
LARGE_KS = (65, 128, 1000, 1024)


@functools.lru_cache(maxsize=None)
def _large_case(d, space):
    """1100 rows and 70 queries whose fp64 gaps at k = 65, 128, 1000, 1024 exceed twice the swap bound (at 4133 rows and d = 384
    no such queries exist: keep n = 1100)."""
    x = sr.make_rows(LARGE_N, d, seed=7 + d)
    q = sr.pick_queries(x, space, 2.0, 70, LARGE_KS, seed=11 + d)
    metric, tol = sr.metric64(q, x, space), sr.swap_tol(q, d, space, 2.0)
    for a in (x, q, metric, tol):
        a.setflags(write=False)
    return x, q, metric, tol


@pytest.mark.parametrize("d", [100, 384])
@pytest.mark.parametrize("space", sr.SPACES)
def test_top_k_65_to_1024(cuda, space, d):
    """The partitioned over-fetch and its certificate (csrc/large_k.hip) under ip / l2, and crs_space_distances' LDS ranking at
    k up to 1024, through the store."""
    x, q, metric, tol = _large_case(d, space)
    assert sr.norm_scale_for(sr.row_norm_max(x)) == 2.0
    assert (sr.kth_gaps(metric, LARGE_KS) > tol[:, None]).all()      # the tolerance is not what makes the test pass
    store = _store(space, "fp16")
    store.create_index(_chunks(LARGE_N), x.copy())
    assert store.collection.shards[0].norm_scale_host == 2.0
    for nq in NQS:
        for k in LARGE_KS:
            res = store.search_batch(q[:nq].copy(), top_k=k)
            tag = (space, d, nq, k)
            _check_lists(res, q[:nq], x, space, k, metric[:nq], tol[:nq], tag)
            ex = store.last_exactness
            # the escalation list holds more rows than the store has: nothing can stay unproven here
            assert ex["mode"] == "certificate" and ex["queries"] == nq and ex["unproven"] == 0, (tag, ex)
            assert ex["certified"] + ex["escalated"] == nq, (tag, ex)


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
@pytest.mark.parametrize("space", sr.SPACES)
def test_top_k_above_the_row_count(cuda, space, dtype):
    d, n = 100, 60
    x = sr.make_rows(n, d, seed=23)
    q = sr.pick_queries(x, space, 2.0, 5, (10,), seed=29)
    metric, tol = sr.metric64(q, x, space), sr.swap_tol(q, d, space, 2.0)
    store = _store(space, dtype)
    store.create_index(_chunks(n), x)
    for k in (61, 100, 1024):
        res = store.search_batch(q, top_k=k)
        # all 60 rows, each once, in metric order (up to the near-tie bound) with ascending distances: no -1, no inf
        _check_lists(res, q, x, space, n, metric, tol, (space, dtype, k))
        for r in range(len(q)):
            assert sorted(_rows_of(res)[r]) == list(range(n)) and np.isfinite(res["distances"][r]).all(), (space, dtype, k, r)


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
@pytest.mark.parametrize("space,d", [("l2", 1), ("l2", 127), ("l2", 1023), ("ip", 1), ("ip", 1024)])
def test_edge_dimensions(cuda, space, d, dtype):
    n, k = 300, 10
    x = sr.make_rows(n, d, seed=7 + d)
    q = sr.pick_queries(x, space, 2.0, 5, (k,), seed=11 + d)
    metric, tol = sr.metric64(q, x, space), sr.swap_tol(q, d, space, 2.0)
    assert (sr.kth_gaps(metric, (k,)) > tol[:, None]).all()
    store = _store(space, dtype)
    store.create_index(_chunks(n), x)
    col = store.collection
    assert col.shards[0].norm_scale_host == 2.0 and col.dim == d and col.sdim == d + (space == "l2")
    _check_lists(store.search_batch(q, top_k=k), q, x, space, k, metric, tol, (space, d, dtype))


def test_l2_refuses_1024_dimensions(cuda):
    x = sr.make_rows(8, 1024, seed=3)
    for how in ("create_index", "upsert"):           # the dimension arrives with the first rows, whichever call brings them
        store = _store("l2", "fp16")
        with pytest.raises(ValueError, match="too large for space 'l2'"):
            getattr(store, how)(_chunks(8), x)
        assert store.collection is None or store.collection.count() == 0
    ok = _store("ip", "fp16")
    ok.create_index(_chunks(8), x)
    assert ok.collection.count() == 8


@pytest.mark.parametrize("space", sr.SPACES)
def test_rows_at_a_power_of_two_norm(cuda, space):
    """R must cover the TRUE norm of every row (every stored row has norm <= 1, the premise of the certificate's
    bound).  The first planted row has its mass in lane 0 of the norm kernel, whose fp32 chain returns exactly 2.0 for a true
    norm of 2 (1 + 3.7e-8): a scale chosen from the fp32 norm alone is R = 2 and stores a row of norm 1 + 3.7e-8."""
    import _space_build_ref as br
    d = 384
    lane0 = br.lane0_power_of_two_row(d)
    axis = np.zeros(d, np.float32)
    axis[5] = 2.0
    rng = np.random.default_rng(13)
    rnd = rng.standard_normal((50, d))
    rnd = (rnd * (rng.uniform(0.2, 0.99, size=(50, 1)) / np.sqrt((rnd * rnd).sum(axis=1, keepdims=True)))).astype(np.float32)
    x = np.concatenate([rnd, lane0[None, :], axis[None, :]])
    norms = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    assert norms[:50].max() < 1.0 and norms[50] > 2.0 and norms[51] == 2.0
    store = _store(space, "fp16")
    store.create_index(_chunks(50), rnd)                         # R = 1
    store.create_index(_chunks(2, first=50), x[50:])             # the planted rows arrive: a rescale
    sh = store.collection.shards[0]
    R = sh.norm_scale_host
    assert R == float(sh.norm_scale.item())
    rows = sh.shadow[: sh.n].cpu().numpy().astype(np.float64)
    assert rows.shape == (52, d + (space == "l2"))
    if space == "ip":
        worst = np.sqrt((rows * rows).sum(axis=1)).max()
        assert worst <= 1.0, f"|u| - 1 = {worst - 1.0:.3e}"
    else:
        v = np.sqrt((rows[:, :d] ** 2).sum(axis=1)).max()
        assert v <= 0.5, f"|v| - 1/2 = {v - 0.5:.3e}"
        assert (rows * rows).sum(axis=1).max() <= 0.25 + 1.0 / 16
    assert R >= norms.max(), (R, norms.max())                    # R covers the fp64 norm of every row ever given
    assert np.array_equal(store.rows_f32(np.arange(52)).view(np.uint32), x.view(np.uint32))
    assert R == 4.0                                              # a norm of exactly 2^e gets R = 2^(e + 1): correct and harmless


def test_retriever_on_an_ip_store(cuda):
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    words = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine similarity "
             "vector index chunk context answer question compression memory latency throughput kernel softmax bias bucket").split()
    p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny-mpnet", "device": "cuda", "batch_size": 256, "normalize": False},
                     "retrieval": {"top_k": 5, "similarity_threshold": -1.0, "rerank": False, "diversity_penalty": 0.0, "batch_queries": 64},
                     "vector_store": {"collection_name": "ip-e2e", "space": "ip"}})
    p.setup(Stub())
    model, store = p.embedding_model, p.vector_store
    assert store.space == "ip" and p.retriever.distance_metric == "ip"
    rng = np.random.default_rng(31)
    chunks = [Chunk(text=" ".join(rng.choice(words, size=int(rng.integers(4, 40)))) + f" {r}", chunk_id=f"c_{r}", start_char=0, end_char=1,
                    page_number=None) for r in range(700)]
    store.create_index(chunks, model.embed_chunks_device(chunks))
    assert store.collection.metadata == {"hnsw:space": "ip"} and store.engine_view() is None
    x = store.rows_f32(np.arange(700))                                 # the store's own vectors
    norms = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
    assert norms.max() / norms.min() > 1.001                           # not normalised
    R = store.collection.shards[0].norm_scale_host
    questions = [" ".join(rng.choice(words, size=int(rng.integers(3, 10)))) + f" {i}" for i in range(96)]
    got = p.retrieve_batch(questions)
    assert p.retriever._engine is None                                 # embed, then search_batch's search
    qb = np.asarray(model.embed(list(questions)), dtype=np.float32)
    rows = np.asarray([[int(c["chunk_id"][2:]) for c in g] for g in got])
    assert rows.shape == (96, 5)
    assert sr.topk_errors(rows, sr.metric64(qb, x, "ip"), 5, sr.swap_tol(qb, x.shape[1], "ip", R)) == {}
    for g, qv in zip(got[:8], qb[:8]):
        for c in g:
            row = x[int(c["chunk_id"][2:])][None, :]
            assert abs(c["distance"] - sr.metric64_rows(qv, row, "ip")[0]) <= sr.distance_tol(qv, row, "ip")[0]
            assert c["score"] == max(0.0, min(1.0, (c["distance"] + 2.0) / 2.0))
    for i in (0, 17, 95):
        single = p.retrieve(questions[i])
        q1 = np.asarray(model.embed(questions[i]), dtype=np.float32).reshape(1, -1)
        r1 = np.asarray([[int(c["chunk_id"][2:]) for c in single]])
        assert sr.topk_errors(r1, sr.metric64(q1, x, "ip"), 5, sr.swap_tol(q1, x.shape[1], "ip", R)) == {}
    # mmr_vectors 'device' is a cosine kernel: it falls back to the index rows, which are the caller's vectors
    p.retriever.diversity_penalty, p.retriever.mmr_vectors = 0.3, "device"
    p.retrieve_batch(questions[:4])
    assert p.retriever.last_mmr["mode"] == "host"
