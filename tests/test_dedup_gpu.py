"""GPU: the near-duplicate join (csrc/join.hip) and the store methods built on it, against fp64 (tests/_join_ref.py).

Op level: on planted data that no threshold comes within epsilon of, the two stages return EXACTLY the fp64 pair set of the shadow
rows -- at every dimension class, at row counts that straddle the 256-row tile and over partial ranges; stage 1 alone is a superset
with the right count whatever the buffer holds and writes nothing past it.  The band test plants 1024 pairs inside
[t - epsilon, t + epsilon]: only a build that verifies in fp32 classifies them as fp64 does.  Store level: near_duplicates,
deduplicate and the dedup_threshold config key against stores built from the survivors (bit-identical searches).
Every bound below comes from the number formats: epsilon is the formula under test (checked against its restatement), similarities
are within 2 d 2^-24 of fp64, and the band's exclusion zone is that same 2 d 2^-24.
"""
import json
import os

import numpy as np
import pytest

import _join_ref as ref

pytestmark = pytest.mark.gpu
T = ref.TILE
KEYS = ("ids", "documents", "metadatas", "distances")
_BUILT = {}


def _build(cuda, key, make):
    """Rows -> the device slab and shadow through the store's own build (crs::slab_append), once per data set."""
    if key not in _BUILT:
        import torch
        from rag import _native as nat
        x = make()
        n, dim = x.shape
        pdim = nat.padded_dim(dim)
        slab = torch.zeros((n, pdim), dtype=torch.float16, device=cuda)
        shadow = torch.zeros((n, dim), dtype=torch.float32, device=cuda)
        err = torch.zeros(1, dtype=torch.float32, device=cuda)
        nat.slab_append_f32(torch.from_numpy(x).to(cuda), slab, 0, nat.SLAB_F16, shadow=shadow, row_err=err)
        E = float(err.item())
        b = dict(x=x, n=n, dim=dim, pdim=pdim, slab=slab, shadow=shadow, E=E, slab_h=slab.cpu().numpy(), shadow_h=shadow.cpu().numpy(),
                 eps=nat.pairs_epsilon(E, pdim))
        b["G"] = ref.gram64(b["shadow_h"])
        true = ref.row_error_max(b["slab_h"], b["shadow_h"])                   # the tracked error covers the rows' error (the window of
        assert true - 2.0 ** -25 <= E <= 1.0002 * true + 2.0 ** -25               # tests/_slab_ref.py check_row_error)
        ref.check_epsilon(b["eps"], E, pdim)
        _BUILT[key] = b
    return _BUILT[key]


def _planted(cuda, n, dim, extras=False):
    return _build(cuda, ("planted", n, dim, extras), lambda: ref.planted_rows(n, dim, extras=extras))


def _stage1(b, thr1, a_range, b_range, cap, pad=64):
    """crs::pairs_above into sentinel-filled buffers of cap + pad slots, of which the op sees the first cap."""
    import torch
    from rag import _native as nat
    dev = b["slab"].device
    pairs = torch.full((cap + pad, 2), -7, dtype=torch.int64, device=dev)
    scores = torch.full((cap + pad,), -7.0, dtype=torch.float32, device=dev)
    count = torch.zeros(1, dtype=torch.int64, device=dev)
    nat.pairs_above(b["slab"], b["n"], b["dim"], a_range, b_range, thr1, cap, out=(pairs[:cap], scores[:cap], count))
    c = int(count.item())
    assert bool((pairs[cap:] == -7).all()) and bool((scores[cap:] == -7.0).all()), "written past cap"
    w = min(c, cap)
    assert bool((pairs[w:cap] == -7).all()) and bool((scores[w:cap] == -7.0).all()), "slots beyond the count were written"
    return pairs[:w].cpu().numpy(), scores[:w].cpu().numpy(), c, pairs[:w]


def _join(b, t, a_range=None, b_range=None, cap=1 << 16):
    """Both stages as the store runs them -> the store's dict (+ the stage 1 output)."""
    from rag import _native as nat
    a_range, b_range = a_range or (0, b["n"]), b_range or (0, b["n"])
    thr1, thr2 = nat.pairs_thresholds(t, b["eps"])
    assert thr1 <= t - b["eps"] and thr2 >= t
    pairs, scores, count, pairs_dev = _stage1(b, thr1, a_range, b_range, cap)
    assert count <= cap, "the test's buffer is too small"
    ra, rb, sims, kept = nat.pairs_verify(pairs_dev, b["shadow"], b["n"], thr2)
    k = int(kept.item())
    a, bb, s = ra[:k].cpu().numpy(), rb[:k].cpu().numpy(), sims[:k].cpu().numpy()
    order = np.lexsort((bb, a))
    return {"rows_a": a[order], "rows_b": bb[order], "similarities": s[order], "candidates": count, "epsilon": b["eps"],
            "stage1": (pairs, scores, count, cap, thr1)}


def _check(b, t, res, a_range=None, b_range=None):
    ref.check_exact_set(res, b["shadow_h"], t, a_range, b_range, G=b["G"])
    pairs, scores, count, cap, thr1 = res["stage1"]
    ref.check_stage1(pairs, scores, count, cap, b["slab_h"], b["shadow_h"], t, b["eps"], thr1, a_range, b_range)


# ---- op level against fp64 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 100, 384, 768, 1000])
def test_planted_pairs_are_exactly_the_fp64_set(cuda, dim):
    b = _planted(cuda, 300, dim, extras=True)
    assert b["n"] == 302
    ref.check_no_pair_near(b["G"], ref.THRESHOLDS, b["eps"])                  # the precondition, in fp64
    for t in ref.THRESHOLDS:
        res = _join(b, t)
        _check(b, t, res)
        assert len(res["rows_a"]) > 0
    if dim == 1:                                                               # degenerate: every pair is +1 or -1
        assert set(np.unique(np.round(b["G"])).tolist()) <= {-1.0, 1.0}
    else:
        got = set(zip(res["rows_a"].tolist(), res["rows_b"].tolist()))         # t = 0.985: the copies at 0.999 and 0.99, the exact one
        assert {(r, 200 + r) for r in range(100) if r % 6 < 2} | {(100, 300)} <= got and (101, 301) not in got


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1])
def test_row_counts_that_straddle_the_tile(cuda, n):
    b = _planted(cuda, n, 100)
    ref.check_no_pair_near(b["G"], ref.THRESHOLDS, b["eps"])
    for t in (0.5, 0.93):
        res = _join(b, t)
        _check(b, t, res)
        assert (len(res["rows_a"]) > 0) == (n > 1)


@pytest.mark.parametrize("a_range,b_range", [((0, 302), (0, 302)), ((0, 302), (200, 102)), ((0, 302), (257, 45)), ((0, 301), (301, 1)),
                                             ((100, 150), (130, 172)), ((250, 52), (0, 302)), ((0, 0), (0, 302))])
def test_ranges(cuda, a_range, b_range):
    """full x full, full x tail, a tail that starts mid-tile, a one-row tail, overlapping windows, A above B, an empty range"""
    b = _planted(cuda, 300, 384, extras=True)
    ref.check_no_pair_near(b["G"], ref.THRESHOLDS, b["eps"])
    for t in (0.5, 0.93):
        _check(b, t, _join(b, t, a_range, b_range), a_range, b_range)


def test_stage1_count_does_not_depend_on_the_buffer(cuda):
    from rag import _native as nat
    b = _planted(cuda, 300, 384, extras=True)
    t = 0.93
    thr1, _ = nat.pairs_thresholds(t, b["eps"])
    full = (0, b["n"])
    pairs, scores, count, _ = _stage1(b, thr1, full, full, 1 << 12)
    assert 0 < count <= 1 << 12
    ref.check_stage1(pairs, scores, count, 1 << 12, b["slab_h"], b["shadow_h"], t, b["eps"], thr1)
    everything = {tuple(p): s for p, s in zip(pairs.tolist(), scores.tolist())}
    for cap in (0, 1, count - 1, count):
        p, s, c, _ = _stage1(b, thr1, full, full, cap)                         # (_stage1 checks the sentinels behind cap)
        assert c == count, f"cap {cap}: count {c}, not {count}"
        assert len(p) == min(cap, count) and len({tuple(q) for q in p.tolist()}) == len(p)
        assert all(everything.get(tuple(q)) == v for q, v in zip(p.tolist(), s.tolist())), f"cap {cap}: a slot holds no candidate"


def test_two_runs_are_bit_identical_after_the_sort(cuda):
    b = _planted(cuda, 2 * T + 1, 100)
    one, two = _join(b, 0.5), _join(b, 0.5)
    for key in ("rows_a", "rows_b", "similarities"):
        assert one[key].tobytes() == two[key].tobytes(), key
    assert one["candidates"] == two["candidates"]


def test_verify_is_independent_of_the_launch_and_drops_bad_rows(cuda):
    import torch
    from rag import _native as nat
    b = _planted(cuda, 300, 1000, extras=True)
    n = b["n"]
    rng = np.random.default_rng(5)
    a = rng.integers(0, n - 1, size=777)
    pairs = np.stack([a, a + 1 + rng.integers(0, n - 1 - a)], axis=1).astype(np.int64)
    bad = np.array([[-1, 5], [3, n], [n + 7, n + 9], [0, -2]], dtype=np.int64)
    dev = torch.from_numpy(np.concatenate([pairs[:300], bad, pairs[300:]])).to(cuda)
    ra, rb, sims, kept = nat.pairs_verify(dev, b["shadow"], n, -2.0)          # a threshold everything passes
    k = int(kept.item())
    assert k == len(pairs)                                                     # the four pairs with a row outside [0, n) are gone
    whole = {(x, y): s for x, y, s in zip(ra[:k].tolist(), rb[:k].tolist(), sims[:k].cpu().numpy().view(np.uint32).tolist())}
    assert len(whole) == len({tuple(p) for p in pairs.tolist()})
    G = b["G"]
    for (x, y), bits in whole.items():
        assert abs(float(np.uint32(bits).view(np.float32)) - G[x, y]) <= 2.0 * b["dim"] * ref.U24
    for lo, hi in ((0, 1), (5, 22), (300, 777)):                               # alone, in a small launch, in another position
        sub = torch.from_numpy(pairs[lo:hi]).to(cuda)
        sa, sb, ss, sk = nat.pairs_verify(sub, b["shadow"], n, -2.0)
        assert int(sk.item()) == hi - lo
        for x, y, s in zip(sa[:hi - lo].tolist(), sb[:hi - lo].tolist(), ss[:hi - lo].cpu().numpy().view(np.uint32).tolist()):
            assert whole[(x, y)] == s, "sim32 of a pair depends on the launch it shares"
    # the stand-in's summation order (lane l: l, l + 16, ...; butterfly 8, 4, 2, 1) is the kernel's: same value to one rounding
    want = ref.sim32_standin(b["shadow_h"], pairs)
    got = np.array([whole[tuple(p)] for p in pairs.tolist()], dtype=np.uint32).view(np.float32)
    assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -23
    # and the threshold is applied to sim32 itself
    t = float(np.median(got))
    ra, rb, sims, kept = nat.pairs_verify(torch.from_numpy(pairs).to(cuda), b["shadow"], n, t)
    assert int(kept.item()) == int((got >= np.float32(t)).sum()) and bool((sims[:int(kept.item())] >= t).all())


# ---- the band: what makes stage 2 necessary ---------------------------------------------------------------------------------------------
def test_band_pairs_are_classified_as_fp64_classifies_them(cuda):
    """d = 64, 2048 rows: 1024 planted pairs whose fp64 cosine is uniform in [t - eps, t + eps] around t = 0.95.  Pairs within
    delta = 2 d 2^-24 of t may be left out (at most 5 % of the planted pairs); every other pair must come out as in fp64.  (On this
    data the slab score thresholded at t gets 26 of those pairs wrong -- tests/test_dedup_cpu.py shows the assertion catch that.)"""
    t = 0.95
    _, _, E0 = ref.build_standin(ref.band_rows(t, 3e-4)[0])
    made = ref.band_rows(t, ref.epsilon64(E0, 128))
    b = _build(cuda, "band", lambda: made[0])
    planted = made[1]
    G = b["G"]
    assert np.all(np.abs(G[planted[:, 0], planted[:, 1]] - t) <= 1.1 * b["eps"])       # the planted pairs fill the band
    rest = G.copy()
    rest[planted[:, 0], planted[:, 1]] = -1.0
    assert np.triu(rest, 1).max() < 0.9                                                 # everything else is far below t
    res = _join(b, t)
    left_out = ref.check_band(res, b["shadow_h"], t, planted)
    print(f"band: eps {b['eps']:.4g}, {left_out} pairs inside delta, {len(res['rows_a'])} of {res['candidates']} candidates kept")
    assert 100 < len(res["rows_a"]) < 924                                               # both classes are populated
    pairs, scores, count, cap, thr1 = res["stage1"]
    assert np.abs(scores.astype(np.float64) - G[pairs[:, 0], pairs[:, 1]]).max() <= b["eps"]


# ---- store level ---------------------------------------------------------------------------------------------------------------------
def _chunks(n, first=0, tag="c"):
    from rag.chunking import Chunk
    out = []
    for i in range(first, first + n):
        text = f"{tag} document number {i} of the planted set"
        out.append(Chunk(text=text, chunk_id=f"{tag}_{i}", start_char=0, end_char=len(text), page_number=i % 5 + 1, section=None,
                         tokens=len(text.split())))
    return out


def _same(a, b):
    for key in KEYS:
        assert a[key] == b[key], key


def _store(x, chunks=None, **cfg):
    from rag.indexing import VectorStore
    store = VectorStore(dict({"collection_name": "dedup"}, **cfg))
    store.create_index(chunks or _chunks(len(x)), x)
    return store


@pytest.fixture(scope="module")
def planted_store(cuda):
    x = ref.planted_rows(300, 100, extras=True)
    store = _store(x)
    sh = store.collection.shards[0]
    shadow = sh.shadow[: sh.n].cpu().numpy()
    return store, x, shadow, ref.gram64(shadow)


def test_near_duplicates_returns_the_fp64_set_with_ids(planted_store):
    from rag import _native as nat
    store, x, shadow, G = planted_store
    sh = store.collection.shards[0]
    eps = nat.pairs_epsilon(sh.row_err_max(), sh.pdim)
    ref.check_no_pair_near(G, ref.THRESHOLDS, eps)
    for t in ref.THRESHOLDS:
        res = store.near_duplicates(t)
        assert set(res) == {"rows_a", "rows_b", "similarities", "ids_a", "ids_b", "candidates", "epsilon"}
        ref.check_exact_set(res, shadow, t, G=G)
        ref.check_epsilon(res["epsilon"], sh.row_err_max(), sh.pdim)
        assert res["ids_a"] == [f"c_{r}" for r in res["rows_a"].tolist()] and res["ids_b"] == [f"c_{r}" for r in res["rows_b"].tolist()]
        assert res["candidates"] >= len(res["rows_a"]) and store.last_join["candidates"] == res["candidates"]
    # rows=: j restricted to the range, i any row below j
    for rows in ((200, 102), (257, 45), (0, 302), (301, 1), (0, 0)):
        res = store.near_duplicates(0.93, rows=rows)
        ref.check_exact_set(res, shadow, 0.93, (0, 302), rows, G=G)
    for rows in ((-1, 5), (300, 3), (0, -1), 7, (1, 2, 3)):
        with pytest.raises(ValueError):
            store.near_duplicates(0.93, rows=rows)
    assert store.mutation_epoch == 0


def test_near_duplicates_stripes_reruns_and_refuses_above_max_pairs(planted_store):
    store, x, shadow, G = planted_store
    want = store.near_duplicates(0.5)
    n_cand = want["candidates"]
    assert store.last_join == {"stripes": 1, "reruns": 0, "candidates": n_cand} and n_cand > 8
    try:
        store._join_first_cap = 4                                          # the first buffer overflows: the stripe is run again
        got = store.near_duplicates(0.5)
        assert store.last_join == {"stripes": 1, "reruns": 1, "candidates": n_cand}
        for key in ("rows_a", "rows_b", "similarities"):
            assert got[key].tobytes() == want[key].tobytes(), key
        store._join_stripe_rows = 256                                      # 2 x 2 stripes, of which the one below the diagonal is skipped
        got = store.near_duplicates(0.5)
        assert store.last_join["stripes"] == 3 and store.last_join["reruns"] >= 1 and store.last_join["candidates"] == n_cand
        for key in ("rows_a", "rows_b", "similarities"):
            assert got[key].tobytes() == want[key].tobytes(), key
        got = store.near_duplicates(0.5, rows=(257, 45))
        ref.check_exact_set(got, shadow, 0.5, (0, 302), (257, 45), G=G)
        for cap0 in (4, 1 << 16):
            store._join_first_cap = cap0
            with pytest.raises(ValueError, match=r"at least \d+ candidate pairs"):
                store.near_duplicates(0.5, max_pairs=n_cand - 1)           # never a silent truncation
            assert len(store.near_duplicates(0.5, max_pairs=n_cand)["rows_a"]) == len(want["rows_a"])
    finally:
        store._join_first_cap, store._join_stripe_rows = 1 << 16, 1 << 18


def test_duplicate_of_and_deduplicate_leave_the_store_of_the_survivors(cuda, planted_store):
    _, x, shadow, G = planted_store
    t = 0.93
    store = _store(x)
    dup = store.duplicate_of(t)
    want = ref.keep_first64(len(x), sorted(ref.pair_set64(G, t)))
    assert dup.dtype == np.int64 and np.array_equal(dup, want)
    tail = store.duplicate_of(t, rows=(250, 52))
    assert np.array_equal(tail, ref.keep_first64(len(x), sorted(ref.pair_set64(G, t, (0, 302), (250, 52))))) and np.all(tail[:250] == -1)
    dead = np.flatnonzero(want >= 0)
    assert len(dead) > 30
    q = ref.planted_rows(40, 100, seed=9)
    assert store.deduplicate(t) == len(dead) and store.collection.count() == len(x) - len(dead) and store.mutation_epoch == 1
    assert len(store.near_duplicates(t)["rows_a"]) == 0                     # nothing is left to find
    assert store.deduplicate(t) == 0 and store.mutation_epoch == 1
    keep = np.flatnonzero(want < 0)
    fresh = _store(x[keep], [c for i, c in enumerate(_chunks(len(x))) if want[i] < 0])
    assert store.collection.ids == fresh.collection.ids
    for k in (5, 70):
        _same(store.search_batch(q, top_k=k), fresh.search_batch(q, top_k=k))


def _two_batches():
    """Batch 1: 150 random rows.  Batch 2: 60 fresh rows, 40 copies of rows of batch 1 and 30 copies of its own fresh rows, at
    cosines that t = 0.93 separates (0.999 / 0.99 / 0.97 / 0.95 in, 0.90 / 0.80 out), shuffled."""
    rng = np.random.default_rng(77)
    base = ref.planted_rows(210, 100, seed=3)[:140]                          # 140 random directions (210 * 2 // 3)
    first, fresh = base[:80], base[80:]
    more = ref.planted_rows(105, 100, seed=4)[:70]
    first = np.concatenate([first, more])                                    # 150 rows
    cos = [ref.COSINES[r % 6] for r in range(70)]
    src = np.concatenate([first[:40], fresh[:30]]).astype(np.float64)
    copies = ref._at_cosine(ref._unit(src), cos, rng).astype(np.float32)
    second = np.concatenate([fresh, copies])
    second = second[rng.permutation(len(second))]
    return np.ascontiguousarray(first), np.ascontiguousarray(second)


def test_dedup_threshold_in_the_config(cuda, tmp_path):
    from rag.indexing import VectorStore
    t = 0.93
    first, second = _two_batches()
    both = np.concatenate([first, second])
    chunks = _chunks(len(both))
    shadow, slab, E = ref.build_standin(both)
    G = ref.gram64(shadow)
    ref.check_no_pair_near(G, (t,), ref.epsilon64(E, 128))
    # keep-first with the old rows always kept: pairs whose second row is in the new batch
    want = ref.keep_first64(len(both), sorted(ref.pair_set64(G, t, (0, len(both)), (len(first), len(second)))))
    dropped = int((want >= 0).sum())
    assert dropped >= 40 and np.all(want[: len(first)] == -1)
    assert any(want[j] >= len(first) for j in range(len(both)) if want[j] >= 0), "no copy of a row of its own batch was dropped"
    keep = np.flatnonzero(want < 0)
    fresh = _store(both[keep], [chunks[i] for i in keep])
    q = ref.planted_rows(40, 100, seed=11)

    persist = str(tmp_path / "db")
    for cfg in ({}, {"persist_directory": persist}):
        store = VectorStore(dict({"collection_name": "dedup", "dedup_threshold": t}, **cfg))
        store.create_index(chunks[: len(first)], first)
        assert store.last_dedup == {"added": len(first), "dropped": 0}
        store.create_index(chunks[len(first):], second)
        assert store.last_dedup == {"added": len(second) - dropped, "dropped": dropped}
        col = store.collection
        assert col.count() == len(keep) == col.shards[0].n and store.mutation_epoch == 0
        assert (col.ids, col.documents, col.metadatas) == (fresh.collection.ids, fresh.collection.documents, fresh.collection.metadatas)
        for k in (5, 70):
            _same(store.search_batch(q, top_k=k), fresh.search_batch(q, top_k=k))
        assert len(store.near_duplicates(t, rows=(len(first), len(keep) - len(first)))["rows_a"]) == 0
        if cfg:
            meta = json.load(open(os.path.join(persist, "dedup.meta.json")))
            assert meta["n"] == len(keep) and "gen" not in meta                # appended: no generation rewrite happened
            assert sorted(os.listdir(persist)) == ["dedup.docs.jsonl", "dedup.meta.json", "dedup.shadow.bin", "dedup.slab.bin"]
            again = VectorStore(dict({"collection_name": "dedup", "dedup_threshold": t}, **cfg))
            assert again.collection.ids == fresh.collection.ids and again.collection.documents == fresh.collection.documents
            for k in (5, 70):
                _same(again.search_batch(q, top_k=k), fresh.search_batch(q, top_k=k))
            # a batch of nothing but copies adds nothing
            again.create_index(_chunks(30, first=1000), both[:30])
            assert again.last_dedup == {"added": 0, "dropped": 30} and again.collection.count() == len(keep)
            assert "gen" not in json.load(open(os.path.join(persist, "dedup.meta.json")))

    # without the key the store behaves exactly as before: every row is kept
    plain = VectorStore({"collection_name": "dedup"})
    plain.create_index(chunks[: len(first)], first)
    plain.create_index(chunks[len(first):], second)
    assert plain.collection.count() == len(both) and plain.last_dedup == {"added": 0, "dropped": 0} and plain.dedup_threshold is None
    whole = _store(both, chunks)
    for k in (5, 70):
        _same(plain.search_batch(q, top_k=k), whole.search_batch(q, top_k=k))
    assert len(plain.near_duplicates(t, rows=(len(first), len(second)))["rows_a"]) >= dropped


def test_dedup_failure_leaves_the_store_as_it_was(cuda):
    from rag.indexing import VectorStore
    first, second = _two_batches()
    store = VectorStore({"collection_name": "dedup", "dedup_threshold": 0.5, "dedup_max_pairs": 3})
    store.create_index(_chunks(len(first)), first)
    q = ref.planted_rows(10, 100, seed=12)
    before = store.search_batch(q, top_k=5)
    with pytest.raises(ValueError, match="candidate pairs"):
        store.create_index(_chunks(len(second), first=len(first)), second)
    assert store.collection.count() == len(first) == store.collection.shards[0].n
    _same(store.search_batch(q, top_k=5), before)
