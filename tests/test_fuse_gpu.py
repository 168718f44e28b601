"""GPU: weighted reciprocal rank fusion on the device (csrc/fuse.hip, crs::fuse_rrf) against the Python rule in tests/_bm25_ref.py.

The rule is fp64 arithmetic on ranks, every operation rounded on its own, so there is no tolerance: fused is compared as int64
words; rows, dense_pos, lex_pos and count with ==."""
import numpy as np
import pytest

import _bm25_ref as ref

pytestmark = pytest.mark.gpu


def _run(cuda, dense, lex, k_out, c=60.0, w_dense=1.0, w_lex=1.0):
    import torch
    from rag import _native as nat
    out = nat.fuse_rrf(torch.from_numpy(dense).to(cuda), torch.from_numpy(lex).to(cuda), k_out, c, w_dense, w_lex)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _want(dense, lex, k_out, c=60.0, w_dense=1.0, w_lex=1.0):
    per = [ref.fuse_rrf_ref(dense[i], lex[i], k_out, c, w_dense, w_lex) for i in range(dense.shape[0])]
    return [np.stack([p[j] for p in per]) for j in range(4)] + [np.array([p[4] for p in per], dtype=np.int32)]


def _assert_equal(got, want, what):
    names = ("rows", "fused", "dense_pos", "lex_pos", "count")
    for name, g, w, ty in zip(names, got, want, (np.int64, np.float64, np.int32, np.int32, np.int32)):
        assert g.dtype == ty and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        g, w = (g.view(np.int64), w.view(np.int64)) if name == "fused" else (g, w)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {name} differs first at {bad[0].tolist()}: {got[names.index(name)][tuple(bad[0])]!r} != {want[names.index(name)][tuple(bad[0])]!r}"


def _lists(rng, nq, m_dense, m_lex, universe):
    """Random list pairs over a small universe of rows (so the lists overlap), each with a random number of -1 holes at its tail."""
    dense = np.full((nq, m_dense), -1, dtype=np.int64)
    lex = np.full((nq, m_lex), -1, dtype=np.int64)
    for i in range(nq):
        nd, nl = int(rng.integers(0, m_dense + 1)), int(rng.integers(0, m_lex + 1))
        dense[i, :nd] = rng.choice(universe, size=nd, replace=False)
        lex[i, :nl] = rng.choice(universe, size=nl, replace=False)
    return dense, lex


@pytest.mark.parametrize("m_dense,m_lex", [(1, 1), (1, 64), (20, 20), (20, 64), (64, 1), (64, 20), (64, 64)])
def test_random_lists_at_every_width(cuda, m_dense, m_lex):
    rng = np.random.default_rng(100 * m_dense + m_lex)
    for nq, k_out in ((1, 1), (1, 20), (300, 20), (300, 64), (7, 1)):
        dense, lex = _lists(rng, nq, m_dense, m_lex, universe=max(m_dense, m_lex) * 2)
        _assert_equal(_run(cuda, dense, lex, k_out), _want(dense, lex, k_out), f"m=({m_dense}, {m_lex}) nq={nq} k_out={k_out}")
    dense, lex = _lists(rng, 40, m_dense, m_lex, universe=200)
    for c, w_d, w_l in ((60.0, 2.0, 1.0), (0.0, 1.0, 3.0), (10.5, 0.3, 0.7), (60.0, 1.0, 0.0)):        # unequal weights, a fractional c
        _assert_equal(_run(cuda, dense, lex, 64, c, w_d, w_l), _want(dense, lex, 64, c, w_d, w_l), f"m=({m_dense}, {m_lex}) c={c} w=({w_d}, {w_l})")


def test_disjoint_identical_and_empty_lists(cuda):
    a = np.arange(64, dtype=np.int64)[None, :] + 1000
    b = np.arange(64, dtype=np.int64)[None, :] + 5000
    none = np.full((1, 64), -1, dtype=np.int64)
    for name, dense, lex in (("disjoint", a, b), ("identical", a, a.copy()), ("reversed", a, a[:, ::-1].copy()), ("dense only", a, none),
                             ("lexical only", none, b), ("both empty", none, none)):
        for k_out in (1, 20, 64, 128):
            got = _run(cuda, dense, lex, k_out)
            _assert_equal(got, _want(dense, lex, k_out), f"{name} k_out={k_out}")
    got = _run(cuda, a, b, 128)
    # the exact tie between dense-only position i and lexical-only position i: the dense entry first
    assert got[4].tolist() == [128] and got[0][0, 0::2].tolist() == a[0].tolist() and got[0][0, 1::2].tolist() == b[0].tolist()
    assert (got[1][0, 0::2] == got[1][0, 1::2]).all() and (got[2][0, 1::2] == -1).all() and (got[3][0, 0::2] == -1).all()
    got = _run(cuda, none, none, 20)
    assert got[4].tolist() == [0] and (got[0] == -1).all() and (got[1] == 0.0).all() and (got[2] == -1).all() and (got[3] == -1).all()
    got = _run(cuda, a, a.copy(), 64)
    assert got[0][0].tolist() == a[0].tolist() and got[2][0].tolist() == got[3][0].tolist() == list(range(64))


def test_the_store_method_is_one_launch_with_the_same_results(cuda):
    import torch
    from rag.chunking import Chunk
    from rag.indexing import VectorStore
    store = VectorStore({"collection_name": "fuse"})
    store.create_index([Chunk(text=f"t{r}", chunk_id=f"c{r}", start_char=0, end_char=1, page_number=None) for r in range(8)],
                       torch.randn((8, 64), generator=torch.Generator().manual_seed(1)).numpy())
    rng = np.random.default_rng(4)
    dense, lex = _lists(rng, 50, 20, 20, universe=50)
    got = store.fuse_rrf(dense, lex, 20, c=30.0, weights=(1.0, 2.0))
    assert all(isinstance(g, np.ndarray) for g in got)
    _assert_equal(list(got), _want(dense, lex, 20, 30.0, 1.0, 2.0), "VectorStore.fuse_rrf")
    with pytest.raises(ValueError):
        store.fuse_rrf(dense, lex[:10], 20)
    with pytest.raises(ValueError):
        store.fuse_rrf(np.full((2, 65), -1), np.full((2, 1), -1), 20)
