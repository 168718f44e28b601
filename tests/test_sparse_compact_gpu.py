"""GPU: crs::sparse_compact (csrc/sparse_compact.hip) against _sparse_ref.compact_ref: ids, weights (as int32 words) and counts
are equal -- the kernel does no floating-point arithmetic, so there is no tolerance."""
import numpy as np
import pytest

import _sparse_ref as ref

pytestmark = pytest.mark.gpu

STAGE_MAX_V = 38912      # kStageMaxV of csrc/sparse_compact.hip: longer rows are re-read from global memory


def _run(cuda, weights, vocab, cap, skip=None):
    import torch
    from rag import _native as nat
    batch = weights.shape[0]
    guard = 32
    ids = torch.full((batch * cap + guard,), -9, dtype=torch.int32, device=cuda)
    w = torch.full((batch * cap + guard,), -9.0, dtype=torch.float32, device=cuda)
    counts = torch.full((batch + guard,), -9, dtype=torch.int32, device=cuda)
    skip_t = None if skip is None else torch.tensor(skip, dtype=torch.int32, device=cuda)
    nat.sparse_compact(torch.from_numpy(weights).to(cuda), vocab, cap, skip_t,
                       out=(ids[: batch * cap].view(batch, cap), w[: batch * cap].view(batch, cap), counts[:batch]))
    torch.cuda.synchronize()
    assert (ids[batch * cap:] == -9).all() and (w[batch * cap:] == -9).all() and (counts[batch:] == -9).all(), "wrote past the outputs"
    return ids[: batch * cap].view(batch, cap).cpu().numpy(), w[: batch * cap].view(batch, cap).cpu().numpy(), counts[:batch].cpu().numpy()


def _assert_equal(got, weights, vocab, cap, skip=()):
    ids, w, counts = got
    for b in range(weights.shape[0]):
        want_i, want_w, want_n = ref.compact_ref(weights[b, :vocab], cap, skip)
        assert counts[b] == want_n, (b, counts[b], want_n)
        assert (ids[b] == want_i).all(), (b, np.argwhere(ids[b] != want_i)[:3].tolist())
        assert (w[b].view(np.int32) == want_w.view(np.int32)).all(), b
        assert (np.diff(ids[b, :want_n]) > 0).all()


def _rows(V, vp, seed, n_pos):
    """One row per entry of n_pos: that many positive weights at random ids, the rest zeros, negatives, -0.0 and a NaN; columns
    [V, vp) hold large weights that must not count."""
    rng = np.random.default_rng(seed)
    w = np.zeros((len(n_pos), vp), dtype=np.float32)
    for b, n in enumerate(n_pos):
        w[b, :V] = -np.abs(rng.standard_normal(V)).astype(np.float32) * (rng.random(V) < 0.3)
        w[b, :V][w[b, :V] == 0] = np.where(rng.random((w[b, :V] == 0).sum()) < 0.5, 0.0, -0.0)
        at = rng.choice(V, size=min(n, V), replace=False)
        w[b, at] = rng.random(at.size).astype(np.float32) * 3 + 1e-3
        if V > 4 and n < V:
            free = np.setdiff1d(np.arange(V), at)
            w[b, free[0]] = np.nan
        w[b, V:] = 99.0
    return w


@pytest.mark.parametrize("V", [10, 30522, STAGE_MAX_V + 5])
@pytest.mark.parametrize("cap", [1, 64, 1024])
def test_matches_the_reference_exactly(cuda, V, cap):
    """count < cap, == cap, > cap and an all-zero row, at every cap and at a V of each path (staged in LDS / re-read)."""
    n_pos = [0, max(cap - 3, 0), cap, cap + 1, 3 * cap + 7, V]
    weights = _rows(V, V + 5, seed=V % 1000 + cap, n_pos=n_pos)
    _assert_equal(_run(cuda, weights, V, cap), weights, V, cap)


def test_ties_exactly_at_the_threshold_go_to_the_lower_id(cuda):
    V, cap = 30522, 64
    rng = np.random.default_rng(1)
    weights = np.zeros((3, V), dtype=np.float32)
    # row 0: 40 ids above the threshold value, 100 ids AT it (24 of them fit), 500 below
    at = rng.choice(V, size=640, replace=False)
    weights[0, at[:40]] = 2.0 + rng.random(40).astype(np.float32)
    weights[0, at[40:140]] = 1.5
    weights[0, at[140:]] = rng.random(500).astype(np.float32) + 0.01
    # row 1: every positive weight equal: the 64 lowest ids
    weights[1, at] = 0.25
    # row 2: the smallest positive floats (subnormals) against each other
    weights[2, at[:200]] = np.float32(1e-45) * rng.integers(1, 4, size=200).astype(np.float32)
    got = _run(cuda, weights, V, cap)
    _assert_equal(got, weights, V, cap)
    ids = got[0]
    tied = np.sort(at[40:140])
    assert set(ids[0].tolist()) == set(at[:40].tolist()) | set(tied[:24].tolist())
    assert ids[1].tolist() == np.sort(at)[:64].tolist()


def test_skip_ids_are_always_dropped(cuda):
    V, cap = 250, 64
    weights = _rows(V, V, seed=4, n_pos=[30, 200, 64])
    skip = [0, 101, 102, 249]
    weights[:, skip] = 50.0                            # the largest weights of every row
    got = _run(cuda, weights, V, cap, skip)
    _assert_equal(got, weights, V, cap, skip)
    assert not (np.isin(got[0], skip)).any()
    _assert_equal(_run(cuda, weights, V, cap), weights, V, cap)         # and without the list they are kept


def test_bad_arguments_are_refused(cuda):
    import torch
    from rag import _native as nat
    w = torch.zeros((2, 100), device=cuda)
    with pytest.raises(nat.NativeError, match="CRS_SPARSE_MAX_TERMS"):
        nat.sparse_compact(w, 100, 1025)
    with pytest.raises(nat.NativeError, match="vocab"):
        nat.sparse_compact(w, 101, 8)
    with pytest.raises(nat.NativeError, match="skip"):
        nat.sparse_compact(w, 100, 8, torch.zeros(17, dtype=torch.int32, device=cuda))
