"""GPU: crs_rescore_f32 (csrc/convert.hip: rescore_dot_kernel + sort_rows_kernel) through nat.rescore_f32, against fp64.

The entry re-scores every candidate of a [nq, k] list in place -- scores[i, j] = <q32[i], shadow[ids[i, j] - id_base]> -- and
re-sorts each list by (score desc, id asc).  Slots with id < 0 are empty: they get -inf and go last.  Ids of another shard (outside
[id_base, id_base + n_rows)) keep the score the caller pre-filled and are sorted in place with the others.

Tolerance: the fp32 dot of two vectors differs from the fp64 dot by at most (dim + 2) 2^-24 sum |q_i x_i| (dim / 64 fmas per
lane, six butterfly additions; the bound of tests/_space_ref.py::distance_tol for an inner product).  The rows are drawn so that
distinct candidates of a list are further apart than twice that bound -- asserted before the kernel runs -- so the id order is
exact; the planted ties are bit-equal rows and must come out lower id first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ID_BASE = 2 ** 40 + 5
N_ROWS = 300
U = 2.0 ** -24


def _case(dim, k, nq, seed):
    """(q, shadow, ids, prefilled scores): each list holds -1 slots, a pair of bit-equal rows, and foreign ids (k permitting)."""
    rng = np.random.default_rng(seed)
    shadow = rng.standard_normal((N_ROWS, dim)).astype(np.float32)
    shadow[41] = shadow[17]                                             # an exact tie: rows 17 and 41 score alike for every query
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    ids = np.empty((nq, k), dtype=np.int64)
    pre = rng.standard_normal((nq, k)).astype(np.float32)               # what the caller left in the score slots
    prod = q.astype(np.float64)[:, None, :] * shadow.astype(np.float64)[None, :, :]
    s64, tol = prod.sum(axis=2), (dim + 2) * U * np.abs(prod).sum(axis=2)            # [nq, N_ROWS]
    for r in range(nq):
        slots, taken = [], []                                           # (id, pre-filled score or None); (score, tolerance) taken
        if k >= 7:
            foreign = (rng.standard_normal(2) * s64[r].std()).astype(np.float32)
            slots += [(41 + ID_BASE, None), (17 + ID_BASE, None), (-1, None), (-1, None), (ID_BASE - 1 - r, foreign[0]),
                      (ID_BASE + N_ROWS + r, foreign[1])]              # the tie, two empty slots, two ids of other shards
            taken += [(s64[r, 17], tol[r, 17]), (float(foreign[0]), 0.0), (float(foreign[1]), 0.0)]
        elif r % 2:
            slots += [(-1, None)]
        for c in rng.permutation(N_ROWS).tolist():                      # rows whose scores are clear of every score taken so far
            if len(slots) == k:
                break
            if c not in (17, 41) and all(abs(s64[r, c] - s) > 2.02 * (tol[r, c] + t) for s, t in taken):
                slots.append((c + ID_BASE, None))
                taken.append((s64[r, c], tol[r, c]))
        assert len(slots) == k, "the pool does not hold k separated rows"
        for j, at in enumerate(rng.permutation(k).tolist()):
            ids[r, j] = slots[at][0]
            if slots[at][1] is not None:
                pre[r, j] = slots[at][1]
    return q, shadow, ids, pre


def _expected(q, shadow, ids, pre):
    """Per list: (ids, fp64 scores, tolerance) in the order the entry must leave them."""
    out = []
    for r in range(ids.shape[0]):
        ent = []
        for j, gid in enumerate(ids[r].tolist()):
            row = gid - ID_BASE
            if gid < 0:
                continue
            if 0 <= row < N_ROWS:
                prod = q[r].astype(np.float64) * shadow[row].astype(np.float64)
                ent.append((gid, float(prod.sum()), (shadow.shape[1] + 2) * U * float(np.abs(prod).sum()), False))
            else:
                ent.append((gid, float(pre[r, j]), 0.0, True))         # foreign: the pre-filled fp32 score, exactly
        ent.sort(key=lambda t: (-t[1], t[0]))
        out.append(ent)
    return out


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("k", [1, 7, 64])
@pytest.mark.parametrize("dim", [1, 63, 384, 1024])
def test_rescore_against_fp64(cuda, dim, k, nq):
    import torch
    from rag import _native as nat
    q, shadow, ids, pre = _case(dim, k, nq, seed=1000 * dim + 10 * k + nq)
    want = _expected(q, shadow, ids, pre)
    for ent in want:                                                    # the tolerance must not be what orders the list
        for a, b in zip(ent, ent[1:]):
            same = {a[0], b[0]} == {17 + ID_BASE, 41 + ID_BASE}
            assert same or a[1] - b[1] > 2.0 * (a[2] + b[2]), (dim, k, nq, a, b)
    qd, sd = torch.from_numpy(q).to(cuda), torch.from_numpy(shadow).to(cuda)
    scores, idt = torch.from_numpy(pre.copy()).to(cuda), torch.from_numpy(ids.copy()).to(cuda)
    nat.rescore_f32(qd, sd, N_ROWS, ID_BASE, scores, idt)
    torch.cuda.synchronize()
    got_s, got_i = scores.cpu().numpy(), idt.cpu().numpy()
    for r, ent in enumerate(want):
        m = len(ent)
        assert np.array_equal(got_i[r, :m], np.asarray([e[0] for e in ent], dtype=np.int64)), (r, got_i[r], ent)
        assert (got_i[r, m:] == -1).all() and np.isneginf(got_s[r, m:]).all(), (r, got_i[r], got_s[r])
        for j, (gid, s64, tol, foreign) in enumerate(ent):
            if foreign:
                assert got_s[r, j] == np.float32(s64), (r, j, gid)     # survives bit for bit
            else:
                assert abs(float(got_s[r, j]) - s64) <= tol, (r, j, gid, got_s[r, j], s64, tol)
        if k >= 7:
            at = got_i[r].tolist().index(17 + ID_BASE)
            assert got_i[r, at + 1] == 41 + ID_BASE and got_s[r, at] == got_s[r, at + 1]      # the tie: equal bits, lower id first
    # the shadow and the queries are read only
    assert np.array_equal(sd.cpu().numpy(), shadow) and np.array_equal(qd.cpu().numpy(), q)


def test_rescore_refuses_bad_sizes(cuda):
    import torch
    from rag import _native as nat
    q = torch.zeros((2, 8), device=cuda)
    shadow = torch.zeros((4, 8), device=cuda)
    for k, n_rows in ((65, 4), (7, 0)):
        scores = torch.zeros((2, k), device=cuda)
        ids = torch.zeros((2, k), dtype=torch.int64, device=cuda)
        with pytest.raises(nat.NativeError, match=r"bad sizes \(k <= 64\)"):
            nat.rescore_f32(q, shadow, n_rows, 0, scores, ids)
