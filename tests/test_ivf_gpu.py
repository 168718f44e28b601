"""The IVF probe (csrc/ivf_probe.hip) with hand-made lists against fp64: per query, the best k of the union of the
probed lists' rows under the fp64 dot product of the fp16 values, score descending then row ascending."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

N_ROWS, N_LISTS = 3000, 48


def pdim_of(dim):
    return (dim + 127) // 128 * 128


def unit16(x, dim):
    """fp16 unit rows, zero padded to the slab's row length."""
    out = np.zeros((x.shape[0], pdim_of(dim)), np.float16)
    out[:, :dim] = x / np.linalg.norm(x, axis=1, keepdims=True)
    return out


def scores64(q16, x16, dim):
    """fp64 scores and the fp32 accumulation bound pdim 2^-24 sum |q_i x_i| (fp16 products are exact in fp32)."""
    q, x = q16.astype(np.float64), x16.astype(np.float64)
    return q @ x.T, pdim_of(dim) * 2.0 ** -24 * (np.abs(q) @ np.abs(x).T)


@functools.lru_cache(maxsize=None)
def case(dim):
    rng = np.random.default_rng(dim)
    x = unit16(rng.standard_normal((N_ROWS, dim)), dim)
    q = unit16(rng.standard_normal((256, dim)) + 0.5 * x[rng.integers(0, N_ROWS, 256), :dim], dim)
    return (q, x) + scores64(q, x, dim)


@functools.lru_cache(maxsize=None)
def partition(kind):
    """(list_offsets, list_rows) of N_ROWS rows in N_LISTS lists, rows ascending within a list."""
    rng = np.random.default_rng(len(kind))
    if kind == "balanced":
        assign = rng.integers(0, N_LISTS, N_ROWS)
    else:      # list 0 holds 90 % of the rows, lists 1..5 hold 0, 1, 15, 16 and 17, the rest is random over the other lists
        sizes = [N_ROWS * 9 // 10, 0, 1, 15, 16, 17]
        assign = np.concatenate([np.repeat(np.arange(6), sizes), rng.integers(6, N_LISTS, N_ROWS - sum(sizes))])
        assign = assign[rng.permutation(N_ROWS)]
    rows = np.argsort(assign, kind="stable").astype(np.int32)
    return np.concatenate([[0], np.cumsum(np.bincount(assign, minlength=N_LISTS))]).astype(np.int32), rows


def random_probes(nq, nprobe, seed):
    """nprobe distinct lists per query; past the N_LISTS lists there are, -1 in random places."""
    rng = np.random.default_rng(seed)
    p = np.full((nq, nprobe), -1, np.int32)
    for q in range(nq):
        p[q, rng.permutation(nprobe)[:min(nprobe, N_LISTS)]] = rng.permutation(N_LISTS)[:nprobe]
    return p


def check(cuda, dim, q16, slab, n_rows, offsets, lrows, probes, kp, cand, ref, bound):
    """slab: device fp16 [n_rows, pdim]; cand: the ascending slab rows that ref's and bound's columns stand for."""
    import torch
    from rag import _native as nat
    nq = q16.shape[0]
    s, r = nat.ivf_topk(torch.from_numpy(q16).to(cuda), slab, n_rows, dim, torch.from_numpy(offsets).to(cuda),
                        torch.from_numpy(lrows).to(cuda), torch.from_numpy(probes).to(cuda), kp, kp)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    worst = 0.0
    for q in range(nq):
        union = np.concatenate([lrows[offsets[l]:offsets[l + 1]] for l in probes[q] if l >= 0] + [np.zeros(0, np.int32)])
        cols = np.sort(np.searchsorted(cand, union))
        m = min(kp, len(cols))
        assert (r[q, m:] == -1).all() and np.isneginf(s[q, m:]).all()
        if m == 0:
            continue
        assert np.isin(r[q, :m], union).all() and len(set(r[q, :m])) == m and (np.diff(s[q, :m]) <= 0).all()
        got = np.searchsorted(cand, r[q, :m])
        worst = max(worst, (np.abs(s[q, :m] - ref[q, got]) / bound[q, got]).max())
        order = cols[np.lexsort((cols, -ref[q, cols]))]
        rs = np.concatenate([[np.inf], ref[q, order[:m + 1]], [-np.inf]])[:m + 2]
        near = np.minimum(rs[:-2] - rs[1:-1], rs[1:-1] - rs[2:]) < 2 * bound[q, order[:m]]
        assert not ((got != order[:m]) & ~near).any()
    print(f"dim {dim} nq {nq} kp {kp} nprobe {probes.shape[1]}: worst |score - fp64| / bound = {worst:.3f}")
    assert worst <= 1.0


def check_case(cuda, dim, nq, kp, probes, kind):
    import torch
    q, x, ref, bound = case(dim)
    offsets, lrows = partition(kind)
    check(cuda, dim, q[:nq], torch.from_numpy(x).to(cuda), N_ROWS, offsets, lrows, probes, kp, np.arange(N_ROWS), ref, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["balanced", "skewed"])
@pytest.mark.parametrize("nprobe", [1, 8, 64])      # 64 > N_LISTS: sixteen -1 probes per query
@pytest.mark.parametrize("kp", [32, 64])
@pytest.mark.parametrize("nq", [1, 16, 17, 64, 256])
@pytest.mark.parametrize("dim", [100, 384, 768, 1024])
def test_probe_against_fp64(cuda, dim, nq, kp, nprobe, kind):
    probes = random_probes(nq, nprobe, seed=nq + nprobe)
    if kind == "skewed":      # the long list and the five short ones are probed whatever the draw
        first = list(range(min(nprobe, 6)))
        probes[-1] = (first + [l for l in probes[-1] if l not in first])[:nprobe]
    check_case(cuda, dim, nq, kp, probes, kind)


@pytest.mark.gpu
def test_seventeen_queries_share_their_lists(cuda):
    """Every list is probed by 17 pairs: two work items per list, the second with one pair."""
    check_case(cuda, 384, 17, 32, np.tile(np.array([[0, 3, 4, 5, 7, 11, 40, 47]], np.int32), (17, 1)), "skewed")


@pytest.mark.gpu
def test_missing_probes_and_more_probes_than_lists(cuda):
    probes = random_probes(5, 64, seed=1)
    probes[1] = -1                 # a query with no list at all
    probes[2, 1:] = -1
    check_case(cuda, 100, 5, 64, probes, "balanced")


@pytest.mark.gpu
def test_rows_past_2g_and_4g_byte_offsets(cuda):
    """Listed rows on both sides of byte offsets 2^31 and 2^32 of a slab that is otherwise uninitialised."""
    import torch
    dim, row_bytes = 1024, 2048
    n_rows = (1 << 32) // row_bytes + 40
    cand = np.concatenate([np.arange(3), (1 << 31) // row_bytes + np.arange(-2, 18), (1 << 32) // row_bytes + np.arange(-2, 38)])
    rng = np.random.default_rng(7)
    x = unit16(rng.standard_normal((len(cand), dim)), dim)
    q = unit16(rng.standard_normal((3, dim)) + x[[1, 10, 40]], dim)
    slab = torch.empty((n_rows, dim), dtype=torch.float16, device=cuda)
    slab[torch.from_numpy(cand).to(cuda)] = torch.from_numpy(x).to(cuda)
    offsets = np.array([0, 23, 23, len(cand)], np.int32)      # the middle list is empty
    probes = np.array([[0, 2], [2, 1], [2, -1]], np.int32)
    check(cuda, dim, q, slab, n_rows, offsets, cand.astype(np.int32), probes, 32, cand, *scores64(q, x, dim))


@pytest.mark.gpu
@pytest.mark.parametrize("nq, nprobe, nlist, name", [(257, 1, 4, "nq"), (1, 65, 4, "nprobe"), (1, 1, (1 << 18) + 1, "nlist")])
def test_limits_are_refused(cuda, nq, nprobe, nlist, name):
    import torch
    from rag import _native as nat
    z = lambda *shape, dt=torch.int32: torch.zeros(shape, dtype=dt, device=cuda)
    with pytest.raises(nat.NativeError, match=name):
        nat.ivf_topk(z(nq, 128, dt=torch.float16), z(16, 128, dt=torch.float16), 16, 100, z(nlist + 1), z(16), z(nq, nprobe), 10, 32,
                     workspace=z(1 << 20, dt=torch.uint8))


@pytest.mark.gpu
def test_null_pointer_is_refused(cuda):
    import torch
    from rag import _native as nat
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=cuda)
    p = ctypes.c_void_p(buf.data_ptr())
    with pytest.raises(nat.NativeError, match="slab_dev"):
        nat.check(nat.load().crs_ivf_topk(p, 1, 100, None, 16, p, 4, p, 16, p, 1, 10, 32, p, buf.numel(), p, p, None))
