"""GPU: the kernels of the spaces 'ip' / 'l2' (csrc/space.hip, csrc/row_build.hip, csrc/slab_row.h) each on its own against fp64 -- the row build
through crs_slab_append_space_f32, crs_slab_write_rows_space_f32 and crs_slab_rescale_space, crs_rows_norm_max,
crs_queries_to_space and crs_space_distances.

Every ip / l2 search trusts what these write: the stored row, the t coordinate, the int8 scale, the tracked row error E and the
distances.  The shadow is compared with its input bit for bit, t with the fp64 sum, the stored row with the shadow, the padding
with +0, every row that was not named with the sentinel it held before, E with the fp64 maximum over all d' coordinates.  The
bounds and their derivations are in tests/_space_build_ref.py; test_space_build_cpu.py shows that these assertions reject eight
broken builds.  Arrays a faulty kernel could overrun are views into larger sentinel blocks, so an overrun shows as a changed
sentinel.

Input domain: scaled coordinates inside the fp32 normal range.
"""
import ctypes

import numpy as np
import pytest
import torch

import _space_build_ref as ref
import _space_ref as sr
from rag import _native as nat

pytestmark = pytest.mark.gpu

F16, I8 = ref.SLAB_F16, ref.SLAB_I8
TYPES = [F16, I8]
IDS = {F16: "f16", I8: "i8"}.get
CODE = {"ip": nat.SPACE_IP, "l2": nat.SPACE_L2}
CASES = [(space, dim) for space in sr.SPACES for dim in ref.DIMS[space]]
ROW0 = 4
SCALES = (2.0 ** -10, 2.0, 2.0 ** 12)
GUARD = 2          # sentinel rows in front of an array that is handed to a kernel together with out-of-range rows


def _sizes(dim, space, st):
    sdim = ref.sdim_of(dim, space)
    return sdim, nat.padded_dim(sdim, st)


def _device_arrays(cuda, cap, sdim, pdim, st):
    """Sentinel-filled device arrays (slab bytes 0x5a, scales / shadow NaN) and their host copies."""
    host = ref.sentinel_arrays(cap, sdim, pdim, st)
    slab = torch.from_numpy(host[0].view(np.int16) if st == F16 else host[0]).to(cuda)
    if st == F16:
        slab = slab.view(torch.float16)
    return (slab, torch.from_numpy(host[1]).to(cuda), torch.from_numpy(host[2]).to(cuda)), host


def _to_host(dev, st):
    slab, scales, shadow = dev
    s = slab.view(torch.int16).cpu().numpy().view(np.float16) if st == F16 else slab.cpu().numpy()
    return s, scales.cpu().numpy(), shadow.cpu().numpy()


def _scale(cuda, R):
    return torch.full((1,), float(R), dtype=torch.float32, device=cuda)


def _append(cuda, x, space, R, dev, row0, st, E0=0.0):
    row_err = torch.full((1,), float(E0), dtype=torch.float32, device=cuda)
    nat.slab_append_space_f32(torch.from_numpy(x).to(cuda), CODE[space], _scale(cuda, R), dev[0], row0, scales=dev[1] if st == I8 else None,
                              shadow=dev[2], row_err=row_err)
    torch.cuda.synchronize()
    return float(row_err.item())


def _rescale(cuda, n_rows, dim, space, shift, dev, st, E0):
    row_err = torch.full((1,), float(E0), dtype=torch.float32, device=cuda)
    nat.slab_rescale_space(n_rows, dim, CODE[space], shift, dev[0], dev[2], scales=dev[1] if st == I8 else None, row_err=row_err)
    torch.cuda.synchronize()
    return float(row_err.item())


@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", CASES)
def test_append_against_fp64(cuda, space, dim, st):
    sdim, pdim = _sizes(dim, space, st)
    for n in ref.ROW_COUNTS:
        for R in SCALES:
            x, kinds = ref.make_space_rows(n, dim, R, seed=1000 * dim + n)
            dev, before = _device_arrays(cuda, n + 9, sdim, pdim, st)
            E = _append(cuda, x, space, R, dev, ROW0, st)
            slab, scales, shadow = _to_host(dev, st)
            r = np.arange(ROW0, ROW0 + n)
            ref.check_build_space(x, ref.row_mul(space, R), space, slab[r], scales[r], shadow[r], E, dim, pdim, st)
            # int8 never touches scales it does not own; the fp16 build never touches scales at all
            ref.check_untouched(before, (slab, scales, shadow), r)
            # DESIGN 3.12's own statement about the stored rows
            norm2 = (shadow[r].astype(np.float64) ** 2).sum(axis=1)
            assert norm2.max() <= (1.0 if space == "ip" else 0.25 + 1.0 / 16), (n, R)


@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", [("ip", 100), ("l2", 127)])
def test_write_rows_against_fp64(cuda, space, dim, st):
    n_rows, cap, R = 60, 72, 2.0
    sdim, pdim = _sizes(dim, space, st)
    x, kinds = ref.make_space_rows(16, dim, R, seed=5)
    # 13 rows of the shard in shuffled order, and three targets outside it: they must write nothing.  The arrays are views that
    # start GUARD rows into their blocks and end 12 rows after n_rows, so rows -1, n_rows and n_rows + 7 are sentinel rows
    rows = np.array([59, 0, 17, -1, 3, 58, 31, n_rows, 4, 44, 9, 21, n_rows + 7, 1, 50, 36])
    inside = (rows >= 0) & (rows < n_rows)
    assert inside.sum() == 13 and rows.max() < cap
    full, before = _device_arrays(cuda, GUARD + cap, sdim, pdim, st)
    dev = tuple(a[GUARD:] for a in full)
    E0 = 1e-7                                     # below every batch's error: E must rise to the new maximum
    row_err = torch.full((1,), E0, dtype=torch.float32, device=cuda)
    nat.slab_write_rows_space_f32(torch.from_numpy(x).to(cuda), torch.from_numpy(rows).to(cuda), CODE[space], _scale(cuda, R), dev[0], n_rows,
                                  scales=dev[1] if st == I8 else None, shadow=dev[2], row_err=row_err)
    torch.cuda.synchronize()
    slab, scales, shadow = _to_host(full, st)
    w = rows[inside] + GUARD
    true = ref.check_build_space(x[inside], ref.row_mul(space, R), space, slab[w], scales[w], shadow[w], float(row_err.item()), dim, pdim, st)
    assert true > 10 * E0
    ref.check_untouched(before, (slab, scales, shadow), w)
    # the same vectors appended: the same bits
    app, _ = _device_arrays(cuda, 13, sdim, pdim, st)
    _append(cuda, np.ascontiguousarray(x[inside]), space, R, app, 0, st)
    a_slab, a_scales, a_shadow = _to_host(app, st)
    assert ref.same_bits(slab[w], a_slab) and ref.same_bits(shadow[w], a_shadow)
    assert st == F16 or ref.same_bits(scales[w], a_scales)


@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", CASES)
def test_row_error_is_a_running_maximum(cuda, space, dim, st):
    sdim, pdim = _sizes(dim, space, st)
    R = 2.0
    x, _ = ref.make_space_rows(30, dim, R, seed=77 + dim)
    dev, _ = _device_arrays(cuda, 80, sdim, pdim, st)

    def true_of(rows):
        slab, scales, shadow = _to_host(dev, st)
        return ref.row_error64(slab[rows], scales[rows], shadow[rows], sdim, st)

    def check(E, rows):
        slab, scales, shadow = _to_host(dev, st)
        return ref.check_row_error_space(E, slab[rows], scales[rows], shadow[rows], sdim, st)

    # order the rows by their error (from a first build), so that "smaller" and "larger" batches can be chosen
    _append(cuda, x, space, R, dev, ROW0, st)
    order = np.argsort(true_of(np.arange(ROW0, ROW0 + 30)), kind="stable")
    small, large = np.ascontiguousarray(x[order[:15]]), np.ascontiguousarray(x[order[15:]])

    dev, _ = _device_arrays(cuda, 80, sdim, pdim, st)
    E1 = _append(cuda, large, space, R, dev, ROW0, st)
    t_large = check(E1, np.arange(ROW0, ROW0 + 15))
    # a second append of rows with a smaller error leaves E unchanged
    E2 = _append(cuda, small, space, R, dev, 40, st, E0=E1)
    assert true_of(np.arange(40, 55)).max() <= t_large
    assert E2 == E1
    # a preset above the truth stays as it is
    preset = float(np.float32(2.0 * t_large + 1e-3))
    assert _append(cuda, large, space, R, dev, 60, st, E0=preset) == preset
    # two appends at different row0, the larger error second: the maximum of both
    dev, _ = _device_arrays(cuda, 80, sdim, pdim, st)
    Ea = _append(cuda, small, space, R, dev, 7, st)
    check(Ea, np.arange(7, 22))
    Eb = _append(cuda, large, space, R, dev, 41, st, E0=Ea)
    check(Eb, np.concatenate([np.arange(7, 22), np.arange(41, 56)]))
    assert Eb == E1 >= Ea
    # the rescale: E keeps its old value (errors shrink with the rows, the scalar is a maximum) and covers the rebuilt rows
    dev, _ = _device_arrays(cuda, 30, sdim, pdim, st)
    E3 = _append(cuda, x, space, R, dev, 0, st)
    E4 = _rescale(cuda, 30, dim, space, 1, dev, st, E0=E3)
    rebuilt = true_of(np.arange(30)).max()
    assert E4 >= E3 and E4 >= rebuilt - 2.0 ** -25
    E5 = _rescale(cuda, 30, dim, space, 2, dev, st, E0=0.0)     # from zero: E is the rebuilt rows' own maximum
    check(E5, np.arange(30))


@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", CASES)
def test_rescale_against_a_fresh_build(cuda, space, dim, st):
    sdim, pdim = _sizes(dim, space, st)
    n, cap, R = 37, 42, 2.0          # 37 rows: a part-filled last block; rows 37 .. 41 stay sentinels
    x, _ = ref.make_space_rows(n, dim, R, seed=3 + dim)
    keep = np.arange(n)
    for shift in (1, 3, 20):
        a, before = _device_arrays(cuda, cap, sdim, pdim, st)
        Ea = _append(cuda, x, space, R, a, 0, st)
        old = _to_host(a, st)
        E = _rescale(cuda, n, dim, space, shift, a, st, E0=0.0)          # from zero: the rebuilt rows' own maximum
        b, _ = _device_arrays(cuda, cap, sdim, pdim, st)
        Eb = _append(cuda, x, space, R * 2.0 ** shift, b, 0, st)
        ha, hb = _to_host(a, st), _to_host(b, st)
        assert ref.same_bits(ha[0][:n], hb[0][:n]), ("slab", shift)
        assert ref.same_bits(ha[2][:n], hb[2][:n]), ("shadow", shift)
        assert st == F16 or ref.same_bits(ha[1][:n], hb[1][:n]), ("scales", shift)
        assert E == Eb, ("E", shift)                                     # the same rows through the same function
        ref.check_rescaled(old[2][:n], ha[2][:n], space, shift)          # t 2^-2 shift exactly
        ref.check_untouched(before, ha, keep)
        ref.check_build_space(x, ref.row_mul(space, R * 2.0 ** shift), space, ha[0][:n], ha[1][:n], ha[2][:n], E, dim, pdim, st)    # shift = 0 and n_rows = 0 change nothing, through the wrapper and through the C entry
    a, _ = _device_arrays(cuda, cap, sdim, pdim, st)
    Ea = _append(cuda, x, space, R, a, 0, st)
    old = _to_host(a, st)
    row_err = torch.full((1,), Ea, dtype=torch.float32, device=cuda)
    lib = nat.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for n_rows, shift in ((n, 0), (0, 5)):
        nat.slab_rescale_space(n_rows, dim, CODE[space], shift, a[0], a[2], scales=a[1] if st == I8 else None, row_err=row_err)
        assert lib.crs_slab_rescale_space(n_rows, dim, CODE[space], st, shift, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(row_err), None) == 0
    torch.cuda.synchronize()
    now = _to_host(a, st)
    assert all(ref.same_bits(o, h) for o, h in zip(old, now)) and float(row_err.item()) == Ea


@pytest.mark.parametrize("space,dim", CASES)
def test_queries_to_space_against_fp64(cuda, space, dim):
    sdim = ref.sdim_of(dim, space)
    rng = np.random.default_rng(31 + dim)
    pool = rng.standard_normal((70, dim))
    pool *= np.array([1e-3, 1.0, 50.0])[np.arange(70) % 3][:, None] / np.sqrt((pool * pool).sum(axis=1, keepdims=True))
    pool = pool.astype(np.float32)
    batches = [pool[:1], np.zeros((1, dim), np.float32)]
    for nq in (5, 70):
        q = pool[:nq].copy()
        q[nq - 2] = 0.0                                 # an all-zero query inside the batch
        batches.append(q)
    for st in TYPES:
        pdim = nat.padded_dim(sdim, st)
        for R in (2.0 ** -6, 2.0, 64.0):
            for q in batches:
                nq = len(q)
                # out32 / out16 are views of sentinel blocks two rows longer than nq
                blk16 = torch.from_numpy(ref.sentinel_arrays(nq + 2, sdim, pdim, F16)[0].view(np.int16)).to(cuda).view(torch.float16)
                blk32 = torch.full((nq + 2, sdim), float("nan"), dtype=torch.float32, device=cuda)
                q32_t, q16_t = nat.queries_to_space(torch.from_numpy(q).to(cuda), CODE[space], st, _scale(cuda, R), out32=blk32[:nq], out16=blk16[:nq])
                torch.cuda.synchronize()
                assert q32_t.data_ptr() == blk32.data_ptr() and q16_t.data_ptr() == blk16.data_ptr()
                got32, got16 = blk32.cpu().numpy(), blk16.view(torch.int16).cpu().numpy()
                assert np.isnan(got32[nq:]).all() and (got16[nq:] == ref.sl.SENTINEL_BYTE * 257).all(), "rows past nq were written"
                out = got32[:nq]
                assert np.isfinite(out).all()
                want = sr.queries(q, space, R)
                err = np.abs(out.astype(np.float64) - want)
                tol = ref.queries_tol(want, sdim)
                assert (err <= tol).all(), (st, R, nq, float((err / tol).max()))
                for r in np.flatnonzero(~q.any(axis=1)):
                    zero = np.zeros(sdim, np.float32)
                    if space == "l2":
                        zero[dim] = -1.0
                    assert np.array_equal(out[r], zero), "the zero query"
                assert torch.equal(blk16[:nq, :sdim], blk32[:nq].half()), "q16 is not the fp16 image of q32"
                assert not got16[:nq, sdim:].any(), "padding of the query block is not +0"
                # and without out=: fresh blocks of the same bits
                f32, f16 = nat.queries_to_space(torch.from_numpy(q).to(cuda), CODE[space], st, _scale(cuda, R))
                assert tuple(f32.shape) == (nq, sdim) and tuple(f16.shape) == (nq, pdim)
                assert torch.equal(f32.view(torch.int32), blk32[:nq].view(torch.int32)) and torch.equal(f16.view(torch.int16), blk16[:nq].view(torch.int16))


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 384, 1024])
def test_rows_norm_max(cuda, dim):
    lib = nat.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for n in ref.ROW_COUNTS:
        x, _ = ref.make_space_rows(n, dim, 2.0, seed=9 * dim + n)
        xd = torch.from_numpy(x).to(cuda)
        true = sr.row_norm_max(x)
        got = nat.rows_norm_max(xd)
        assert abs(got - true) <= ref.norm_max_rel_tol(dim) * true, (n, got, true)
        # a running maximum: a preset above the batch's norm stays, one below it is raised to the same bits
        for preset, expect in ((4.5, 4.5), (1e-3, got)):
            out = torch.full((1,), preset, dtype=torch.float32, device=cuda)
            nat.ops().rows_norm_max(xd, out)
            assert float(out.item()) == expect, (n, preset)
        # NaN, +inf or -inf in the LAST row (alone or in a part-filled block): +inf, and the flag of the C entry is 1
        for bad in (float("nan"), float("inf"), float("-inf")):
            y = xd.clone()
            y[n - 1, dim - 1] = bad
            assert nat.rows_norm_max(y) == float("inf"), (n, bad)
            out = torch.zeros(1, dtype=torch.float32, device=cuda)
            flag = torch.zeros(1, dtype=torch.int32, device=cuda)
            assert lib.crs_rows_norm_max(ptr(y), n, dim, ptr(out), ptr(flag), None) == 0
            torch.cuda.synchronize()
            assert float(out.item()) == float("inf") and int(flag.item()) == 1, (n, bad)
        flag = torch.zeros(1, dtype=torch.int32, device=cuda)
        out = torch.zeros(1, dtype=torch.float32, device=cuda)
        assert lib.crs_rows_norm_max(ptr(xd), n, dim, ptr(out), ptr(flag), None) == 0
        torch.cuda.synchronize()
        assert float(out.item()) == got and int(flag.item()) == 0


DIST_N = 300
DIST_KS = (1, 4, 5, 64, 255, 256, 257, 1024)


@pytest.mark.parametrize("space,dim", [("ip", 1), ("ip", 100), ("ip", 1024), ("l2", 1), ("l2", 100), ("l2", 1023)])
def test_space_distances_direct(cuda, space, dim):
    """crs_space_distances on id lists it never sees from a search: k up to 1024 (above the row count: duplicates), a large
    id_base, empty slots and ids outside the view.  The shadow is a view GUARD rows into its block and the block goes on after
    n_rows, so a read of row -1 or row n_rows would stay inside the allocation."""
    n, R = DIST_N, 2.0
    sdim, pdim = _sizes(dim, space, F16)
    x, _ = ref.make_space_rows(n, dim, R, seed=41 + dim)
    x[200] = x[17]                                   # two exact duplicate rows
    full, _ = _device_arrays(cuda, GUARD + n + 4, sdim, pdim, F16)
    dev = tuple(a[GUARD:] for a in full)
    _append(cuda, x, space, R, dev, 0, F16)
    shadow = dev[2]
    rec = sr.recover(shadow[:n].cpu().numpy(), space, R)
    assert np.array_equal(rec.view(np.uint32), x.view(np.uint32))          # shadow R / shadow[:, :d] 2R: the caller's vectors
    rng = np.random.default_rng(7 + dim)
    qs = rng.standard_normal((3, dim))
    qs = (qs * (np.array([0.8, 1.0, 1.3])[:, None] / np.sqrt((qs * qs).sum(axis=1, keepdims=True)))).astype(np.float32)
    Rd = _scale(cuda, R)
    for id_base in (0, 2 ** 40 + 5):
        for nq in (1, 3):
            q = np.ascontiguousarray(qs[:nq])
            qd = torch.from_numpy(q).to(cuda)
            for k in DIST_KS:
                ids = rng.integers(0, n, size=(nq, k)) + id_base                 # with replacement: k = 1024 > n repeats ids
                empty = rng.uniform(size=(nq, k)) < 0.1
                ids[empty] = rng.choice([-1, id_base - 1, id_base + n], size=int(empty.sum()))
                if k >= 4:
                    ids[:, 0], ids[:, 1] = 200 + id_base, 17 + id_base           # the duplicate rows, the higher id first
                valid = (ids >= id_base) & (ids < id_base + n) & (ids >= 0)
                ids_d = torch.from_numpy(ids).to(cuda)
                out_d, out_i = nat.space_distances(qd, CODE[space], shadow, n, id_base, Rd, ids_d)
                torch.cuda.synchronize()
                assert torch.equal(ids_d.cpu(), torch.from_numpy(ids))           # the input list is left alone
                gd, gi = out_d.cpu().numpy(), out_i.cpu().numpy()
                for r in range(nq):
                    tag = (id_base, nq, k, r)
                    m = int(valid[r].sum())
                    assert np.array_equal(np.sort(gi[r, :m]), np.sort(ids[r][valid[r]])), tag       # the multiset of valid ids
                    assert (gi[r, m:] == -1).all() and np.isposinf(gd[r, m:]).all(), tag            # empty slots last
                    assert np.isfinite(gd[r, :m]).all(), tag
                    d, i = gd[r, :m], gi[r, :m]
                    assert all(d[a] < d[a + 1] or (d[a] == d[a + 1] and i[a] <= i[a + 1]) for a in range(m - 1)), tag
                    same = np.flatnonzero(i[1:] == i[:-1])                                          # copies of an id: adjacent, same bits
                    assert len(np.unique(i)) + len(same) == m and (d[same] == d[same + 1]).all(), tag
                    rows = (i - id_base).astype(np.int64)
                    want = sr.metric64_rows(q[r], rec[rows], space)
                    tol = ref.distance_tol_full(q[r], rec[rows], space)
                    assert (np.abs(d.astype(np.float64) - want) <= tol).all(), (tag, float((np.abs(d - want) / np.maximum(tol, 1e-300)).max()))
                    if k >= 4:
                        lo, hi = np.flatnonzero(i == 17 + id_base), np.flatnonzero(i == 200 + id_base)
                        assert lo.max() < hi.min() and (d[hi] == d[lo[0]]).all(), tag            # equal distance: the lower id first
    ids_d = torch.zeros((1, 4), dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError, match="must not be ids"):
        nat.ops().space_distances(torch.from_numpy(qs[:1]).to(cuda), CODE[space], shadow, n, 0, Rd, ids_d,
                                  torch.empty((1, 4), dtype=torch.float32, device=cuda), ids_d)
