"""GPU: the slab build (slab_store_row, csrc/slab_row.h) against its INPUT in fp64 -- through crs_slab_append_f32,
crs_queries_to_f16 and crs_slab_write_rows_f32.

Every other GPU test builds its store with this kernel and takes the result as the truth; here the shadow is compared with
normalise64(input), the stored row with the shadow (bit for bit), the padding with +0, every row that was not named with the
sentinel it held before, and the tracked row error E with the fp64 maximum.  The bounds and their derivations are in
tests/_slab_ref.py; test_slab_ref_cpu.py shows that these assertions reject six broken builds.

Input domain: encoder output.  Magnitudes above ~1e18 overflow the kernel's fp32 sum of squares; that is outside the documented
domain and not tested.
"""
import numpy as np
import pytest
import torch

import _slab_ref as ref
from rag import _native as nat

pytestmark = pytest.mark.gpu

F16, I8 = ref.SLAB_F16, ref.SLAB_I8
TYPES = [F16, I8]
IDS = {F16: "f16", I8: "i8"}
ROW0 = 4


def _device_arrays(cuda, cap, dim, pdim, st):
    """Sentinel-filled device arrays (slab bytes 0x5a, scales / shadow NaN) and their host copies."""
    host = ref.sentinel_arrays(cap, dim, pdim, st)
    slab = torch.from_numpy(host[0].view(np.int16) if st == F16 else host[0]).to(cuda)
    if st == F16:
        slab = slab.view(torch.float16)
    return (slab, torch.from_numpy(host[1]).to(cuda), torch.from_numpy(host[2]).to(cuda)), host


def _to_host(dev, st):
    slab, scales, shadow = dev
    s = slab.view(torch.int16).cpu().numpy().view(np.float16) if st == F16 else slab.cpu().numpy()
    return s, scales.cpu().numpy(), shadow.cpu().numpy()


def _append(cuda, x, dev, row0, st, E0=0.0):
    row_err = torch.full((1,), float(E0), dtype=torch.float32, device=cuda)
    nat.slab_append_f32(torch.from_numpy(x).to(cuda), dev[0], row0, st, scales=dev[1] if st == I8 else None, shadow=dev[2], row_err=row_err)
    torch.cuda.synchronize()
    return float(row_err.item())


@pytest.mark.parametrize("n", ref.ROW_COUNTS)
@pytest.mark.parametrize("dim", ref.DIMS)
@pytest.mark.parametrize("st", TYPES, ids=IDS.get)
def test_append_against_fp64(cuda, st, dim, n):
    pdim = nat.padded_dim(dim, st)
    x, kinds, twin = ref.make_rows(n, dim, seed=1000 * dim + n)
    dev, before = _device_arrays(cuda, n + 9, dim, pdim, st)
    E = _append(cuda, x, dev, ROW0, st)
    slab, scales, shadow = _to_host(dev, st)
    r = np.arange(ROW0, ROW0 + n)
    true = ref.check_build(x, kinds, twin, slab[r], scales[r], shadow[r], E, dim, pdim, st, nat.exact_row_error_bound(dim, st))
    # int8 never touches scales it does not own; the fp16 build never touches scales at all
    ref.check_untouched(before, (slab, scales, shadow), r)
    # E is the maximum over all input kinds, so E <= the analytic bound holds for each of them, the wide-range rows (which reach
    # fp16's subnormals) included; n >= 5 has one of those
    assert n < 5 or (kinds[2] == "wide" and ref.row_error64(slab[r[2:3]], scales[r[2:3]], shadow[r[2:3]], dim, st)[0] <= true)


@pytest.mark.parametrize("dim", ref.DIMS)
@pytest.mark.parametrize("st", TYPES, ids=IDS.get)
def test_row_error_is_a_running_maximum(cuda, st, dim):
    pdim = nat.padded_dim(dim, st)
    bound = nat.exact_row_error_bound(dim, st)
    x, kinds, twin = ref.make_rows(30, dim, seed=77 + dim)
    dev, _ = _device_arrays(cuda, 80, dim, pdim, st)

    def true_of(rows):
        slab, scales, shadow = _to_host(dev, st)
        return ref.row_error64(slab[rows], scales[rows], shadow[rows], dim, st)

    # order the rows by their error (from a first build), so that "smaller" and "larger" batches can be chosen
    _append(cuda, x, dev, ROW0, st)
    order = np.argsort(true_of(np.arange(ROW0, ROW0 + 30)), kind="stable")
    small, large = np.ascontiguousarray(x[order[:15]]), np.ascontiguousarray(x[order[15:]])

    dev, _ = _device_arrays(cuda, 80, dim, pdim, st)
    E1 = _append(cuda, large, dev, ROW0, st)
    t_large = ref.check_row_error(E1, *[a[ROW0:ROW0 + 15] for a in _to_host(dev, st)], dim, st, bound)
    # a second append of rows with a smaller error leaves E unchanged
    E2 = _append(cuda, small, dev, 40, st, E0=E1)
    assert true_of(np.arange(40, 55)).max() <= t_large
    assert E2 == E1
    # a preset above the truth stays as it is
    preset = float(np.float32(2.0 * t_large + 1e-3))
    assert _append(cuda, large, dev, 60, st, E0=preset) == preset
    # two appends at different row0, the larger error second: the maximum of both
    dev, _ = _device_arrays(cuda, 80, dim, pdim, st)
    Ea = _append(cuda, small, dev, 7, st)
    ref.check_row_error(Ea, *[a[7:22] for a in _to_host(dev, st)], dim, st, bound)
    Eb = _append(cuda, large, dev, 41, st, E0=Ea)
    rows = np.concatenate([np.arange(7, 22), np.arange(41, 56)])
    ref.check_row_error(Eb, *[a[rows] for a in _to_host(dev, st)], dim, st, bound)
    assert Eb == E1 >= Ea


@pytest.mark.parametrize("dim", ref.DIMS)
@pytest.mark.parametrize("st", TYPES, ids=IDS.get)
def test_queries_to_f16_is_the_fp16_slab_row(cuda, st, dim):
    nq = 13
    x, _, _ = ref.make_rows(nq, dim, seed=31 + dim)
    pdim = nat.padded_dim(dim, st)
    p16 = nat.padded_dim(dim, F16)
    dev, _ = _device_arrays(cuda, nq, dim, p16, F16)
    _append(cuda, x, dev, 0, F16)
    want = _to_host(dev, F16)[0]
    # out= prefilled with the sentinel, two rows more than nq
    host = ref.sentinel_arrays(nq + 2, dim, pdim, F16)[0]
    out = torch.from_numpy(host.view(np.int16)).to(cuda).view(torch.float16)
    got_t = nat.queries_to_f16(torch.from_numpy(x).to(cuda), st, out=out[:nq])
    torch.cuda.synchronize()
    assert got_t.data_ptr() == out.data_ptr()
    got = out.view(torch.int16).cpu().numpy()
    assert got.shape == (nq + 2, pdim)
    assert np.array_equal(got[:nq, :dim], want.view(np.int16)[:, :dim]), "queries_to_f16 differs from the fp16 slab row"
    assert not got[:nq, dim:].any(), "padding of the query block is not +0"
    assert (got[nq:] == ref.SENTINEL_BYTE * 257).all(), "rows past nq were written"
    # and without out=: a fresh block of the slab type's padded length
    fresh = nat.queries_to_f16(torch.from_numpy(x).to(cuda), st)
    assert tuple(fresh.shape) == (nq, pdim) and np.array_equal(fresh.view(torch.int16).cpu().numpy(), got[:nq])


@pytest.mark.parametrize("st", TYPES, ids=IDS.get)
def test_write_rows_against_fp64(cuda, st):
    dim, cap, n_rows = 100, 64, 60
    pdim = nat.padded_dim(dim, st)
    assert pdim > dim
    x, kinds, twin = ref.make_rows(13, dim, seed=5)
    rows = np.array([59, 0, 17, 3, 58, 31, 4, 44, 9, 21, 1, 50, 36])
    dev, before = _device_arrays(cuda, cap, dim, pdim, st)
    E0 = 1e-7                                     # below every batch's error: E must rise to the new maximum
    row_err = torch.full((1,), E0, dtype=torch.float32, device=cuda)
    nat.slab_write_rows_f32(torch.from_numpy(x).to(cuda), torch.from_numpy(rows).to(cuda), dev[0], n_rows,
                            scales=dev[1] if st == I8 else None, shadow=dev[2], row_err=row_err)
    torch.cuda.synchronize()
    slab, scales, shadow = _to_host(dev, st)
    true = ref.check_build(x, kinds, twin, slab[rows], scales[rows], shadow[rows], float(row_err.item()), dim, pdim, st,
                           nat.exact_row_error_bound(dim, st))
    assert true > 10 * E0
    ref.check_untouched(before, (slab, scales, shadow), rows)
