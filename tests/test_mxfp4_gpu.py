"""The MXFP4 index (csrc/row_build_mxfp4.hip, csrc/scan_mxfp4.hip): the row build bit for bit against the numpy
restatement of the MX quantiser (tests/_mxfp4_ref.py), and the block-scaled MFMA scan against the fp64 scores of the dequantised operands."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from _mxfp4_ref import dequant_fp4, quant_dequant_e4m3, quant_fp4, row_error32, slab_layout, unit_rows

# ---- 1. the row build, bit for bit -------------------------------------------------------------------------------------------------
def build_rows(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    t = np.float32(2.0) ** -30
    x[0] = 0                                   # norm exactly 1 (sixteen 0.25s; the rest is below its rounding): values stay as written
    x[0, 32:48] = 0.25
    x[0, :16] = np.array([4, .25, -.25, .75, -.75, 1.25, -1.25, 1.75, 2.5, -2.5, 3.5, -3.5, .5, 3, 1.5, 0], np.float32) * t   # max 2^2, every midpoint
    x[0, 64:72] = np.array([7.5, 5, -5, 7, 6.5, -7.5, 6, 5.5], np.float32) * t                                               # saturation, the 4 | 6 midpoint
    x[0, 96:100] = np.array([1e-40, -3e-39, 2.0 ** -127, 2.0 ** -126], np.float32)                                           # subnormal block maximum
    x[1, 32:64] = 0                            # an all-zero block in a random row
    x[2] = 0                                   # an all-zero row
    x[3] *= np.float32(1e-30)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [100, 384, 520])
def test_row_build_bits(cuda, dim):
    import torch
    from rag import _native as nat
    counts = [1, 15, 16, 17, 5]                # the second, third and fifth append start mid-tile
    n = sum(counts)
    x = build_rows(n, dim, seed=dim)
    v = unit_rows(x)
    assert np.array_equal(v[0, :16], x[0, :16])
    nib, E = quant_fp4(v)
    assert (E == 0).any() and nib[0, 64] == 7 and nib[0, 65] == 6 and nib[0, 1] == 0 and nib[0, 3] == 2
    xd = torch.from_numpy(x).to(cuda)

    def fresh():
        data, scales = nat.mxfp4_alloc(n + 3, dim, cuda)
        return data, scales, torch.zeros((n + 3, dim), device=cuda), torch.zeros(n + 3, device=cuda)

    data, scales, shadow, err = fresh()
    r0 = 0
    for c in counts:
        nat.slab_append_mxfp4(xd[r0:r0 + c], data, scales, r0, shadow=shadow, row_err=err)
        r0 += c
    want_d, want_s = slab_layout(nib, E, np.arange(n), n + 3)
    assert np.array_equal(data.cpu().numpy(), want_d)
    assert np.array_equal(scales.cpu().numpy(), want_s)
    assert np.array_equal(shadow.cpu().numpy()[:n].view(np.uint32), v.view(np.uint32))
    # the kernel's own summation order restated in fp32: a few ulp cover the double rounding of the stand-in's FMA and the sqrt
    np.testing.assert_array_max_ulp(err.cpu().numpy()[:n], row_error32(v, nib, E), maxulp=4)

    # the scatter form onto arbitrary rows: the same bits (a row outside the slab is skipped)
    perm = np.random.default_rng(1).permutation(n + 3)[:n]
    data2, scales2, shadow2, err2 = fresh()
    rows = torch.from_numpy(np.concatenate([perm, [n + 3, -1]])).to(cuda)
    nat.slab_write_rows_mxfp4(torch.cat([xd, xd[:2]]), rows, data2, scales2, n + 3, shadow=shadow2, row_err=err2)
    want_d, want_s = slab_layout(nib, E, perm, n + 3)
    assert np.array_equal(data2.cpu().numpy(), want_d) and np.array_equal(scales2.cpu().numpy(), want_s)
    assert np.array_equal(shadow2.cpu().numpy()[perm].view(np.uint32), v.view(np.uint32))
    assert np.array_equal(err2.cpu().numpy()[perm], err.cpu().numpy()[:n])


# ---- 2. the scan against fp64 -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_case(pdim, n_rows):
    """Quantised rows and 64 queries of one shape, their slab bytes, fp64 scores and the fp32 accumulation bound."""
    rng = np.random.default_rng(pdim + n_rows)
    v = unit_rows(rng.standard_normal((n_rows, pdim)))
    q = unit_rows(rng.standard_normal((64, pdim)) + 0.5 * v[rng.integers(0, n_rows, 64)])
    nib, E = quant_fp4(v)
    xh, qh = dequant_fp4(nib, E), quant_dequant_e4m3(q, pdim)
    return q, slab_layout(nib, E, np.arange(n_rows), n_rows), qh @ xh.T, pdim * 2.0 ** -24 * (np.abs(qh) @ np.abs(xh).T)


def check_scan(cuda, pdim, nq, kp, n_rows, id_base=0):
    import torch
    from rag import _native as nat
    q, (data, scales), ref, bound = scan_case(pdim, n_rows)
    ref, bound = ref[:nq], bound[:nq]
    s, i = nat.mxfp4_topk(torch.from_numpy(q[:nq]).to(cuda), torch.from_numpy(data).to(cuda), torch.from_numpy(scales).to(cuda), n_rows, kp,
                          id_base=id_base)
    s, i = s.cpu().numpy(), i.cpu().numpy()
    m = min(kp, n_rows)
    assert (i[:, m:] == -1).all() and np.isneginf(s[:, m:]).all()
    rows = i[:, :m] - id_base
    assert ((rows >= 0) & (rows < n_rows)).all() and all(len(set(r)) == m for r in rows)
    assert (np.diff(s[:, :m], axis=1) <= 0).all()
    qi = np.arange(nq)[:, None]
    excess = (np.abs(s[:, :m] - ref[qi, rows]) / bound[qi, rows]).max()
    print(f"pdim {pdim} nq {nq} kp {kp} n_rows {n_rows}: worst |score - fp64| / bound = {excess:.3f}")
    assert excess <= 1.0
    order = np.lexsort((np.broadcast_to(np.arange(n_rows), ref.shape), -ref), axis=1)[:, :m]
    rs = np.pad(ref[qi, order], ((0, 0), (1, 1)), constant_values=np.inf)
    rs[:, -1] = -np.inf
    if m < n_rows:
        rs[:, -1] = np.sort(ref, axis=1)[:, n_rows - m - 1]
    near = np.minimum(rs[:, :-2] - rs[:, 1:-1], rs[:, 1:-1] - rs[:, 2:]) < 2 * bound[qi, order]
    differ = rows != order
    assert not (differ & ~near).any()
    assert differ.mean() <= 0.01


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [1, -1, 16 * 3 + 5, 4099])      # -1: kp - 1 rows
@pytest.mark.parametrize("kp", [32, 64, 128])
@pytest.mark.parametrize("nq", [1, 16, 17, 64])
@pytest.mark.parametrize("pdim", [128, 384, 768, 1024])
def test_scan_against_fp64(cuda, pdim, nq, kp, n_rows):
    check_scan(cuda, pdim, nq, kp, kp - 1 if n_rows < 0 else n_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("pdim, nq, kp, n_rows, id_base", [
    (384, 17, 64, 4099, (1 << 31) + 12345),      # ids past 2^31
    (128, 17, 32, 16400, 0),                     # 1025 tiles: one stream per CU, sixteen lists at the merge's second level
])
def test_scan_offsets_and_full_grid(cuda, pdim, nq, kp, n_rows, id_base):
    check_scan(cuda, pdim, nq, kp, n_rows, id_base=id_base)


@pytest.mark.gpu
def test_negative_id_base_is_refused(cuda):
    from rag import _native as nat
    with pytest.raises(nat.NativeError, match="id_base"):
        check_scan(cuda, 128, 1, 32, 1, id_base=-1)
