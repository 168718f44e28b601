"""numpy restatement of the MX quantiser of the MXFP4 index (csrc/row_build_mxfp4.hip, csrc/scan_mxfp4.hip), of its
slab layout (csrc/mxfp4.h) and the dequantisers: what tests/test_mxfp4_*.py compare the kernels with."""
from __future__ import annotations

import numpy as np

from _slab_ref import _fma32, _lanes, _sumsq32, _wsum32

E2M1 = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)


# ---- numpy restatement of the MX quantiser, the slab layout and the dequantiser ------------------------------------------------
def pow2(e):
    return np.ldexp(np.float32(1), e).astype(np.float32)      # exact, subnormals included


def unit_rows(x):
    x = np.asarray(x, np.float32)
    den = np.maximum(np.sqrt(_sumsq32(x, x.shape[1])).astype(np.float32), np.float32(1e-12))
    return (x / den[:, None]).astype(np.float32)


def block_scale(v, emax):
    """v [n, pdim] fp32 -> E [n, pdim / 32] uint8: clamp(biased floor(log2 max|v|) - emax, 0)."""
    amax = np.abs(v).reshape(v.shape[0], -1, 32).max(axis=2)
    return np.maximum((amax.view(np.uint32) >> 23).astype(np.int64) - emax, 0)


def quant_fp4(v):
    n, dim = v.shape
    vp = np.zeros((n, -(-dim // 128) * 128), np.float32)
    vp[:, :dim] = v
    E = block_scale(vp, 2)
    y = (np.abs(vp) * np.repeat(pow2(127 - E), 32, axis=1)).astype(np.float32)
    code = ((y > 0.25).astype(int) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5.0))
    return code | (np.signbit(vp).astype(int) << 3), E


def dequant_fp4(nib, E):
    return np.where(nib & 8, -1.0, 1.0) * E2M1[nib & 7] * np.repeat(np.ldexp(1.0, E - 127), 32, axis=1)


def slab_layout(nib, E, rows, cap):
    """The tiled slab bytes (csrc/mxfp4.h) of rows `rows` in buffers sized for `cap` rows."""
    pdim = nib.shape[1]
    ks, sp, tiles = pdim // 128, (4 if pdim <= 512 else 8), -(-cap // 16)
    data = np.zeros((tiles, ks, 64, 16), np.uint8)
    scales = np.zeros((tiles, 64, sp), np.uint8)
    byte = (nib[:, 0::2] | (nib[:, 1::2] << 4)).astype(np.uint8).reshape(-1, ks, 4, 16)      # [row, k-step, block, 16 bytes]
    for i, r in enumerate(np.asarray(rows)):
        lanes = r % 16 + 16 * np.arange(4)
        data[r // 16, :, lanes] = byte[i].transpose(1, 0, 2)
        scales[r // 16, lanes, :ks] = E[i].reshape(ks, 4).T
    return data.reshape(-1), scales.reshape(-1)


def quant_dequant_e4m3(q, pdim):
    """fp32 queries -> the values of their MX e4m3 image (fp64)."""
    qp = np.zeros((q.shape[0], pdim), np.float32)
    qp[:, :q.shape[1]] = q
    E = block_scale(qp, 8)
    y = (np.abs(qp) * np.repeat(pow2(127 - E), 32, axis=1)).astype(np.float32)
    b = y.view(np.uint32).astype(np.int64)
    code = np.where(y < 0.015625, np.rint(y * np.float32(512)).astype(np.int64), ((b + 0x7ffff + ((b >> 20) & 1)) >> 20) - (120 << 3))
    code = np.minimum(code, 0x7e)
    e, m = code >> 3, code & 7
    val = np.where(e > 0, np.ldexp(1 + m / 8.0, e - 7), np.ldexp(m / 8.0, -6))
    return np.where(np.signbit(qp), -val, val) * np.repeat(np.ldexp(1.0, E - 127), 32, axis=1)


def row_error32(v, nib, E):
    """|v - dequantised row|_2 in the build kernel's fp32 order: per-lane strided FMA sums over the padded row, the butterfly, sqrt."""
    vp = np.zeros(nib.shape, np.float32)
    vp[:, :v.shape[1]] = v
    d = _lanes((vp - dequant_fp4(nib, E).astype(np.float32)).astype(np.float32), nib.shape[1])      # the dequantised values are fp32 numbers
    acc = np.zeros((v.shape[0], 64), np.float32)
    for s in range(d.shape[1]):
        acc = _fma32(d[:, s], d[:, s], acc)
    return np.sqrt(_wsum32(acc)).astype(np.float32)
