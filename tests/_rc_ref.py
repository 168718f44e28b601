"""The 2-bit residual token format of DESIGN 3.24 restated in numpy: the decode (three individually rounded fp16 operations), the
compression, and the fp64 MaxSim over decoded tokens with the tolerance of an fp32 accumulation of exact products
(tests/test_maxsim_rc_gpu.py)."""
import numpy as np


def unpack(codes, dimp):
    """uint8 [T, dimp / 4] -> the 2-bit code of every coordinate, [T, dimp]: coordinate d in bits 2 (d % 4) of byte d / 4."""
    d = np.arange(dimp)
    return (np.asarray(codes)[:, d // 4] >> (2 * (d % 4))) & 3


def decode(centroids, weights, cid, codes, scale):
    """fp64 [T, dimp] of the fp16 values fp16_mul(fp16_add(centroid, fp16(weight)), scale); a cid outside the table gives zeros.
    numpy rounds every float16 operation once (an fp32 intermediate is innocuous for one add or one multiply of fp16 values)."""
    cid = np.asarray(cid)
    ok = (cid >= 0) & (cid < len(centroids))
    c = np.asarray(centroids, np.float16)[np.where(ok, cid, 0)]
    w16 = np.asarray(weights, np.float32).astype(np.float16)
    t = (c + w16[unpack(codes, c.shape[1])]).astype(np.float16)
    v = (t * np.where(ok, np.asarray(scale, np.float16), np.float16(0))[:, None]).astype(np.float16)
    return v.astype(np.float64)


def compress(x16, centroids, cutoffs, weights, dim):
    """(cid, packed codes, scale in fp64, margin): nearest centroid by fp64 dot products (ties to the lowest id), the codes of the
    fp32 residual, 1 / |centroid + weight| over the first dim coordinates, and the fp64 gap to the best centroid whose row
    differs from the winner's."""
    x, c = np.asarray(x16, np.float64), np.asarray(centroids, np.float64)
    dots = x @ c.T
    cid = dots.argmax(1)
    same = (c[cid][:, None, :] == c[None, :, :]).all(2)
    margin = dots.max(1) - np.where(same, -np.inf, dots).max(1)
    res = np.asarray(x16, np.float32) - np.asarray(centroids, np.float32)[cid]
    code = (res[:, :, None] >= np.asarray(cutoffs, np.float32)[None, None, :]).sum(2)
    packed = np.zeros((len(x), x.shape[1] // 4), np.uint8)
    for d in range(x.shape[1]):
        packed[:, d // 4] |= (code[:, d] << (2 * (d % 4))).astype(np.uint8)
    v = c[cid] + np.asarray(weights, np.float64)[code]
    return cid.astype(np.int32), packed, 1.0 / np.sqrt((v[:, :dim] ** 2).sum(1)), margin


def maxsim(q16, q_len, dec, offsets, rows):
    """(scores fp64 [nq, m], tolerance): sum_i max_j <Q_i, V_j>, 0 for an empty document or query, -inf for a negative row.  fp16
    products are exact in fp32, so the only error is the fp32 accumulation of dimp products per pair and of q_len maxima per
    score: lq dimp 2^-23 max|Q| max|V| (the form of tests/_f8_ref.py)."""
    q = np.asarray(q16, np.float64)
    out, tol = np.zeros(np.shape(rows)), np.zeros(np.shape(rows))
    for a in range(q.shape[0]):
        lq = int(q_len[a])
        for c, r in enumerate(rows[a]):
            if r < 0:
                out[a, c] = -np.inf
                continue
            t0, t1 = int(offsets[r]), int(offsets[r + 1])
            if lq == 0 or t1 <= t0:
                continue
            out[a, c] = (q[a, :lq] @ dec[t0:t1].T).max(1).sum()
            tol[a, c] = lq * q.shape[2] * 2.0 ** -23 * np.abs(q[a, :lq]).max() * np.abs(dec[t0:t1]).max()
    return out, tol
