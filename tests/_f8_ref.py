"""The fp8 token format of DESIGN 3.23 in plain numpy: the 256 OCP e4m3 (e4m3fn) codes decoded, a nearest-code encoder for test
inputs, and the fp64 MaxSim over decoded operands (tests/test_maxsim_f8_gpu.py, tests/test_late_f8_store_gpu.py)."""
import numpy as np

S = 8      # CRS_F8_TOKEN_SHIFT


def _decode_table():
    out = np.zeros(256)
    for code in range(256):
        e, m = (code >> 3) & 15, code & 7
        mag = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
        out[code] = -mag if code & 0x80 else mag
    out[[0x7f, 0xff]] = np.nan
    return out


DECODE = _decode_table()
_POS = DECODE[:0x7f]      # ascending magnitudes, 0 .. 448


def decode(codes):
    return DECODE[np.asarray(codes, dtype=np.uint8)]


def encode(x):
    """uint8 codes of the e4m3 value nearest to each x (saturating); ties go either way -- inputs only, never an expectation."""
    x = np.asarray(x, dtype=np.float64)
    a = np.minimum(np.abs(x), 448.0)
    hi = np.clip(np.searchsorted(_POS, a), 1, len(_POS) - 1)
    code = np.where(a - _POS[hi - 1] <= _POS[hi] - a, hi - 1, hi).astype(np.uint8)
    return code | (np.signbit(x).astype(np.uint8) << 7)


def half_step(mag):
    """Half the distance between neighbouring e4m3 values at magnitude `mag` (subnormal spacing below 2^-6)."""
    e = np.floor(np.log2(np.maximum(np.abs(mag), 2.0 ** -6)))
    return 2.0 ** (e - 4)


def maxsim(q8, q_len, tok8, offsets, rows):
    """(scores fp64 [nq, m], tolerance fp64 [nq, m]): 2^(-2S) sum_i max_j <Q_i, D_j> over the decoded codes; 0 for an empty
    document or query.  Products of e4m3 values are exact in fp32, so the only error is the fp32 accumulation of dimp products per
    pair and of q_len maxima per score: lq dimp 2^-23 2^(-2S) max|Q| max|D|."""
    q, t = decode(q8), decode(tok8)
    out = np.zeros(np.shape(rows))
    tol = np.zeros(np.shape(rows))
    for a in range(q.shape[0]):
        lq = int(q_len[a])
        for c, r in enumerate(rows[a]):
            t0, t1 = int(offsets[r]), int(offsets[r + 1])
            if lq == 0 or t1 <= t0:
                continue
            out[a, c] = (q[a, :lq] @ t[t0:t1].T).max(1).sum() * 2.0 ** (-2 * S)
            tol[a, c] = lq * q.shape[2] * 2.0 ** -23 * 2.0 ** (-2 * S) * np.abs(q[a, :lq]).max() * np.abs(t[t0:t1]).max()
    return out, tol
