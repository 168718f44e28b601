"""fp64 reference, DERIVED bound and fp32 emulation of the sliding-window attention kernel (csrc/enc_attn.hip: attention_window_kernel),
under the derivation of tests/_attn_ref.py with two changes: the key set of query q is {j : |j - q| <= W, j < len} and nb, the
number of 64-key blocks the PV accumulation and the row sum walk, is the number of blocks the query's WORKGROUP visits,
    blocks of [max(0, qb - W) rounded down to 64, min(len, qb + 64 + W)),   qb = 64 (q // 64);   none where qb - W >= len
(at most 2 + ceil(2 W / 64)), not ceil(len / 64).  Everything else -- the fp16 rounding of P, the per-score eps, the row-sum and
normalisation terms, the output rounding -- is that module's, term for term.  The kernel scales a score before it subtracts the
running maximum (t = fl(s c), p = exp2(fl(t - m))) where the plain kernel folds the scale into an fma; the eps budget of _attn_ref
(three roundings of the constant, the scale, the subtraction, the exponential) covers both.

Rows q < len are compared.  A row q >= len is padding: it must be FINITE (zeros where it has no allowed key), nothing else.
Inputs are _attn_ref.make_inputs' (poisoned padding: K x 4 and V = 1000 at positions >= len)."""
import numpy as np

import _attn_ref as ar

KB, U = ar.KB, ar.U
WIN_FAULTS = ("window_short_right", "window_long_left", "skip_first_block", "skip_last_block", "sentinel_not_wiped")


def visited_blocks(q, seq, ln, window):
    """(first key of the first visited block, end of the visited keys) of the workgroup that owns query q"""
    w = min(window, seq)
    qb = (q // KB) * KB
    return (max(0, qb - w) // KB) * KB, (0 if qb - w >= ln else min(ln, qb + KB + w))


def ref_and_bound(qkv, lens, batch, seq, heads, hd, window):
    """(ref, bound), fp64 [batch * seq, H]; rows q >= len of ref are 0 and of bound inf (not compared)"""
    q, k, v = ar.split_heads(np.asarray(qkv, dtype=np.float64), batch, seq, heads, hd)
    n = ar.clamp_lens(lens, seq)
    ref = np.zeros((batch, seq, heads, hd))
    bound = np.full((batch, seq, heads, hd), np.inf)
    rs = 1.0 / np.sqrt(hd)
    qi = np.arange(seq)
    for b in range(batch):
        ln = int(n[b])
        nb = np.array([(visited_blocks(x, seq, ln, window)[1] - visited_blocks(x, seq, ln, window)[0] + KB - 1) // KB for x in range(ln)],
                      dtype=np.float64)[:, None]
        allowed = (np.abs(qi[:ln, None] - qi[None, :ln]) <= window)
        for h in range(heads):
            qq, kk, vv = q[b, h, :ln], k[b, h, :ln], v[b, h, :ln]
            d = qq @ kk.T * rs
            a = np.abs(qq) @ np.abs(kk).T * rs
            s = np.where(allowed, d, -np.inf)
            mx = s.max(axis=1, keepdims=True)
            p = np.where(allowed, np.exp(s - mx), 0.0)
            l = p.sum(axis=1, keepdims=True)
            w = p / l
            o = w @ vv
            pabs = w @ np.abs(vv)
            eps = np.where(allowed, U * (2 * hd * a + 6 * np.abs(d) + 2 * np.abs(d) + 4 * np.abs(np.where(allowed, d - mx, 0.0)) + 4), 0.0)
            weps = w * eps
            e = 2.0 ** -10 * pabs + 2.0 ** -25 * ((allowed & (p < 2.0 ** -14)) @ np.abs(vv)) / l
            e += np.exp(2 * eps.max(axis=1, keepdims=True)) * (weps @ np.abs(vv) + np.abs(o) * weps.sum(axis=1, keepdims=True))
            e += 2 * U * (66 * nb) * pabs + 2 * U * (18 + 2 * nb + 3) * np.abs(o)
            ref[b, :ln, h] = o
            bound[b, :ln, h] = e + 2.0 ** -11 * (np.abs(o) + e) + 2.0 ** -24
    return ref.reshape(batch * seq, heads * hd), bound.reshape(batch * seq, heads * hd)


def real_rows(lens, batch, seq):
    n = ar.clamp_lens(lens, seq)
    return (np.arange(seq)[None, :] < n[:, None]).reshape(-1)


def ratio_real(out, ref, bound, lens, batch, seq):
    """(largest |out - ref| / bound over the rows q < len, whether every row is finite)"""
    out = np.asarray(out, dtype=np.float64)
    rows = real_rows(lens, batch, seq)
    return ar.ratio(out[rows], ref[rows], bound[rows]), bool(np.isfinite(out).all())


F32 = np.float32


def emulate(qkv, lens, batch, seq, heads, hd, window, fault=None):
    """attention_window_kernel in fp32: per 64-query workgroup the visited 64-key blocks, scores scaled then masked to -1e30, the online
    rescale in base 2 from the finite sentinel, P rounded to fp16, 16-deep accumulation; a row whose maximum is still the sentinel
    is written as zeros.  fault: one of WIN_FAULTS.  Returns fp16 [T, H]."""
    hidden = heads * hd
    sp = (seq + KB - 1) // KB * KB
    n = ar.clamp_lens(lens, seq)
    c = F32(F32(ar.LOG2E) / np.sqrt(F32(hd)))
    out = np.zeros((batch * seq, hidden), dtype=np.float16)
    w = min(window, seq)
    w_right = w - 1 if fault == "window_short_right" else w
    w_left = w + 1 if fault == "window_long_left" else w
    for b in range(batch):
        ln = int(n[b])
        rows = np.zeros((sp + KB, 3 * hidden), dtype=F32)
        rows[:seq] = np.asarray(qkv[b * seq:(b + 1) * seq], dtype=F32)
        for h in range(heads):
            k = rows[:, hidden + h * hd:hidden + (h + 1) * hd]
            v = rows[:, 2 * hidden + h * hd:2 * hidden + (h + 1) * hd]
            for qb in range(0, seq, KB):
                qn = min(KB, seq - qb)
                q = rows[qb:qb + qn, h * hd:(h + 1) * hd]
                qi = qb + np.arange(qn)
                m = np.full(qn, -1e30, dtype=F32)
                l = np.zeros(qn, dtype=F32)
                o = np.zeros((qn, hd), dtype=F32)
                k_lo, k_hi = visited_blocks(qb, seq, ln, window)
                blocks = list(range(k_lo, k_hi, KB))
                if fault == "skip_first_block" and len(blocks) > 1:
                    blocks = blocks[1:]
                if fault == "skip_last_block" and len(blocks) > 1:
                    blocks = blocks[:-1]
                for kb in blocks:
                    key = kb + np.arange(KB)
                    t = (ar._matmul32(q, k[kb:kb + KB], 16) * c).astype(F32)
                    dlt = key[None, :] - qi[:, None]
                    dead = (key[None, :] >= ln) | (dlt > w_right) | (dlt < -w_left)
                    t = np.where(dead, F32(-1e30), t)
                    mn = np.maximum(m, t.max(axis=1))
                    alpha = np.exp2(m - mn).astype(F32)
                    if fault == "sentinel_not_wiped":        # the rescale of a row that leaves the sentinel is skipped
                        alpha = np.where(m <= F32(-1e29), F32(1), alpha)
                    m = mn
                    p = np.exp2((t - mn[:, None]).astype(F32)).astype(F32)
                    l = l * alpha + p.sum(axis=1, dtype=F32)
                    pf = p.astype(np.float16).astype(F32)
                    o = o * alpha[:, None]
                    for j in range(0, KB, 16):
                        o = o + pf[:, j:j + 16] @ v[kb + j:kb + j + 16]
                with np.errstate(divide="ignore", invalid="ignore"):
                    inv = np.where(m > F32(-1e29), F32(1) / l, F32(0)).astype(F32)
                out[b * seq + qb:b * seq + qb + qn, h * hd:(h + 1) * hd] = (o * inv[:, None]).astype(np.float16)
    return out
