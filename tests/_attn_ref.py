"""fp64 reference and DERIVED error bound for the encoder's attention kernels on their own (csrc/enc_attn.hip, csrc/enc_qkvattn.hip), an
fp32 emulation of their forms and the faults the bound must catch.  Shared by tests/test_attn_ref_cpu.py and test_attn_forms_gpu.py.
numpy only, no device.

    ctx[b, q, h hd + d] = sum_j w_j v_jd,   w = softmax_j(s_j),   s_j = q . k_j / sqrt(hd) + bias[h][j - q]   over the keys j < len_b

from the fp16 operand VALUES in fp64, per (batch row, head); len_b = lens[b] clamped to [1, seq], as the kernels clamp it.  Every query
row < seq is compared: a padding query attends the real keys like any other.

The bound, per output element (q, d), from the reference alone.  u = 2^-24, and every fp32 operation is charged 2u relative (one whole
ulp: no rounding mode is assumed, as in tests/_gemm_ref.py); o = the reference, P = sum_j w_j |v_jd|, nb = ceil(len / 64) key blocks.

  P in fp16     2^-10 P.  The unnormalised weights p_j are rounded to fp16 before the second product; the row sum l keeps the fp32
                values, so the rounding does not cancel: one fp16 ulp (2^-10 relative) per weight, whichever way the conversion rounds.
                A weight below the normal range (p_j < 2^-14 relative to the row maximum) errs by up to 2^-25 absolute instead: + 2^-25
                sum over those keys of |v_jd| / l, l = sum_j exp(s_j - max) >= 1.
  scores        each log-weight errs by at most
                  eps_j = u (2 hd A_j + 6 (|d_j| + |b_j|) + 2 |s_j| + 4 |s_j - max| + 4),      A_j = sum_i |q_i| |k_ji| / sqrt(hd)
                -- the hd fp32 additions of the score accumulator (fp16 x fp16 products are exact in fp32); the constants
                log2(e) / sqrt(hd) and log2(e) bias, three roundings each at most; the scale / bias fma; the subtraction of the running
                maximum and the exponent's argument, both proportional to |s - max| (this covers __expf = exp2(x log2 e) in the fused
                kernel and the fma into v_exp_f32 in the others); the exponential itself, one ulp, taken as 4u.  The running maximum is
                ANY number as far as the result goes (softmax is shift-invariant and the same stored value is used for every key, for
                l and for the rescale), so its own rounding costs nothing.  Numerator and denominator see the SAME perturbed
                weights, so  |d o_d| <= G sum_j w_j eps_j |v_jd - o_d| <= G ((w eps) . |v_d| + |o_d| sum_j w_j eps_j),  G = exp(2 max_j
                eps_j) (the exact envelope, derived with F below; eps stays below 2e-3, G below 1.004); the second form is computed.
  PV in fp32    2u (66 nb) P: 64 additions per key block and the rescale of the accumulator, one multiplication per block.  The rescale
                factor alpha multiplies numerator and denominator alike and cancels.
  row sum       2u (18 + 2 nb) |o_d|: 16 additions per lane and two cross-lane steps in a block, one multiply-add per block.
  normalise     6u |o_d|: the reciprocal and the multiplication.
  output        2^-11 (|o_d| + everything above) + 2^-24: half an fp16 ulp, and the smallest fp16 subnormal.

The fused kernel (qkv_attn_kernel) projects first: the reference computes x16 W^T + b in fp64 and rounds Q, K, V to fp16 -- the
kernel's rounding points -- and the bound gains a perturbation term.  Each Q / K / V element of the kernel may differ from that
rounding by delta = the mode-0 GEMM bound of tests/_gemm_ref.py (accumulator, bias addition, output rounding).  A score then moves by
at most  E_s(q, j) = sum_i (|dq_i| |k_ji| + |q_i| |dk_ji| + |dq_i| |dk_ji|) / sqrt(hd), and with e_j the change of log-weight j
(|e_j| <= E_s):  o' - o = sum_j w_j (exp(e_j) - 1) (v_j - o) / sum_i w_i exp(e_i), so
    |d o_d| <= F (sum_j w_j E_s(q, j) |v_jd - o_d| + sum_j w_j |dv_jd|),     F = exp(2 max_j E_s(q, j))
F is the stated second-order factor: it is exact, not an estimate.  This bound is LOOSER than the others: delta is about 1e-3 per element
(half an fp16 ulp of a value near 1.6 plus 2 K u S), every one of the 2 hd products of a score is charged it at once, and E_s comes to
some 1e-2; at the median real query of a case the term is 0.5 to 19 times the plain bound, most at hidden 384
(tests/test_attn_ref_cpu.py prints the factor per case).  A wrong
key, mask or sequence start still leaves it by orders of magnitude, which is what the planted faults show.

Inputs (make_inputs): Q, K ~ 1.6 N(0, 1), so that the scores q . k / sqrt(hd) have a standard deviation near 2.6 at every head_dim and
the softmax is not flat; `peaked` multiplies Q by 3.  V ~ N(0, 1) plus an offset per key.  POISONED padding: K rows at positions
len <= pos < seq are multiplied by 4 and V rows there are 1000 -- finite, so an exactly zero weight contributes exactly zero, and a key
the mask lets through lands far outside the bound.  Bias tables: uniform in [-8, 8] per head and offset (distinct per head, asymmetric
in the offset, large enough to outweigh the product).  For the fused kernel the x16 rows of padding positions are multiplied by 8,
which scales their K and V rows alike (V cannot be set directly: it is a projection)."""
import math

import numpy as np

U = 2.0 ** -24
LOG2E = 1.44269504088896341
KB = 64                     # keys per block in every kernel
POISON_V = 1000.0


def clamp_lens(lens, seq):
    return np.clip(np.asarray(lens, dtype=np.int64), 1, seq)


def make_inputs(batch, seq, heads, hd, lens, seed, peaked=False):
    """qkv fp16 [batch * seq, 3 H] (Q | K | V column blocks, head h in columns h hd .. of each), poisoned at padding positions"""
    rng = np.random.default_rng(seed)
    q = rng.normal(0.0, 1.6, (batch, seq, heads * hd)) * (3.0 if peaked else 1.0)
    k = rng.normal(0.0, 1.6, (batch, seq, heads * hd))
    pos = np.arange(seq)
    v = rng.normal(0.0, 1.0, (batch, seq, heads * hd)) + (0.25 * ((7 * pos) % 13 - 6) + 0.01 * pos)[None, :, None]
    for b, n in enumerate(clamp_lens(lens, seq)):
        k[b, n:] *= 4.0
        v[b, n:] = POISON_V
    return np.concatenate([q, k, v], axis=2).reshape(batch * seq, 3 * heads * hd).astype(np.float16)


def make_bias(heads, span, seed):
    """fp32 [heads, 2 span - 1]: entry (key - query) + span - 1"""
    return np.random.default_rng(seed).uniform(-8.0, 8.0, (heads, 2 * span - 1)).astype(np.float32)


def make_fused_inputs(batch, seq, hidden, heads, lens, seed):
    """x16 fp16 [T, H] ~ 0.5 N(0, 1), padding rows times 8; W fp16 [3H, H] scaled so that Q, K have a standard deviation near 1.6 and V
    near 1; bias fp32 [3H] ~ 0.1 N(0, 1)"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 0.5, (batch, seq, hidden))
    for b, n in enumerate(clamp_lens(lens, seq)):
        x[b, n:] *= 8.0
    sd = np.repeat([1.6, 1.6, 1.0], hidden)[:, None] / (0.5 * math.sqrt(hidden))
    w = rng.normal(0.0, 1.0, (3 * hidden, hidden)) * sd
    bias = rng.normal(0.0, 0.1, 3 * hidden).astype(np.float32)
    return x.reshape(batch * seq, hidden).astype(np.float16), w.astype(np.float16), bias


def half_ulp16(x):
    """half an fp16 ulp at magnitude |x|: normal 2^(e - 11), 2^-25 in the subnormal range"""
    return 0.5 * np.exp2(np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -14))) - 10)


def project(x16, w, bias):
    """the fused kernel's projection in fp64: (pre [T, 3H], delta [T, 3H]) -- delta the mode-0 GEMM bound of tests/_gemm_ref.py"""
    import torch

    import _gemm_ref as gr
    pre, bound = gr.gemm_ref_and_bound(torch.from_numpy(x16), torch.from_numpy(w), torch.from_numpy(bias), None, 0)
    return pre.numpy(), bound.numpy()


def split_heads(qkv64, batch, seq, heads, hd):
    """[T, 3H] -> q, k, v [batch, heads, seq, hd]"""
    t = qkv64.reshape(batch, seq, 3, heads, hd)
    return tuple(np.ascontiguousarray(t[:, :, i].transpose(0, 2, 1, 3)) for i in range(3))


def ref_and_bound(qkv, lens, batch, seq, heads, hd, bias=None, delta=None):
    """(ref, bound, info), fp64 [batch * seq, H].  qkv: fp16 (or fp64 holding fp16 values) [T, 3H]; bias: fp32 [heads, 2 span - 1] or
    None; delta: per-element perturbation of qkv [T, 3H] (the fused kernel) or None.  info: largest eps, and for the fused kernel the
    largest F and the median of (perturbation term / plain bound) over real queries."""
    q, k, v = split_heads(np.asarray(qkv, dtype=np.float64), batch, seq, heads, hd)
    dq = dk = dv = None
    if delta is not None:
        dq, dk, dv = split_heads(np.asarray(delta, dtype=np.float64), batch, seq, heads, hd)
    n = clamp_lens(lens, seq)
    ref = np.empty((batch, seq, heads, hd))
    bound = np.empty((batch, seq, heads, hd))
    eps_max, f_max, loose = 0.0, 1.0, []
    rs = 1.0 / math.sqrt(hd)
    if bias is not None:
        span = (bias.shape[1] + 1) // 2
        off = np.arange(seq)[None, :] - np.arange(seq)[:, None] + span - 1      # [query, key] -> table entry
    for b in range(batch):
        ln = int(n[b])
        nb = (ln + KB - 1) // KB
        for h in range(heads):
            qq, kk, vv = q[b, h], k[b, h, :ln], v[b, h, :ln]
            d = qq @ kk.T * rs
            a = np.abs(qq) @ np.abs(kk).T * rs
            bs = bias[h].astype(np.float64)[off[:, :ln]] if bias is not None else np.zeros_like(d)
            s = d + bs
            mx = s.max(axis=1, keepdims=True)
            p = np.exp(s - mx)
            l = p.sum(axis=1, keepdims=True)
            w = p / l
            o = w @ vv
            pabs = w @ np.abs(vv)
            eps = U * (2 * hd * a + 6 * (np.abs(d) + np.abs(bs)) + 2 * np.abs(s) + 4 * np.abs(s - mx) + 4)
            eps_max = max(eps_max, float(eps.max()))
            weps = w * eps
            e = 2.0 ** -10 * pabs + 2.0 ** -25 * ((p < 2.0 ** -14) @ np.abs(vv)) / l
            e += np.exp(2 * eps.max(axis=1, keepdims=True)) * (weps @ np.abs(vv) + np.abs(o) * weps.sum(axis=1, keepdims=True))
            e += 2 * U * (66 * nb) * pabs + 2 * U * (18 + 2 * nb + 3) * np.abs(o)
            if delta is not None:
                ddq, ddk, ddv = np.abs(dq[b, h]), np.abs(dk[b, h, :ln]), np.abs(dv[b, h, :ln])
                es = (ddq @ np.abs(kk).T + np.abs(qq) @ ddk.T + ddq @ ddk.T) * rs
                f = np.exp(2 * es.max(axis=1, keepdims=True))
                f_max = max(f_max, float(f.max()))
                spread = np.abs(vv[None, :, :] - o[:, None, :])                  # [query, key, d]: seq <= 64 here
                pert = f * (np.einsum("qj,qjd->qd", w * es, spread) + w @ ddv)
                loose.append(np.median(pert[:ln] / e[:ln]))
                e += pert
            ref[b, :, h] = o
            bound[b, :, h] = e + 2.0 ** -11 * (np.abs(o) + e) + 2.0 ** -24
    info = {"eps_max": eps_max, "f_max": f_max, "pert_over_plain": float(np.median(loose)) if loose else 0.0}
    return ref.reshape(batch * seq, heads * hd), bound.reshape(batch * seq, heads * hd), info


def fused_ref_and_bound(x16, w, bias, lens, batch, seq, heads):
    hidden = x16.shape[1]
    pre, delta = project(x16, w, bias)
    qkv_r = pre.astype(np.float16)                  # the kernel's rounding points
    return ref_and_bound(qkv_r, lens, batch, seq, heads, hidden // heads, None, delta)


def ratio(out, ref, bound):
    """largest |out - ref| / bound over the elements; a NaN or an infinity in the output counts as infinite"""
    r = np.abs(np.asarray(out, dtype=np.float64) - ref) / bound
    return float("inf") if not np.isfinite(r).all() else float(r.max())


# ---- fp32 emulation of the kernels' forms, with the faults the bound must catch (tests/test_attn_ref_cpu.py) ---------------------------
FAULTS = ("mask_admits_len", "mask_drops_last", "wrong_hd_scale", "no_rescale", "vt_group_swap", "bias_query_minus_key",
          "bias_head_stride", "lens_of_neighbour", "rows_past_seq_not_zeroed_last_row", "fused_sequence_start")
# rows_past_seq_not_zeroed_last_row: K / V rows >= seq taken from the rows that follow in memory instead of zero.  Their keys are masked,
# so their weight is exactly zero: inside the tensor (every batch row but the last) the rows that follow are finite and the result does
# NOT change -- the fault cannot be seen there, by this bound or by any other.  It shows only in the LAST batch row, where the rows that
# follow are the NaN guard rows behind the tensor (0 x NaN = NaN), and only if that row's keys reach the block that holds rows >= seq.
F32 = np.float32


def _fma32(a, b, c):
    """one rounding: fp32(a * b + c), a, b, c fp32 arrays (the product of two fp32 values is exact in fp64)"""
    return (a.astype(np.float64) * np.float64(b) + c).astype(F32)


def _matmul32(a, b, depth):
    """a [m, K] b [n, K]^T accumulated `depth` columns at a time in fp32 (one MFMA's depth)"""
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=F32)
    for i in range(0, a.shape[1], depth):
        acc = acc + a[:, i:i + depth] @ b[:, i:i + depth].T
    return acc


def emulate(qkv, lens, batch, seq, heads, hd, bias=None, form="blocked", fault=None):
    """What a kernel of enc_attn.hip computes, in fp32: 64-key blocks with the online rescale in base 2, P rounded to fp16, 16-deep
    (form "blocked": attention_kernel, attention_seq_kernel) or 32-deep ("seq32"; "short": 32-deep scores, 16-deep second product)
    accumulation.  Rows >= seq read as zero.  fault: one of FAULTS, planted as a kernel would commit it.  Returns fp16 [T, H]."""
    hidden = heads * hd
    tokens = batch * seq
    sp = (seq + KB - 1) // KB * KB
    flat = np.concatenate([np.asarray(qkv, dtype=F32), np.full((sp, 3 * hidden), np.nan, dtype=F32)])   # the guard rows behind the tensor
    n = clamp_lens(lens, seq)
    d_qk = 16 if form == "blocked" else 32
    d_pv = 32 if form == "seq32" else 16
    c = F32(F32(LOG2E) / np.sqrt(F32(2 * hd if fault == "wrong_hd_scale" else hd)))
    out = np.zeros((tokens, hidden), dtype=np.float16)
    qi = np.arange(seq)
    for b in range(batch):
        ln = int(n[(b + 1) % batch] if fault == "lens_of_neighbour" else n[b])
        rows = flat[b * seq:b * seq + sp].copy()
        if fault != "rows_past_seq_not_zeroed_last_row":
            rows[seq:] = 0.0
        for h in range(heads):
            q = rows[:seq, h * hd:(h + 1) * hd]
            k = rows[:, hidden + h * hd:hidden + (h + 1) * hd]
            v = rows[:, 2 * hidden + h * hd:2 * hidden + (h + 1) * hd]
            if bias is not None:
                span = (bias.shape[1] + 1) // 2
                stride = span if fault == "bias_head_stride" else 2 * span - 1
                table = np.concatenate([bias.ravel(), np.zeros(2 * span, dtype=F32)])
                hb = (table * F32(LOG2E)).astype(F32)
            m = np.full(seq, -1e30, dtype=F32)
            l = np.zeros(seq, dtype=F32)
            o = np.zeros((seq, hd), dtype=F32)
            for kb in range(0, ln, KB):
                key = kb + np.arange(KB)
                s = _matmul32(q, k[kb:kb + KB], d_qk)
                if bias is not None:
                    dlt = key[None, :] - qi[:, None]
                    if fault == "bias_query_minus_key":
                        dlt = -dlt
                    inside = np.abs(dlt) < seq
                    t = _fma32(s, c, np.where(inside, hb[h * stride + span - 1 + np.where(inside, dlt, 0)], F32(0)))
                else:
                    t = s
                dead = key >= ln
                if fault == "mask_admits_len":
                    dead = key > ln
                if fault == "mask_drops_last" and ln >= 2:
                    dead = key >= ln - 1
                t = np.where(dead[None, :], F32(-1e30), t)
                mx = t.max(axis=1)
                mn = np.maximum(m, mx if bias is not None else (mx * c).astype(F32))
                alpha = np.exp2(m - mn).astype(F32)
                if fault == "no_rescale":
                    alpha = np.ones_like(alpha)
                m = mn
                p = np.exp2(t - mn[:, None]).astype(F32) if bias is not None else np.exp2(_fma32(t, c, -mn[:, None].astype(np.float64))).astype(F32)
                l = l * alpha + p.sum(axis=1, dtype=F32)
                pf = p.astype(np.float16).astype(F32)
                vb = v[kb:kb + KB]
                if fault == "vt_group_swap":          # keys 4..7 and 16..19 of every 32-key group trade places in V^T, not in P
                    vb = vb.copy()
                    for g0 in (0, 32):
                        vb[g0 + 4:g0 + 8], vb[g0 + 16:g0 + 20] = vb[g0 + 16:g0 + 20].copy(), vb[g0 + 4:g0 + 8].copy()
                o = o * alpha[:, None]
                with np.errstate(invalid="ignore"):
                    for j in range(0, KB, d_pv):
                        o = o + pf[:, j:j + d_pv] @ vb[j:j + d_pv]
            out[b * seq:(b + 1) * seq, h * hd:(h + 1) * hd] = (o * (F32(1) / l)[:, None]).astype(np.float16)
    return out


def emulate_fused(x16, w, bias, lens, batch, seq, heads, fault=None):
    """qkv_attn_kernel in fp32: the projection accumulated 16 columns at a time, + bias, rounded to fp16; one pass over the <= 64 keys
    of the sequence (no rescale), exp in base e, P rounded to fp16.  64 tokens = 64 / seq whole sequences share a workgroup: a wave
    finds its sequence's keys at s0 in the block's K / V^T tiles."""
    hidden = x16.shape[1]
    hd = hidden // heads
    qkv = (_matmul32(x16.astype(F32), w.astype(F32), 16) + bias[None, :]).astype(np.float16).astype(F32)
    n = clamp_lens(lens, seq)
    scale = F32(F32(1) / np.sqrt(F32(2 * hd if fault == "wrong_hd_scale" else hd)))
    out = np.zeros((batch * seq, hidden), dtype=np.float16)
    per_block = KB // seq
    for b in range(batch):
        ln = int(n[(b + 1) % batch] if fault == "lens_of_neighbour" else n[b])
        kv_b = b - b % per_block if fault == "fused_sequence_start" else b      # s0 = 0: the keys of the block's first sequence
        for h in range(heads):
            q = qkv[b * seq:(b + 1) * seq, h * hd:(h + 1) * hd]
            k = qkv[kv_b * seq:(kv_b + 1) * seq, hidden + h * hd:hidden + (h + 1) * hd]
            v = qkv[kv_b * seq:(kv_b + 1) * seq, 2 * hidden + h * hd:2 * hidden + (h + 1) * hd]
            s = (_matmul32(q, k, 16) * scale).astype(F32)
            key = np.arange(seq)
            dead = key >= ln
            if fault == "mask_admits_len":
                dead = key > ln
            if fault == "mask_drops_last" and ln >= 2:
                dead = key >= ln - 1
            s = np.where(dead[None, :], F32(-1e30), s)
            mx = s.max(axis=1, keepdims=True)
            p = np.exp((s - mx).astype(F32)).astype(F32)
            rs = p.sum(axis=1, dtype=F32)
            o = _matmul32(p.astype(np.float16).astype(F32), np.ascontiguousarray(v.T), 16)
            out[b * seq:(b + 1) * seq, h * hd:(h + 1) * hd] = (o * (F32(1) / rs)[:, None]).astype(np.float16)
    return out
