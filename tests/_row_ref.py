"""fp64 references, DERIVED error bounds and fp32 emulations of the encoder's HBM-bound row kernels on their own (csrc/enc_misc.hip,
csrc/enc_pair.hip, csrc/enc_ln.h), shared by tests/test_row_ref_cpu.py and tests/test_row_kernels_gpu.py.  Needs no device.

    embed_ln     x = LayerNorm((word[id] + type[type id]) + pos[t % seq])                          -> x32 fp32, x16 fp16
    layernorm    x = LayerNorm(((y[0] + ... + y[nsplit - 1]) + bias) + residual)                   -> x32, x16
    pool         mean over tokens [0, len) or token 0, then x / max(||x||, 1e-12) if asked         -> out fp32, out16 fp16 zero padded
    pair_head    score = w_c . tanh(W_p h_0 + b_p) + b_c, then 1 / (1 + exp(-score)) if asked      -> scores, pooled fp32

The references are fp64 functions of the exact fp32 / int inputs.  Out-of-range ids, type ids and lens are clamped, as the kernels
document it.  Every bound below comes from counting the kernel's fp32 operations, none from what a kernel gives.  u = 2^-24; an fp32
operation (+, *, /, sqrt) is taken to err by at most ONE ulp of its result, 2u relative, so that no rounding mode is assumed (round to
nearest gives u); gamma(n) = 2 n u / (1 - 2 n u) bounds n of them in a row.  A fused multiply-add only drops a rounding.

  row value    v = ((t_1 + t_2) + ...) + t_n in the kernel's association; the terms are the operands PRESENT (an absent position row,
               bias or residual adds 0.f, which is exact): n <= 3 for the embedding, n <= nsplit + 2 for LayerNorm.  Addition k errs by
               one ulp of a partial sum of magnitude at most P_k = |t_1| + ... + |t_k|:
                 E = 2u (1 + gamma(n)) (P_2 + ... + P_n).
               An addition whose exact result is an fp32 number returns it in every rounding mode; while that holds from the first
               addition on, P_k is left out (the row of all 0.5 below: E = 0).
  LayerNorm    two-pass statistics on v, out = g (v - mean) / sigma + b, sigma = sqrt(var + eps).  The first-order bound of
               _gemm_ref.proj_ln_ref_and_bound with E above in place of its GEMM term:
                 |d out_ij| <= |g_j| / sigma_i (E_ij + mean_j E_ij + |xhat_ij| sqrt(mean_j E_ij^2)) + a_i
               a_i: the accumulation-order term of that function, 4 |torch fp32 LayerNorm - fp64 LayerNorm| on the same fp32 row
               values -- the largest over the ordinary rows, and for a designed row (below) no less than its own largest, so that a
               designed row does not loosen the bound of the others.  Its second-order figure (1 + |xhat|) |g| (max_j E_ij / sigma_i)^2
               is returned as a fraction of the bound; above 0.01 a case is inadmissible and the tests fail it as such.
               x16: + half an fp16 ulp of (|ref| + bound).
               Designed rows: all 0.5 (exact value, sum 0.5 H and mean: d = 0, the output is beta bit for bit) and mean ~100 with
               spread ~0.01, the 100 carried by the LAST term added so that one or two additions see it (E / sigma ~ 1e-3; in the first
               slab of 16 the guard would refuse it).  A one-pass E[x^2] - mean^2 variance loses 100^2 u ~ 6e-4 against a variance of
               1e-4 there.
  pool, mean   the sum of len rows in ANY order (waves x unroll accumulators, then two trees) has every element in at most len
               additions: gamma(len) S, S = sum_t |x_t|.  inv = 1 / float(len) and the product add 2u each:
                 E = (gamma(len) + 4u (1 + gamma(len))) S / len.
               len clamped to 0: sum 0, 0 * 1e9 = +0, and normalised 0 * 1e12 = +0: the exact zero vector (the tests compare bits;
               its bound is the smallest subnormal so that the ratio is defined).  CLS pooling copies token 0: E = 0.
  normalise    q = sum v^2: a product and at most 3 + 6 + 3 additions per element, bounded by gamma(hidden) as a whole; sqrt, the
               division 1 / max(sqrt(q), 1e-12) and the product v * scale add 2u each: out = vhat / ||vhat|| (1 + eta),
               |eta| <= eta_h = gamma(hidden) / 2 + 6u (taken as eta_h / (1 - eta_h)).  With vhat = v + e, |e| <= E, rigorously
                 |vhat_i / ||vhat|| - v_i / ||v||| <= (E_i + |v_i| ||E|| / ||v||) / (||v|| - ||E||) =: N_i,   bound = N_i + eta (|v_i| / ||v|| + N_i).
               Row norms are kept well inside the fp32 normal range (the reference asserts ||v|| > 1e-3 for every normalised row that
               is not the exact zero vector).  Where the squared norm underflows the kernel follows torch.nn.functional.normalize in
               fp32; that regime is out of scope here.
               out16: + half an fp16 ulp of (|ref| + bound); its columns [hidden, pdim16) are exact +0 (compared as bits).
  pair head    pre_j = W_p[j] . h + b_p[j]: hidden products and additions in any order, then the bias:
                 E_pre = gamma(hidden + 1) (sum_c |W_p[j, c]| |h_c| + |b_p[j]|);
               pooled = tanhf(pre): E_pooled = E_pre (|tanh'| <= 1) + TANH_ULP 2u (|pooled| + E_pre);
               score = sum_j w_c[j] pooled_j + b_c: per wave hidden / 4 terms in sequence (the first addition is to 0), two additions
               across the waves, one for b_c, and the product:
                 E_score = sum_j |w_c[j]| E_pooled_j + gamma(hidden / 4 + 3) (sum_j |w_c[j]| (|pooled_j| + E_pooled_j) + |b_c|);
               activation 1: s = 1 / (1 + e), e = expf(-score).  d s / d score = s (1 - s) <= 1/4; e errs by EXP_ULP ulps, moving s by
               at most EXP_ULP 2u e / (1 + e)^2 <= EXP_ULP u / 2; the addition and the division add 2u s each:
                 E_sig = E_score / 4 + EXP_ULP u / 2 + 4u s.
               TANH_ULP = 5, EXP_ULP = 3: nothing under the ROCm installation states the accuracy of the device library's tanhf and
               expf, so these are the OpenCL single-precision limits the library is written to -- a SPECIFICATION figure, not a
               measurement, and not tuned afterwards.
"""
import numpy as np
import torch

from _gemm_ref import U, distinct, half_ulp16, layer_norm64, ratio  # noqa: F401  (re-exported for the tests)

TANH_ULP, EXP_ULP = 5, 3
NAN32 = 0x7FC5A5A5            # the NaN pattern of padded tokens, guard rows and unwritten outputs
NAN16 = 0x7E5A
TINY = 2.0 ** -149            # the bound of an exact result: the ratio is 0 when it is met and >= 1 otherwise
SECOND_ORDER_LIMIT = 0.01     # tests/test_proj_ln_gpu.py


def gamma(n):
    return 2.0 * n * U / (1.0 - 2.0 * n * U)


def nan32(shape):
    return torch.full(shape, NAN32, dtype=torch.int32).view(torch.float32)


def distinct_table(t):
    """a table with every VALUE distinct (a wrong row or column cannot hide)"""
    return distinct(t.flatten()).reshape(t.shape)


def clamp_rows(i, rows):
    return i.long().clamp(0, rows - 1)


# ---- the row value -----------------------------------------------------------------------------------------------------------------------
def sum_ref_and_err(terms):
    """terms: fp64 tensors in the kernel's order.  (their sum, E of the module text)"""
    y, p, acc = terms[0].clone(), terms[0].abs(), torch.zeros_like(terms[0])
    exact = torch.ones_like(y, dtype=torch.bool)            # every addition so far gave an fp32 number: no error yet
    for t in terms[1:]:
        y, p = y + t, p + t.abs()
        exact &= y.float().double() == y
        acc = acc + torch.where(exact, torch.zeros_like(p), p)
    return y, 2.0 * U * (1.0 + gamma(len(terms))) * acc


def ln_ref_and_bound(y, e, g, b, eps, designed=()):
    """fp64 LayerNorm of the row values y [tokens, hidden] whose fp32 evaluation errs by at most e.  designed: rows that take their own
    accumulation-order term.  Returns (ref, bound32, bound16, second-order fraction)."""
    ref, xhat, sigma = layer_norm64(y, g, b, eps)
    gabs = g.double().abs()[None, :]
    first = gabs / sigma * (e + e.mean(1, keepdim=True) + xhat.abs() * torch.sqrt((e ** 2).mean(1, keepdim=True)))
    y32 = y.float()
    ln32 = torch.nn.functional.layer_norm(y32, (y32.shape[1],), g.float(), b.float(), eps).double()
    per_row = (ln32 - layer_norm64(y32.double(), g, b, eps)[0]).abs().max(1).values
    ordinary = torch.ones(y.shape[0], dtype=torch.bool)
    ordinary[list(designed)] = False
    a = torch.full_like(per_row, per_row[ordinary].max().item() if ordinary.any() else 0.0)
    a[~ordinary] = torch.maximum(a[~ordinary], per_row[~ordinary])
    bound32 = first + 4.0 * a[:, None]
    second = (1.0 + xhat.abs()) * gabs * (e.max(1, keepdim=True).values / sigma) ** 2
    bound16 = bound32 + half_ulp16(ref.abs() + bound32)
    return ref, bound32, bound16, (second / bound32).max().item()


def x16_is_a_rounding_of_x32(x16, x32):
    """tests/test_proj_ln_gpu.py's assertion: x16 is the fp16 rounding of the value x32 is the fp32 rounding of (one rounding each)"""
    x = x32.double()
    return bool(((x16.double() - x).abs() <= half_ulp16(x.abs() * (1 + 2.0 ** -23)) + x.abs() * 2.0 ** -24).all())


# ---- embedding ---------------------------------------------------------------------------------------------------------------------------
def embed_terms(ids, type_ids, word, pos, type_tab, seq):
    """the fp64 terms of a token row in the kernel's order: word, type (row 0 without type ids), position (absent: no term)"""
    tokens = ids.numel()
    terms = [word.double()[clamp_rows(ids, word.shape[0])]]
    rows = clamp_rows(type_ids, type_tab.shape[0]) if type_ids is not None else torch.zeros(tokens, dtype=torch.long)
    terms.append(type_tab.double()[rows])
    if pos is not None:
        terms.append(pos.double()[torch.arange(tokens) % seq])
    return terms


def embed_ref_and_bound(ids, type_ids, word, pos, type_tab, g, b, eps, seq):
    y, e = sum_ref_and_err(embed_terms(ids, type_ids, word, pos, type_tab, seq))
    return ln_ref_and_bound(y, e, g, b, eps)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def ln_terms(y, bias, residual):
    terms = [s.double() for s in y]
    if bias is not None:
        terms.append(bias.double()[None, :].expand_as(terms[0]))
    if residual is not None:
        terms.append(residual.double())
    return terms


def layernorm_ref_and_bound(y, bias, residual, g, b, eps, designed=()):
    v, e = sum_ref_and_err(ln_terms(y, bias, residual))
    return ln_ref_and_bound(v, e, g, b, eps, designed)


# ---- pool --------------------------------------------------------------------------------------------------------------------------------
def pool_ref_and_bound(x, lens, pooling, normalize):
    """x fp32 [batch, seq, hidden] (NaN patterns at the tokens that must not be read).  Returns (ref, bound, bound16, zero rows), fp64
    [batch, hidden]; zero rows: the rows whose result is the exact zero vector."""
    batch, seq, hidden = x.shape
    ln = lens.long().clamp(0, seq)
    ref, err = torch.zeros((batch, hidden), dtype=torch.float64), torch.zeros((batch, hidden), dtype=torch.float64)
    for i in range(batch):
        n = int(ln[i])
        if pooling == 1:
            ref[i] = x[i, 0].double()
        elif n:
            rows = x[i, :n].double()
            ref[i] = rows.sum(0) / n
            err[i] = (gamma(n) + 4.0 * U * (1.0 + gamma(n))) * rows.abs().sum(0) / n
    zero = (ln == 0) if pooling == 0 else torch.zeros(batch, dtype=torch.bool)
    if normalize:
        live = ~zero
        norm, enorm = ref[live].norm(dim=1, keepdim=True), err[live].norm(dim=1, keepdim=True)
        assert (norm > 1e-3).all() and (enorm < 1e-3 * norm).all(), "row norms must stay well inside the fp32 normal range"
        unit = ref[live] / norm
        moved = (err[live] + unit.abs() * enorm) / (norm - enorm)
        eta = 0.5 * gamma(hidden) + 6.0 * U
        eta = eta / (1.0 - eta)
        ref[live], err[live] = unit, moved + eta * (unit.abs() + moved)
    bound = err.clamp(min=TINY)
    return ref, bound, bound + half_ulp16(ref.abs() + bound), zero


# ---- pair head ---------------------------------------------------------------------------------------------------------------------------
def pair_head_ref_and_bound(h0, w_pool, b_pool, w_cls, b_cls, activation):
    """h0 fp32 [batch, hidden]: token 0 of every pair.  Returns (scores, score bound, pooled, pooled bound), fp64."""
    hidden = h0.shape[1]
    h, wp, bp, wc, bc = h0.double(), w_pool.double(), b_pool.double(), w_cls.double(), float(b_cls.double()[0])
    pre = h @ wp.T + bp[None, :]
    e_pre = gamma(hidden + 1) * (h.abs() @ wp.abs().T + bp.abs()[None, :])
    pooled = torch.tanh(pre)
    e_pooled = e_pre + TANH_ULP * 2.0 * U * (pooled.abs() + e_pre)
    score = pooled @ wc + bc
    e_score = e_pooled @ wc.abs() + gamma(hidden // 4 + 3) * ((pooled.abs() + e_pooled) @ wc.abs() + abs(bc))
    if activation == 1:
        s = 1.0 / (1.0 + torch.exp(-score))
        return s, e_score / 4.0 + EXP_ULP * U / 2.0 + 4.0 * U * s, pooled, e_pooled
    return score, e_score, pooled, e_pooled


# ---- fp32 emulations in the kernels' order, with the faults the bounds must catch (tests/test_row_ref_cpu.py) ----------------------------
F = np.float32
EMBED_FAULTS = ("pos_row_t", "type_row_ignored")
LN_FAULTS = ("uncentred_variance", "one_pass_variance", "eps_outside_sqrt", "mean_over_64pl", "last_slab_dropped", "bias_skipped",
             "residual_skipped")
POOL_FAULTS = ("mean_over_seq", "last_token_dropped_at_13_mod_16", "token_len_included", "cls_reads_last_token", "padding_unwritten")
PAIR_FAULTS = ("pooler_bias_skipped", "tanh_skipped", "sigmoid_skipped", "neighbour_cls_row", "token_1_read")


def row_form(hidden):
    """csrc/enc_forms.h: (per-lane width, float2 form)"""
    return (3, True) if hidden == 384 else (6, True) if hidden == 768 else (1, False) if hidden <= 64 else (16, False)


def _wave_sum(x):
    """x [..., 64] -> [...]: the xor butterfly of csrc/enc_ln.h (every lane ends with the same value)"""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lanes ^ o]
    return x[..., 0]


def _lane_view(v, hidden):
    """v fp32 [tokens, hidden] -> [tokens, steps, 64 lanes(, 2)] as a lane of the row form holds it, zero where a lane has no column"""
    pl, two = row_form(hidden)
    if two:
        return v.reshape(v.shape[0], pl, 64, 2)
    pad = np.zeros((v.shape[0], 64 * pl), dtype=F)
    pad[:, :hidden] = v
    return pad.reshape(v.shape[0], pl, 64)


def emulate_ln_store(v, g, b, eps, fault=None):
    """ln_store<PL> / ln_store2<P2> on fp32 row values v [tokens, hidden]: (x32, x16)"""
    tokens, hidden = v.shape
    pl, two = row_form(hidden)
    div = F(64 * pl) if fault == "mean_over_64pl" else F(hidden)

    def total(x):                                  # per-lane sums in step order, then the butterfly
        lv = _lane_view(x, hidden)
        s = np.zeros((tokens, 64), dtype=F)
        for i in range(pl):
            s = s + ((lv[:, i, :, 0] + lv[:, i, :, 1]) if two else lv[:, i])
        return _wave_sum(s)

    mean = (total(v) / div)[:, None]
    d = (v - mean).astype(F)
    if fault == "uncentred_variance":
        var = total(v * v) / div
    elif fault == "one_pass_variance":
        var = total(v * v) / div - (mean * mean)[:, 0]
    else:
        var = total(d * d) / div                   # (a lane view is zero where a lane has no column, as the kernels mask it)
    eps = F(eps)
    with np.errstate(invalid="ignore"):            # (a planted fault may give a negative variance)
        rstd = F(1.0) / ((np.sqrt(var) + eps) if fault == "eps_outside_sqrt" else np.sqrt(var + eps))
    o = (d * rstd[:, None] * g[None, :] + b[None, :]).astype(F)
    return o, o.astype(np.float16)


def emulate_embed(ids, type_ids, word, pos, type_tab, g, b, eps, seq, fault=None):
    """numpy fp32 / int32 inputs.  pos_row_t needs a position table of at least `tokens` rows."""
    tokens = ids.shape[0]
    w = word[np.clip(ids.astype(np.int64), 0, word.shape[0] - 1)]
    rows = np.zeros(tokens, dtype=np.int64)
    if type_ids is not None and fault != "type_row_ignored":
        rows = np.clip(type_ids.astype(np.int64), 0, type_tab.shape[0] - 1)
    v = w + type_tab[rows]
    if pos is not None:
        t = np.arange(tokens)
        v = v + pos[t if fault == "pos_row_t" else t % seq]
    return emulate_ln_store(v.astype(F), g, b, eps)


def emulate_layernorm(y, bias, residual, g, b, eps, fault=None):
    slabs = y.shape[0] - 1 if (fault == "last_slab_dropped" and y.shape[0] > 1) else y.shape[0]
    a = y[0].copy()
    for s in range(1, slabs):
        a = a + y[s]
    if bias is not None and fault != "bias_skipped":
        a = a + bias[None, :]
    if residual is not None and fault != "residual_skipped":
        a = a + residual
    return emulate_ln_store(a.astype(F), g, b, eps, fault)


def emulate_pool(x, lens, pooling, normalize, pdim16=0, fault=None):
    """pool_kernel: four waves x four unrolled accumulators over the tokens, a stride-4 tail.  Returns (out, out16 or None); out16 is
    [batch, pdim16], NaN patterns where nothing was written."""
    batch, seq, hidden = x.shape
    out = np.zeros((batch, hidden), dtype=F)
    for i in range(batch):
        n = min(max(int(lens[i]), 0), seq)
        if pooling == 1:
            v = x[i, n - 1 if (fault == "cls_reads_last_token" and n > 0) else 0].copy()
        else:
            last = n
            if fault == "last_token_dropped_at_13_mod_16" and n % 16 == 13:
                last = n - 1
            if fault == "token_len_included" and n < seq:
                last = n + 1
            part = []
            for wave in range(4):
                a = [np.zeros(hidden, dtype=F) for _ in range(4)]
                t = wave
                while t + 12 < last:
                    for u in range(4):
                        a[u] = a[u] + x[i, t + 4 * u]
                    t += 16
                while t < last:
                    a[0] = a[0] + x[i, t]
                    t += 4
                part.append((a[0] + a[1]) + (a[2] + a[3]))
            inv = F(1.0) / max(F(seq if fault == "mean_over_seq" else n), F(1e-9))
            v = (((part[0] + part[1]) + (part[2] + part[3])) * inv).astype(F)
        if normalize:
            pad = np.zeros(1024, dtype=F)
            pad[:hidden] = v
            th = pad.reshape(4, 256)                     # thread tid owns columns tid + 256 i
            q = ((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2]) + th[3] * th[3]
            red = _wave_sum(q.reshape(4, 64))
            qq = ((red[0] + red[1]) + red[2]) + red[3]
            v = (v * (F(1.0) / max(np.sqrt(qq), F(1e-12)))).astype(F)
        out[i] = v
    out16 = None
    if pdim16:
        out16 = np.full((batch, pdim16), NAN16, dtype=np.int16).view(np.float16)
        with np.errstate(over="ignore"):
            out16[:, :hidden] = out.astype(np.float16)
        if fault != "padding_unwritten":
            out16[:, hidden:] = 0
    return out, out16


def emulate_pair_head(h32, w_pool, b_pool, w_cls, b_cls, activation, fault=None, group=8):
    """pair_head_kernel<VEC> on hidden states h32 fp32 [batch, seq, hidden]: (scores, pooled)"""
    batch, seq, hidden = h32.shape
    vec = 2 if hidden % 128 == 0 else 1
    h0 = h32[:, 1 if (fault == "token_1_read" and seq > 1) else 0].copy()
    if fault == "neighbour_cls_row":
        for i in range(batch - 1, 0, -1):
            if i % group:
                h0[i] = h32[i - 1, 0]
    steps = hidden // (64 * vec)
    acc = np.zeros((batch, hidden, 64), dtype=F)            # [pair, pooler row j, lane]
    wl, hl = w_pool.reshape(hidden, steps, 64, vec), h0.reshape(batch, steps, 64, vec)
    for k in range(steps):
        for e in range(vec):
            acc = acc + wl[None, :, k, :, e] * hl[:, None, k, :, e]
    pre = _wave_sum(acc)
    if fault != "pooler_bias_skipped":
        pre = pre + b_pool[None, :]
    pooled = pre.astype(F) if fault == "tanh_skipped" else np.tanh(pre.astype(F)).astype(F)
    cls = np.zeros((batch, 4), dtype=F)
    for j in range(0, hidden, 4):
        cls = cls + w_cls[None, j:j + 4] * pooled[:, j:j + 4]
    s = (((cls[:, 0] + cls[:, 1]) + (cls[:, 2] + cls[:, 3])) + b_cls[0]).astype(F)
    if activation == 1 and fault != "sigmoid_skipped":
        s = (F(1.0) / (F(1.0) + np.exp(-s).astype(F))).astype(F)
    return s, pooled
