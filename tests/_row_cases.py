"""The cases of tests/test_row_ref_cpu.py and tests/test_row_kernels_gpu.py: the smallest shapes at which each form of the encoder's row
kernels (csrc/enc_misc.hip, csrc/enc_pair.hip) can still go wrong.  Every case names the kernel instantiation it must launch and its
grid; the inputs and the fp64 reference with its bounds (tests/_row_ref.py) are made once per case and shared.

  embedding   hidden 64 <1>; 128 <16>, lanes masked from the third element; 320 <16>, a partial last 64-block; 1024 <16> full; 384 <3>;
              768 <6>.  3 x 5 tokens (15: no multiple of 4, positions wrap) and one case of 1 token; vocab 37; typed with 2 and 1 type
              rows and untyped; position table given and absent; ids 0, vocab - 1, negative, >= vocab and 2^31 - 1, type ids outside
              [0, type_rows) -- clamped, as documented.  The position table has 16 rows (> 15 tokens) so that a row indexed by t
              instead of t % seq is a wrong row of the table, not a read outside it.
  LayerNorm   the six hidden sizes x the seven slab counts; tokens 1 / 5 / 130, the four bias / residual combinations and eps
              1e-12 / 1e-5 rotate so that every row form sees each of them.  From 5 tokens on, token tokens - 2 is the row of mean ~100
              and spread ~0.01, and without a bias token 1 is the row of all 0.5 (with a bias the row value 0.5 would need an exact
              cancellation).
  pool        hidden 64 / 320 / 384 / 768 / 1024, seq 40, one batch row per length of POOL_LENS (47 clamps to 40, -3 to 0); mean and
              CLS, normalised or not, out16 absent, in the f16 layout and in the int8 layout (pdim16 256 at hidden 64, 512 at 320).
              Tokens at positions >= max(len, 1) hold NaN patterns.
  pair head   hidden 64 / 192 (VEC 1) and 128 / 384 / 768 / 1024 (VEC 2; 1024: 32 KB of LDS) x batch 1 / 7 / 8 / 9 / 17; seq 1 / 3 with
              NaN patterns in every token but the first, both activations and pooled_out absent / given rotate.  b_pool holds +20 and
              -20 so that tanhf saturates; a classifier weight on those rows saturates the sigmoid.
"""
import functools
from dataclasses import dataclass

import numpy as np
import torch

import _row_ref as rr

RATIO_TAG = "row-ratio"
HIDDENS = (64, 128, 320, 1024, 384, 768)
LN_SLABS = (1, 2, 3, 4, 6, 8, 16)           # csrc/enc_forms.h: CRS_LN_SLABS
VOCAB, POS_ROWS, SEQ = 37, 16, 5
POOL_SEQ = 40
POOL_LENS = (0, 1, 2, 3, 4, 5, 12, 13, 15, 16, 17, 28, 29, 31, 32, 33, 40, 47, -3)
PAIR_GROUP = 8                               # csrc/enc_forms.h: kPairGroup
KIND_EMBED, KIND_LN, KIND_POOL, KIND_PAIR = 0, 1, 2, 3      # crs_row_plan_describe


def form_name(hidden):
    pl, two = rr.row_form(hidden)
    return ("2" if two else ""), pl


def padded_dim(hidden, slab_type):
    """crs_row_elems (csrc/scan_forms.h); the CPU test holds it against the library"""
    g = 256 if slab_type == 1 else 128
    return (hidden + g - 1) // g * g


@dataclass(frozen=True)
class EmbedCase:
    hidden: int
    tokens: int
    typed: bool
    type_rows: int
    pos: bool

    @property
    def kernel(self):
        two, pl = form_name(self.hidden)
        return f"embed_ln{two}_kernel<{pl}, {'true' if self.typed else 'false'}>"

    @property
    def line(self):
        return f"{self.kernel} grid={(self.tokens + 3) // 4}x1x1 wg=256x1x1 lds=0\n"

    @property
    def describe(self):
        return (KIND_EMBED, self.tokens, self.hidden, int(self.typed))

    @property
    def id(self):
        return f"embed-h{self.hidden}-t{self.tokens}-{'typed%d' % self.type_rows if self.typed else 'untyped'}-{'pos' if self.pos else 'nopos'}"


@dataclass(frozen=True)
class LnCase:
    hidden: int
    nsplit: int
    tokens: int
    bias: bool
    residual: bool
    eps: float

    @property
    def kernel(self):
        two, pl = form_name(self.hidden)
        return f"layernorm{two}_kernel<{pl}, {self.nsplit}>"

    @property
    def line(self):
        return f"{self.kernel} grid={(self.tokens + 3) // 4}x1x1 wg=256x1x1 lds=0\n"

    @property
    def describe(self):
        return (KIND_LN, self.tokens, self.hidden, self.nsplit)

    @property
    def half_row(self):
        return 1 if (self.tokens >= 5 and not self.bias) else None

    @property
    def big_row(self):
        return self.tokens - 2 if self.tokens >= 5 else None

    @property
    def id(self):
        return f"ln-h{self.hidden}-ns{self.nsplit}-t{self.tokens}-{'b' if self.bias else ''}{'r' if self.residual else ''}-eps{self.eps:g}"


@dataclass(frozen=True)
class PoolCase:
    hidden: int
    pooling: int          # 0 mean, 1 CLS
    normalize: bool
    out16: int            # -1: no out16; else the slab type of its layout (0 f16, 1 int8)

    kernel = "pool_kernel"

    @property
    def batch(self):
        return len(POOL_LENS)

    @property
    def pdim16(self):
        return padded_dim(self.hidden, self.out16) if self.out16 >= 0 else 0

    @property
    def line(self):
        return f"pool_kernel grid={self.batch}x1x1 wg=256x1x1 lds=0\n"

    @property
    def describe(self):
        return (KIND_POOL, self.batch, self.hidden, 0)

    @property
    def id(self):
        return f"pool-h{self.hidden}-{'cls' if self.pooling else 'mean'}-{'norm' if self.normalize else 'raw'}-{('none', 'f16', 'i8')[self.out16 + 1]}"


@dataclass(frozen=True)
class PairCase:
    hidden: int
    batch: int
    seq: int
    activation: int
    pooled_out: bool

    @property
    def kernel(self):
        return f"pair_head_kernel<{2 if self.hidden % 128 == 0 else 1}>"

    @property
    def line(self):
        return f"{self.kernel} grid={(self.batch + PAIR_GROUP - 1) // PAIR_GROUP}x1x1 wg=256x1x1 lds={PAIR_GROUP * self.hidden * 4}\n"

    @property
    def describe(self):
        return (KIND_PAIR, self.batch, self.hidden, 0)

    @property
    def id(self):
        return f"pair-h{self.hidden}-b{self.batch}-s{self.seq}-act{self.activation}-{'pooled' if self.pooled_out else 'nopooled'}"


EMBED_CASES = [c for h in HIDDENS for c in (EmbedCase(h, 15, False, 1, True), EmbedCase(h, 15, True, 2, True),
                                            EmbedCase(h, 15, True, 1, False), EmbedCase(h, 1, False, 1, False))]
LN_CASES = [LnCase(h, ns, (1, 5, 130)[(hi + ni) % 3], bool((hi + ni) & 1), bool((hi + ni) & 2), (1e-12, 1e-5)[(ni + hi // 2) % 2])
            for hi, h in enumerate(HIDDENS) for ni, ns in enumerate(LN_SLABS)]
POOL_CASES = [PoolCase(h, p, n, o) for h in (64, 320, 384, 768, 1024) for p in (0, 1) for n in (False, True) for o in (-1, 0, 1)]
PAIR_CASES = [PairCase(h, b, (1, 3)[(hi + bi) % 2], (0, 1)[(hi + bi // 2) % 2], bool((hi + bi // 2 + bi) % 2))
              for hi, h in enumerate((64, 192, 128, 384, 768, 1024)) for bi, b in enumerate((1, 7, 8, 9, 17))]
ALL_CASES = EMBED_CASES + LN_CASES + POOL_CASES + PAIR_CASES

INSTANTIATIONS = tuple(
    [f"embed_ln{two}_kernel<{pl}, {t}>" for two, pl in (("", 1), ("", 16), ("2", 3), ("2", 6)) for t in ("false", "true")] +
    [f"layernorm{two}_kernel<{pl}, {ns}>" for two, pl in (("", 1), ("", 16), ("2", 3), ("2", 6)) for ns in LN_SLABS] +
    ["pool_kernel", "pair_head_kernel<1>", "pair_head_kernel<2>"])


def case_id(c):
    return c.id


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def _gain_and_bias(gen, hidden):
    return rr.distinct(1.0 + 0.1 * torch.randn(hidden, generator=gen)), rr.distinct(0.1 * torch.randn(hidden, generator=gen))


# ---- inputs (CPU tensors; fp32 / int32) --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def embed_tables(hidden):
    gen = _gen(1, hidden)
    word = rr.distinct_table(torch.randn((VOCAB, hidden), generator=gen))
    pos = rr.distinct_table(0.5 * torch.randn((POS_ROWS, hidden), generator=gen))
    type_tab = rr.distinct_table(0.5 * torch.randn((2, hidden), generator=gen))
    g, b = _gain_and_bias(gen, hidden)
    return word, pos, type_tab, g, b


EMBED_IDS = (0, VOCAB - 1, -1, VOCAB, 2 ** 31 - 1, -2 ** 31, 5, 17, 36, 1, VOCAB + 100, 20, 3, 30, 11)
EMBED_TYPE_IDS = (0, 1, 1, 0, -1, 2, 7, 1, 0, 1, -2 ** 31, 2 ** 31 - 1, 1, 0, 1)


def embed_inputs(c):
    """(ids, type_ids or None, word, pos or None, type_tab [type_rows, H], g, b)"""
    word, pos, type_tab, g, b = embed_tables(c.hidden)
    ids = torch.tensor(EMBED_IDS[:c.tokens] if c.tokens > 1 else (VOCAB + 3,), dtype=torch.int32)
    type_ids = torch.tensor(EMBED_TYPE_IDS[:c.tokens], dtype=torch.int32) if c.typed else None
    return ids, type_ids, word, (pos if c.pos else None), type_tab[:c.type_rows].contiguous(), g, b


def ln_inputs(c):
    """(y [nsplit, tokens, H], bias or None, residual or None, g, b)"""
    gen = _gen(2, c.hidden, c.nsplit, c.tokens)
    y = torch.randn((c.nsplit, c.tokens, c.hidden), generator=gen) / c.nsplit ** 0.5
    bias = rr.distinct(0.1 * torch.randn(c.hidden, generator=gen)) if c.bias else None
    res = torch.randn((c.tokens, c.hidden), generator=gen) if c.residual else None
    if res is not None:
        res[0] = rr.distinct(res[0])
    g, b = _gain_and_bias(gen, c.hidden)
    if c.half_row is not None:                 # every term exact: 0.25 + 0.25, or 0.5 alone
        r = c.half_row
        y[:, r] = 0.0
        if res is not None:
            y[0, r], res[r] = 0.25, 0.25
        elif c.nsplit > 1:
            y[0, r], y[1, r] = 0.25, 0.25
        else:
            y[0, r] = 0.5
    if c.big_row is not None:                  # the 100 in the LAST term added
        r = c.big_row
        y[:, r] *= 0.003
        z = (100.0 + 0.01 * torch.randn(c.hidden, generator=gen)).double()
        if bias is not None:
            z = z - bias.double()
        if res is not None:
            res[r] = (z - y[:, r].double().sum(0)).float()
        else:
            y[-1, r] = (z - y[:-1, r].double().sum(0)).float()
    return y, bias, res, g, b


@functools.lru_cache(maxsize=8)
def pool_inputs(hidden):
    """(x [batch, seq, H] with NaN patterns at the tokens that must not be read, lens)"""
    gen = _gen(3, hidden)
    lens = torch.tensor(POOL_LENS, dtype=torch.int32)
    x = torch.randn((len(POOL_LENS), POOL_SEQ, hidden), generator=gen) + 0.25
    for i, n in enumerate(POOL_LENS):
        x.view(torch.int32)[i, max(min(max(n, 0), POOL_SEQ), 1):] = rr.NAN32
    return x, lens


@functools.lru_cache(maxsize=8)
def pair_weights(hidden):
    gen = _gen(4, hidden)
    w_pool = rr.distinct_table(torch.randn((hidden, hidden), generator=gen) / hidden ** 0.5)
    b_pool = 0.5 * torch.randn(hidden, generator=gen)
    b_pool[0], b_pool[1], b_pool[hidden - 1] = 20.0, -20.0, 20.0
    w_cls = 0.2 * torch.randn(hidden, generator=gen)
    w_cls[0], w_cls[hidden - 1] = 6.0, 6.0            # +12 from the two rows saturated at +1: the sigmoid saturates too
    b_cls = 0.1 * torch.randn(1, generator=gen)
    return w_pool, rr.distinct(b_pool), rr.distinct(w_cls), b_cls


def pair_hidden(hidden, batch, seq, seed_row0=0):
    """hidden states [batch, seq, H]: token 0 drawn per (hidden, GLOBAL row seed) so that the same pair can sit in two batches"""
    x = rr.nan32((batch, seq, hidden)).clone()
    for i in range(batch):
        x[i, 0] = torch.randn(hidden, generator=_gen(5, hidden, seed_row0 + i))
    return x


def pair_inputs(c):
    return (pair_hidden(c.hidden, c.batch, c.seq),) + pair_weights(c.hidden)


# ---- references, once per case -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def case_reference(c):
    """(inputs, reference) -- embedding / LayerNorm: (ref, bound32, bound16, second order); pool: (ref, bound, bound16, zero rows);
    pair head: (scores, score bound, pooled, pooled bound)"""
    if isinstance(c, EmbedCase):
        inp = embed_inputs(c)
        return inp, rr.embed_ref_and_bound(*inp, 1e-12, SEQ)
    if isinstance(c, LnCase):
        inp = ln_inputs(c)
        designed = [r for r in (c.half_row, c.big_row) if r is not None]
        return inp, rr.layernorm_ref_and_bound(*inp, c.eps, designed)
    if isinstance(c, PoolCase):
        inp = pool_inputs(c.hidden)
        return inp, rr.pool_ref_and_bound(inp[0], inp[1], c.pooling, c.normalize)
    inp = pair_inputs(c)
    return inp, rr.pair_head_ref_and_bound(inp[0][:, 0], *inp[1:], c.activation)


def np_(t):
    return None if t is None else t.numpy()


def emulate(c, fault=None):
    """the fp32 emulation of the case's kernel (tests/_row_ref.py), outputs as CPU tensors in the order of the kernel's outputs"""
    inp, _ = case_reference(c)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
    if isinstance(c, EmbedCase):
        ids, type_ids, word, pos, type_tab, g, b = inp
        if fault == "pos_row_t" and pos is not None:
            pos = embed_tables(c.hidden)[1]
        return tuple(map(t, rr.emulate_embed(np_(ids), np_(type_ids), np_(word), np_(pos), np_(type_tab), np_(g), np_(b), 1e-12, SEQ, fault)))
    if isinstance(c, LnCase):
        return tuple(map(t, rr.emulate_layernorm(*map(np_, inp), c.eps, fault)))
    if isinstance(c, PoolCase):
        return tuple(map(t, rr.emulate_pool(np_(inp[0]), np_(inp[1]), c.pooling, c.normalize, c.pdim16, fault)))
    return tuple(map(t, rr.emulate_pair_head(*map(np_, inp), c.activation, fault)))


def ratios(c, outs):
    """name -> max |out - ref| / bound of every output of the case that was produced (a NaN counts as infinite)"""
    _, ref = case_reference(c)

    def r(out, want, bound):
        v = rr.ratio(out.float() if out.dtype == torch.float16 else out, want, bound)
        return float("inf") if v != v else v
    if isinstance(c, (EmbedCase, LnCase)):
        return {"x32": r(outs[0], ref[0], ref[1]), "x16": r(outs[1], ref[0], ref[2])}
    if isinstance(c, PoolCase):
        d = {"out": r(outs[0], ref[0], ref[1])}
        if outs[1] is not None:
            d["out16"] = r(outs[1][:, :c.hidden], ref[0], ref[2])
        return d
    d = {"scores": r(outs[0], ref[0], ref[1])}
    if len(outs) > 1 and outs[1] is not None:
        d["pooled"] = r(outs[1], ref[2], ref[3])
    return d


def violations(c, outs):
    """everything a set of outputs of case c must satisfy, as a list of what it does not: the ratios, x16 / out16 as a rounding of the
    fp32 output, and the bit-level claims -- the row of all 0.5 gives beta, a mean-pooled row of length 0 gives +0, out16's padding is +0"""
    bad = [f"{k}: max err / bound = {v:.3g}" for k, v in ratios(c, outs).items() if not v <= 1.0]
    inp, ref = case_reference(c)
    bits = lambda t: t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)
    if isinstance(c, (EmbedCase, LnCase)):
        if not rr.x16_is_a_rounding_of_x32(outs[1], outs[0]):
            bad.append("x16 is not within half an fp16 ulp of x32")
        if isinstance(c, LnCase) and c.half_row is not None and not torch.equal(bits(outs[0][c.half_row]), bits(inp[4])):
            bad.append("the row of all 0.5 is not beta bit for bit")
    elif isinstance(c, PoolCase):
        zero = ref[3]
        if zero.any() and bool((bits(outs[0][zero]) != 0).any()):
            bad.append("a mean-pooled row of length 0 is not the exact zero vector")
        if outs[1] is not None:
            if not rr.x16_is_a_rounding_of_x32(outs[1][:, :c.hidden], outs[0]):
                bad.append("out16 is not within half an fp16 ulp of out")
            if bool((bits(outs[1][:, c.hidden:]) != 0).any()) or (zero.any() and bool((bits(outs[1][zero]) != 0).any())):
                bad.append("out16: padding columns or a zero row are not exact +0")
    return bad
