"""GPU: the encoder's HBM-bound row kernels launched on their own (crs_embed_ln_f32, crs_layernorm_f32, crs_pool_f32, crs_pair_head_f32)
and compared ELEMENT BY ELEMENT with the fp64 reference of their exact inputs under the derived bounds of tests/_row_ref.py: the eight
embedding + LayerNorm forms, the 28 LayerNorm forms (4 row forms x 7 slab counts), pool_kernel and pair_head_kernel<1> / <2>.

Every case (tests/_row_cases.py) names the kernel instantiation and grid it must run and asserts the line of crs_row_plan_describe
BEFORE it launches.  Outputs are framed by canary rows that must keep their bits and start out as NaN bit patterns (an element the
kernel does not write fails); every operand sits between NaN guard blocks inside one larger allocation, so a stray read shows as NaN
without any access outside an allocation, and must keep its bits.  Two launches must agree bit for bit.  The bit-level claims of the
kernels' comments are asserted: all-zero type ids give the bits of the untyped embedding launch; LayerNorm in place (residual == x32)
gives the bits of the launch with a separate residual; a row of all 0.5 gives beta; a mean-pooled row of length 0 is exact +0 and so
is out16's padding; a pair's score and pooled row do not depend on its place in the group or on the batch it came in.  The kernels
read no environment knobs: everything runs in this process."""
import os
import sys
from ctypes import c_float, c_void_p

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _row_cases as rc  # noqa: E402
import _row_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 8                   # rows before and after an output
GUARD = 1024                 # NaN elements (4 KB) before and after an operand
NAN16, NAN32 = rr.NAN16, rr.NAN32


def ibits(t):
    return t.view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def framed(rows, n, dtype, device):
    buf = torch.empty((rows + 2 * CANARY, n), dtype=dtype, device=device)
    ibits(buf).fill_(NAN16 if dtype == torch.float16 else NAN32)
    return buf, buf[CANARY:CANARY + rows]


def canaries_intact(buf, rows):
    v, want = ibits(buf), (NAN16 if buf.dtype == torch.float16 else NAN32)
    return bool((v[:CANARY] == want).all()) and bool((v[CANARY + rows:] == want).all())


def unwritten(out):
    return bool((ibits(out) == (NAN16 if out.dtype == torch.float16 else NAN32)).any())


class Guarded:
    """fp32 / int32 operands, each between GUARD elements of NaN patterns inside its own allocation"""

    def __init__(self, device):
        self.device, self.bufs = device, []

    def __call__(self, t):
        if t is None:
            return None
        buf = torch.empty(t.numel() + 2 * GUARD, dtype=torch.int32, device=self.device)
        buf.fill_(NAN32)
        mid = buf[GUARD:GUARD + t.numel()]
        mid.copy_(t.contiguous().view(torch.int32).flatten())
        self.bufs.append((buf, buf.clone()))
        return mid.view(t.dtype).view(t.shape)

    def intact(self):
        return all(torch.equal(buf, before) for buf, before in self.bufs)


def check(c, outs, enc):
    """print the ratios, assert everything tests/_row_cases.py asks of the outputs of case c"""
    outs = tuple(None if o is None else o.cpu() for o in outs)
    for name, r in rc.ratios(c, outs).items():
        print(f"{rc.RATIO_TAG} {c.kernel} {r:.4f} {c.id}/{name}")
    assert rc.violations(c, outs) == []


def same_bits(a, b):
    return all((x is None and y is None) or torch.equal(ibits(x), ibits(y)) for x, y in zip(a, b))


def describe_first(c, enc):
    text = enc.row_plan_describe(*c.describe)
    assert text == c.line and text.split(" grid=")[0] == c.kernel, text


@pytest.mark.parametrize("c", rc.EMBED_CASES, ids=rc.case_id)
def test_embed_case(cuda, c):
    from rag import _encoder as enc
    describe_first(c, enc)
    (ids, type_ids, word, pos, type_tab, g, b), ref = rc.case_reference(c)
    assert ref[3] < rr.SECOND_ORDER_LIMIT, f"inadmissible case: second-order term {ref[3]:.2e} of the bound"
    guard = Guarded(cuda)
    d_ids, d_ty, d_word, d_pos, d_tab, d_g, d_b = map(guard, (ids, type_ids, word, pos, type_tab, g, b))

    def launch(ty):
        xb, x32 = framed(c.tokens, c.hidden, torch.float32, cuda)
        hb, x16 = framed(c.tokens, c.hidden, torch.float16, cuda)
        enc.embed_ln_f32(d_ids, ty, d_word, d_pos, d_tab, d_g, d_b, 1e-12, rc.SEQ, x32, x16)
        return (xb, hb), (x32, x16)
    runs = [launch(d_ty), launch(d_ty)]
    if c.typed:              # "an all-zero type block gives the bits of the plain form"
        plain = rc.EmbedCase(c.hidden, c.tokens, False, 1, c.pos)
        assert enc.row_plan_describe(*plain.describe) == plain.line
        runs += [launch(guard(torch.zeros(c.tokens, dtype=torch.int32))), launch(None)]
    torch.cuda.synchronize()
    assert all(canaries_intact(buf, c.tokens) for bufs, _ in runs for buf in bufs)
    assert guard.intact()
    check(c, runs[0][1], enc)
    assert same_bits(runs[0][1], runs[1][1]), "two launches differ"
    if c.typed:
        assert same_bits(runs[2][1], runs[3][1]), "all-zero type ids do not give the bits of the untyped launch"
        assert not unwritten(runs[3][1][0]) and not unwritten(runs[3][1][1])
        if c.type_rows == 1:  # every type id clamps to row 0
            assert same_bits(runs[0][1], runs[3][1])


@pytest.mark.parametrize("c", rc.LN_CASES, ids=rc.case_id)
def test_layernorm_case(cuda, c):
    from rag import _encoder as enc
    describe_first(c, enc)
    (y, bias, res, g, b), ref = rc.case_reference(c)
    assert ref[3] < rr.SECOND_ORDER_LIMIT, f"inadmissible case: second-order term {ref[3]:.2e} of the bound"
    guard = Guarded(cuda)
    d_y, d_bias, d_res, d_g, d_b = map(guard, (y, bias, res, g, b))

    def launch(in_place):
        xb, x32 = framed(c.tokens, c.hidden, torch.float32, cuda)
        hb, x16 = framed(c.tokens, c.hidden, torch.float16, cuda)
        if in_place:
            x32.copy_(d_res)
        enc.layernorm_f32(d_y, d_bias, x32 if in_place else d_res, d_g, d_b, c.eps, x32, x16)
        return (xb, hb), (x32, x16)
    runs = [launch(False), launch(False)] + ([launch(True)] if c.residual else [])
    torch.cuda.synchronize()
    assert all(canaries_intact(buf, c.tokens) for bufs, _ in runs for buf in bufs)
    assert guard.intact()
    check(c, runs[0][1], enc)
    assert same_bits(runs[0][1], runs[1][1]), "two launches differ"
    if c.residual:
        assert same_bits(runs[0][1], runs[2][1]), "in place (residual == x32) differs from a separate residual"


@pytest.mark.parametrize("c", rc.POOL_CASES, ids=rc.case_id)
def test_pool_case(cuda, c):
    from rag import _encoder as enc
    describe_first(c, enc)
    (x, lens), ref = rc.case_reference(c)
    guard = Guarded(cuda)
    d_x, d_lens = guard(x), guard(lens)

    def launch():
        ob, out = framed(c.batch, c.hidden, torch.float32, cuda)
        hb, out16 = framed(c.batch, c.pdim16, torch.float16, cuda) if c.out16 >= 0 else (None, None)
        enc.pool_f32(d_x, d_lens, c.pooling, c.normalize, out, out16, max(c.out16, 0))
        return (ob, hb), (out, out16)
    runs = [launch(), launch()]
    torch.cuda.synchronize()
    assert all(buf is None or canaries_intact(buf, c.batch) for bufs, _ in runs for buf in bufs)
    assert guard.intact()
    check(c, runs[0][1], enc)
    assert same_bits(runs[0][1], runs[1][1]), "two launches differ"


@pytest.mark.parametrize("c", rc.PAIR_CASES, ids=rc.case_id)
def test_pair_head_case(cuda, c):
    from rag import _encoder as enc
    describe_first(c, enc)
    inp, ref = rc.case_reference(c)
    guard = Guarded(cuda)
    dev = list(map(guard, inp))

    def launch():
        sb, scores = framed(c.batch, 1, torch.float32, cuda)
        pb, pooled = framed(c.batch, c.hidden, torch.float32, cuda) if c.pooled_out else (None, None)
        enc.pair_head_f32(*dev, c.activation, scores, pooled)
        return (sb, pb), (scores[:, 0], pooled)
    runs = [launch(), launch()]
    torch.cuda.synchronize()
    assert all(buf is None or canaries_intact(buf, c.batch) for bufs, _ in runs for buf in bufs)
    assert guard.intact()
    check(c, runs[0][1], enc)
    assert same_bits(runs[0][1], runs[1][1]), "two launches differ"


@pytest.mark.parametrize("hidden", (64, 192, 128, 384, 768, 1024))
def test_a_pair_does_not_depend_on_its_place(cuda, hidden):
    """the same pair as row 0 of a batch of 1 and as row 6 of a batch of 9 (groups of 8: the second to last slot of the first group):
    the same score and pooled bits, with NaN patterns in every other token"""
    from rag import _encoder as enc
    x9 = rc.pair_hidden(hidden, 9, 3)
    guard = Guarded(cuda)
    d9, d1 = guard(x9), guard(x9[6:7].clone())
    w = list(map(guard, rc.pair_weights(hidden)))
    got = []
    for act in (0, 1):
        for d, batch in ((d9, 9), (d1, 1)):
            sb, scores = framed(batch, 1, torch.float32, cuda)
            pb, pooled = framed(batch, hidden, torch.float32, cuda)
            enc.pair_head_f32(d, *w, act, scores, pooled)
            got.append((sb, pb, scores, pooled, batch))
    torch.cuda.synchronize()
    assert all(canaries_intact(sb, n) and canaries_intact(pb, n) for sb, pb, _, _, n in got) and guard.intact()
    for nine, one in ((got[0], got[1]), (got[2], got[3])):
        assert not unwritten(nine[2]) and not unwritten(nine[3]) and not unwritten(one[2]) and not unwritten(one[3])
        assert torch.equal(ibits(nine[2][6]), ibits(one[2][0])), "the score depends on the pair's place"
        assert torch.equal(ibits(nine[3][6]), ibits(one[3][0])), "the pooled row depends on the pair's place"


def test_the_table_launches_every_instantiation():
    """every case asserts its line before it launches, so the kernels of the table are the kernels launched"""
    assert {c.kernel for c in rc.ALL_CASES} == set(rc.INSTANTIATIONS) and len(rc.INSTANTIATIONS) == 8 + 28 + 1 + 2


def _ptr(t, shift=0):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr() + shift)


def test_refusals(cuda):
    """CRS_EINVAL before any launch, outputs untouched: every condition of include/crs_encoder.h, with buffers large enough for the
    launch that must not happen; the accepted call next to the refused ones does launch."""
    from rag import _native as nat
    import rag._encoder  # noqa: F401  (registers the signatures)
    lib = nat.load()
    st = nat._stream_ptr()
    H, T = 1088, 64                                  # the largest sizes any refused call names
    z32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=cuda)
    zi = lambda *s: torch.zeros(s, dtype=torch.int32, device=cuda)
    ids, lens, tab, vec, y = zi(T + 4), zi(T + 4), z32(40, H), z32(H + 4), z32(16, T, H)
    x32b, x32 = framed(T, H, torch.float32, cuda)
    x16b, x16 = framed(T, H, torch.float16, cuda)
    frames = [(x32b, T), (x16b, T)]           # the accepted calls write a small block that lies flat at the start of row 0
    P = lambda t, s=0: (t, s)

    def run(fn, order, ok, bad, written):
        for kw in bad:
            a = dict(ok)
            a.update(kw)
            assert fn(*[_ptr(*a[k]) if isinstance(a[k], tuple) else a[k] for k in order], st) == -1, (fn.__name__, kw)   # CRS_EINVAL
            assert lib.crs_last_error()
        torch.cuda.synchronize()
        assert all(bool((ibits(buf) == (NAN16 if buf.dtype == torch.float16 else NAN32)).all()) for buf, _ in frames), fn.__name__
        assert fn(*[_ptr(*ok[k]) if isinstance(ok[k], tuple) else ok[k] for k in order], st) == 0, fn.__name__
        torch.cuda.synchronize()
        assert all(not unwritten(w) for w in written) and all(canaries_intact(buf, n) for buf, n in frames), fn.__name__
        for buf, _ in frames:
            ibits(buf).fill_(NAN16 if buf.dtype == torch.float16 else NAN32)

    hidden_bad = [dict(hidden=0), dict(hidden=100), dict(hidden=1088), dict(hidden=-64)]
    ok = dict(ids=P(ids), ty=P(ids), type_rows=2, word=P(tab), pos=P(tab), tab=P(tab), g=P(vec), b=P(vec), eps=c_float(1e-12), tokens=8,
              seq=4, hidden=128, vocab=37, x32=P(x32), x16=P(x16))
    bad = [dict(ids=P(None)), dict(word=P(None)), dict(tab=P(None)), dict(g=P(None)), dict(b=P(None)), dict(x32=P(None)), dict(x16=P(None)),
           dict(ids=P(ids, 4)), dict(ty=P(ids, 8)), dict(word=P(tab, 4)), dict(pos=P(tab, 8)), dict(tab=P(tab, 4)), dict(g=P(vec, 4)),
           dict(b=P(vec, 8)), dict(x32=P(x32, 8)), dict(x16=P(x16, 2)), dict(tokens=0), dict(seq=0), dict(tokens=-1),
           # (a table of no rows clamps to row -1: the pointer stands two rows into the allocation)
           dict(vocab=0, word=P(tab, 2 * H * 4)), dict(type_rows=0, tab=P(tab, 2 * H * 4))] + hidden_bad
    run(lib.crs_embed_ln_f32, ("ids", "ty", "type_rows", "word", "pos", "tab", "g", "b", "eps", "tokens", "seq", "hidden", "vocab", "x32",
                               "x16"), ok, bad, [x32[0, :8 * 128], x16[0, :8 * 128]])

    ok = dict(y=P(y), nsplit=2, bias=P(vec), res=P(tab), g=P(vec), b=P(vec), eps=c_float(1e-12), tokens=8, hidden=128, x32=P(x32), x16=P(x16))
    bad = [dict(y=P(None)), dict(g=P(None)), dict(b=P(None)), dict(x32=P(None)), dict(x16=P(None)),
           dict(y=P(y, 4)), dict(bias=P(vec, 4)), dict(res=P(tab, 8)), dict(g=P(vec, 8)), dict(b=P(vec, 4)), dict(x32=P(x32, 4)),
           dict(x16=P(x16, 8)), dict(tokens=0), dict(nsplit=0), dict(nsplit=5), dict(nsplit=7), dict(nsplit=12), dict(nsplit=32),
           dict(nsplit=-1)] + hidden_bad
    run(lib.crs_layernorm_f32, ("y", "nsplit", "bias", "res", "g", "b", "eps", "tokens", "hidden", "x32", "x16"), ok, bad,
        [x32[0, :8 * 128], x16[0, :8 * 128]])

    ok = dict(x=P(y), lens=P(lens), batch=4, seq=8, hidden=128, pooling=0, normalize=1, out=P(x32), out16=P(x16), slab=0)
    bad = [dict(x=P(None)), dict(lens=P(None)), dict(out=P(None)), dict(x=P(y, 8)), dict(lens=P(lens, 4)), dict(out=P(x32, 4)),
           dict(out16=P(x16, 2)), dict(batch=0), dict(seq=0), dict(pooling=2), dict(pooling=-1), dict(slab=2), dict(slab=-1),
           dict(slab=2, out16=P(None))] + hidden_bad
    run(lib.crs_pool_f32, ("x", "lens", "batch", "seq", "hidden", "pooling", "normalize", "out", "out16", "slab"), ok, bad,
        [x32[:1, :512].reshape(-1)[:4 * 128], x16[:1, :512].reshape(-1)[:4 * 128]])

    wp = z32(H, H)
    ok = dict(h=P(y), batch=4, seq=2, hidden=128, wp=P(wp), bp=P(vec), wc=P(vec), bc=P(vec), act=0, scores=P(x32), pooled=P(x16b.view(torch.float32)[CANARY:]))
    bad = [dict(h=P(None)), dict(wp=P(None)), dict(bp=P(None)), dict(wc=P(None)), dict(bc=P(None)), dict(scores=P(None)),
           dict(h=P(y, 4)), dict(wp=P(wp, 8)), dict(bp=P(vec, 4)), dict(wc=P(vec, 8)), dict(bc=P(vec, 4)), dict(scores=P(x32, 4)),
           dict(pooled=P(x32, 8)), dict(batch=0), dict(seq=0), dict(act=2), dict(act=-1)] + hidden_bad
    run(lib.crs_pair_head_f32, ("h", "batch", "seq", "hidden", "wp", "bp", "wc", "bc", "act", "scores", "pooled"), ok, bad,
        [x32[:1, :4].reshape(-1), x16[:1, :4 * 128 * 2].reshape(-1)])
