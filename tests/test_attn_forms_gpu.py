"""GPU: every attention kernel instantiation launched on its own (crs_attention_f16, crs_qkv_attn_f16) and compared ELEMENT BY ELEMENT
with the fp64 attention of its fp16 operands under the derived bound of tests/_attn_ref.py -- the blocked kernel without and with a
relative-position bias, the short kernel, the 16-deep and 32-deep whole-sequence kernels (csrc/enc_attn.hip) and the fused QKV
projection + attention kernel (csrc/enc_qkvattn.hip).

Every case (tests/_attn_cases.py) names the kernel with template arguments it must run and asserts it, and the grid, from
crs_attention_plan_describe BEFORE it launches; the route sets the planner's knobs per call, so every form runs in this process.  ctx is
framed by canary rows that must keep their bits and starts out as NaN bit patterns (an element the kernel does not write fails); the
operand sits between NaN guard rows inside one larger allocation, so a read outside the tensor that reaches an MFMA shows as NaN
without any access outside an allocation, and must keep its bits.  Two launches must agree bit for bit, and the 16-deep whole-sequence
kernel must agree bit for bit with the blocked kernel (the claim of its comment)."""
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_cases as ac  # noqa: E402
import _attn_ref as ar  # noqa: E402

pytestmark = pytest.mark.gpu
CANARY = 8                   # ctx rows before and after the output
GUARD = 64                   # NaN rows before and after an operand: a whole key block
NAN16 = 0x7E5A               # a quiet NaN


def framed_ctx(rows, hidden, device):
    buf = torch.empty((rows + 2 * CANARY, hidden), dtype=torch.float16, device=device)
    buf.view(torch.int16).fill_(NAN16)
    return buf, buf[CANARY:CANARY + rows]


def canaries_intact(buf, rows):
    v = buf.view(torch.int16)
    return bool((v[:CANARY] == NAN16).all()) and bool((v[CANARY + rows:] == NAN16).all())


def guarded(arr, device):
    """(whole buffer, view of the middle rows holding arr) -- fp16 [rows, cols] between GUARD rows of NaN patterns"""
    rows, cols = arr.shape
    buf = torch.empty((rows + 2 * GUARD, cols), dtype=torch.float16, device=device)
    buf.view(torch.int16).fill_(NAN16)
    mid = buf[GUARD:GUARD + rows]
    mid.copy_(torch.from_numpy(arr))
    return buf, mid


def describe(enc, c, route=None):
    return enc.attention_plan_describe(c.batch, c.seq, c.heads * c.hd, c.heads, c.span != 0, c.route if route is None else route)


@pytest.mark.parametrize("c", ac.CASES, ids=ac.attn_id)
def test_attn_case(cuda, c):
    from rag import _encoder as enc
    hidden, rows = c.heads * c.hd, c.batch * c.seq
    text = describe(enc, c)
    assert text.split(" grid=")[0] == c.kernel and ac.grid_of(text) == ac.expected_grid(c), text
    if c.form == "bias":         # "the other attention forms are not selected"
        assert all(describe(enc, c, r) == text for r in (0, 1, 2, 4, 8))
    inp, ref, bound, _ = ac.case_reference(c)
    lens = torch.tensor(c.lens, dtype=torch.int32, device=cuda)
    opbuf, op = guarded(inp[0], cuda)
    before = opbuf.view(torch.int16).clone()
    if c.form == "fused":
        w, bq = torch.from_numpy(inp[1]).to(cuda), torch.from_numpy(inp[2]).to(cuda)
        launch = lambda out, route: enc.qkv_attn_f16(op, w, bq, lens, out, c.batch, c.seq, c.heads)
    else:
        bias = torch.from_numpy(inp[1]).to(cuda) if c.span else None
        launch = lambda out, route: enc.attention_f16(op, lens, out, c.batch, c.seq, c.heads, bias, route)
    outs = []
    for _ in range(2):
        buf, out = framed_ctx(rows, hidden, cuda)
        launch(out, c.route)
        outs.append((buf, out))
    if c.form == "seq":          # the blocked kernel on the same input
        assert describe(enc, c, 1).split(" grid=")[0] == f"attention_kernel<{c.hd}, false>"
        buf, out = framed_ctx(rows, hidden, cuda)
        launch(out, 1)
        outs.append((buf, out))
    torch.cuda.synchronize()
    assert all(canaries_intact(buf, rows) for buf, _ in outs)
    assert torch.equal(opbuf.view(torch.int16), before) and lens.cpu().tolist() == list(c.lens)      # the operands were only read
    if c.form == "fused":
        assert torch.equal(w.cpu(), torch.from_numpy(inp[1])) and torch.equal(bq.cpu(), torch.from_numpy(inp[2]))
    elif c.span:
        assert torch.equal(bias.cpu(), torch.from_numpy(inp[1]))
    got = outs[0][1].cpu().numpy()
    r = ar.ratio(got, ref, bound)
    print(f"{ac.RATIO_TAG} {r:.4f} {ac.attn_id(c)} | {c.kernel}")
    assert r <= 1.0              # (a NaN left in the output counts as infinite)
    assert torch.equal(outs[0][1].view(torch.int16), outs[1][1].view(torch.int16)), "two launches differ"
    if c.form == "seq":
        same = torch.equal(outs[0][1].view(torch.int16), outs[2][1].view(torch.int16))
        print(f"attn-bit-equal {c.kernel} vs attention_kernel<{c.hd}, false>: {same} {ac.attn_id(c)}")
        assert same, "attention_seq_kernel is not bit-equal to the blocked kernel"


def test_the_table_launches_every_instantiation():
    assert {c.kernel for c in ac.CASES} == set(ac.INSTANTIATIONS)


def _ptr(t, shift=0):
    return c_void_p(0) if t is None else c_void_p(t.data_ptr() + shift)


def test_refusals(cuda):
    """CRS_EINVAL before any launch, ctx untouched: every condition of include/crs_encoder.h, with buffers large enough for the launch
    that must not happen."""
    from rag import _native as nat
    import rag._encoder  # noqa: F401  (registers the signatures)
    lib = nat.load()
    st = nat._stream_ptr()
    qkv = torch.zeros((65536, 48), dtype=torch.float16, device=cuda)            # batch 65536 x seq 1 x hidden 16; 513 x 192; ...
    lens = torch.ones(65536 + 4, dtype=torch.int32, device=cuda)
    ctxbuf, ctx = framed_ctx(65536, 16, cuda)
    bias = torch.zeros((2, 2 * 520 - 1), dtype=torch.float32, device=cuda)
    ok = dict(qkv=(qkv, 0), lens=(lens, 0), ctx=(ctx, 0), batch=4, seq=16, hidden=64, heads=2, bias=(None, 0), span=0, route=0)

    def attention(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.crs_attention_f16(_ptr(*a["qkv"]), _ptr(*a["lens"]), _ptr(*a["ctx"]), a["batch"], a["seq"], a["hidden"], a["heads"],
                                     _ptr(*a["bias"]), a["span"], a["route"], st)
    bad = [dict(qkv=(None, 0)), dict(lens=(None, 0)), dict(ctx=(None, 0)),                      # null pointers
           dict(qkv=(qkv, 2)), dict(lens=(lens, 4)), dict(ctx=(ctx, 8)), dict(bias=(bias, 4), span=520),   # not 16-byte aligned
           dict(hidden=64, heads=3), dict(hidden=128, heads=1), dict(hidden=24, heads=3),       # hidden % heads, head_dim 128 and 8
           dict(batch=0), dict(batch=65536, seq=1, hidden=16, heads=1), dict(seq=0), dict(route=16),
           dict(bias=(bias, 0), span=520, seq=513, batch=1, hidden=32), dict(bias=(bias, 0), span=15)]          # seq > 512, rel_span < seq
    for kw in bad:
        assert attention(**kw) == -1, kw                                                         # CRS_EINVAL
        assert lib.crs_last_error()
    x16 = torch.zeros((4112, 384), dtype=torch.float16, device=cuda)
    w = torch.zeros((3 * 512, 512), dtype=torch.float16, device=cuda)
    bq = torch.zeros(3 * 512 + 4, dtype=torch.float32, device=cuda)
    fctxbuf, fctx = framed_ctx(4112, 512, cuda)
    fok = dict(x=(x16, 0), w=(w, 0), b=(bq, 0), lens=(lens, 0), ctx=(fctx, 0), batch=4, seq=16, hidden=128, heads=4)

    def fused(**kw):
        a = dict(fok)
        a.update(kw)
        return lib.crs_qkv_attn_f16(_ptr(*a["x"]), _ptr(*a["w"]), _ptr(*a["b"]), _ptr(*a["lens"]), _ptr(*a["ctx"]), a["batch"], a["seq"],
                                    a["hidden"], a["heads"], st)
    fbad = [dict(x=(None, 0)), dict(w=(None, 0)), dict(b=(None, 0)), dict(lens=(None, 0)), dict(ctx=(None, 0)),
            dict(x=(x16, 2)), dict(b=(bq, 4)), dict(ctx=(fctx, 8)),
            dict(heads=3), dict(heads=1), dict(heads=8), dict(batch=0), dict(batch=65536), dict(seq=0),
            dict(seq=48), dict(seq=128), dict(hidden=512, heads=16), dict(hidden=384, heads=6), dict(hidden=192, heads=6), dict(batch=257)]
    for kw in fbad:
        assert fused(**kw) == -1, kw
    torch.cuda.synchronize()
    for buf in (ctxbuf, fctxbuf):
        assert bool((buf.view(torch.int16) == NAN16).all())
    # ... and the accepted call next to them launches
    assert attention() == 0 and fused() == 0
    torch.cuda.synchronize()
    assert not bool((ctx[:64].view(torch.int16) == NAN16).any()) and not bool((fctx[:16].view(torch.int16) == NAN16).any())
