"""GPU: the out-projection / FFN-down + LayerNorm step of a layer on its own (crs_proj_ln_f16, the function the forward runs), on each of
its four routes -- the fused projection + LayerNorm kernel of enc_rowln.hip in both ring forms, split-K panel slabs + LayerNorm, split-K
slabs of the 256 x 256 kernel + LayerNorm, the mode-2 tiled GEMM + the generic LayerNorm -- element by element against the fp64
LayerNorm of the fp64 product, under the first-order bound of tests/_gemm_ref.py (x32 and x16 separately).

Every case asserts its kernels from crs_proj_ln_plan_describe before it launches.  x32 is the residual and is updated in place, as in
the forward; x32, x16 and the slab workspace are framed by canary rows (128 behind: the rows past `tokens` in the fused kernel's last
128-row block must stay untouched).  LayerNorm gains and biases are distinct per column.  CRS_ROWLN2_VARIANT=0 runs in a fresh child."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as gc  # noqa: E402
import _gemm_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu
SI = gc.setting_here()
HERE = [c for c in gc.PROJ_LN_CASES if c.setting == SI]
FRONT, BACK = 8, 128
NAN16, NAN32 = 0x7E5A, 0x7FC5A5A5
EPS = 1e-12

_shared = {}


def _inputs(c):
    key = (c.tokens, c.hidden, c.k)
    if key not in _shared:
        _shared.clear()
        a, w, bias, res = gr.make_inputs(c.tokens, c.hidden, c.k)
        gen = torch.Generator().manual_seed(c.tokens + c.k)
        g = gr.distinct(1.0 + 0.1 * torch.randn(c.hidden, generator=gen))
        b = gr.distinct(0.1 * torch.randn(c.hidden, generator=gen))
        _shared[key] = (a, w, bias, res, g, b, gr.products(a, w, 1))
    return _shared[key]


def framed(rows, n, dtype, device):
    buf = torch.empty((FRONT + rows + BACK, n), dtype=dtype, device=device)
    buf.view(torch.int16 if dtype == torch.float16 else torch.int32).fill_(NAN16 if dtype == torch.float16 else NAN32)
    return buf, buf[FRONT:FRONT + rows]


def canaries_intact(buf, rows):
    v = buf.view(torch.int16 if buf.dtype == torch.float16 else torch.int32)
    want = NAN16 if buf.dtype == torch.float16 else NAN32
    return bool((v[:FRONT] == want).all()) and bool((v[FRONT + rows:] == want).all())


@pytest.mark.parametrize("c", HERE, ids=gc.proj_ln_id)
def test_proj_ln_case(cuda, c):
    from rag import _encoder as enc
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    text, slabs = enc.proj_ln_plan_describe(c.tokens, c.hidden, c.k, c.flags, c.big_ln)
    kernels = tuple(line.split(" grid=")[0] for line in text.splitlines())
    if (kernels != c.kernels or slabs != c.slabs) and cus != gc.TABLE_CUS:
        pytest.skip(f"the case table was written for {gc.TABLE_CUS} CUs; this device has {cus} and plans {kernels}, not {c.kernels}")
    assert kernels == c.kernels and slabs == c.slabs, text
    a, w, bias, res, g, b, ps = _inputs(c)
    ref, b32, b16, second, a_term = gr.proj_ln_ref_and_bound(a, w, bias, res, g, b, EPS, c.slabs, ps=ps)
    assert second < 0.01, f"inadmissible case: second-order term {second:.2e} of the bound"
    t, h = c.tokens, c.hidden
    xbuf, x32 = framed(t, h, torch.float32, cuda)
    hbuf, x16 = framed(t, h, torch.float16, cuda)
    ybuf, y32 = framed(c.slabs * t, h, torch.float32, cuda)
    x32.copy_(res)                                           # the residual stream, updated in place
    dev = [v.to(cuda) for v in (a, w, bias, g, b)]
    enc.proj_ln_f16(dev[0], dev[1], dev[2], dev[3], dev[4], EPS, y32, x32, x16, c.flags, c.big_ln)
    torch.cuda.synchronize()
    assert canaries_intact(xbuf, t) and canaries_intact(hbuf, t) and canaries_intact(ybuf, c.slabs * t)
    r32, r16 = gr.ratio(x32.cpu(), ref, b32), gr.ratio(x16.cpu(), ref, b16)
    print(f"{gc.RATIO_TAG} projln-{c.kernels[0].split('<')[0]}-x32 mode - {r32:.4f} {gc.proj_ln_id(c)} setting {SI}")
    print(f"{gc.RATIO_TAG} projln-{c.kernels[0].split('<')[0]}-x16 mode - {r16:.4f} {gc.proj_ln_id(c)} setting {SI} (a = {a_term:.1e}, second order {second:.1e})")
    assert r32 <= 1.0 and r16 <= 1.0
    # x16 is the fp16 rounding of the value x32 is the fp32 rounding of (one rounding each: the compiler may round the last
    # multiply-add to fp16 directly, so x16 need not equal x32.half() bit for bit)
    x = x32.cpu().double()
    assert ((x16.cpu().double() - x).abs() <= gr.half_ulp16(x.abs() * (1 + 2.0 ** -23)) + x.abs() * 2.0 ** -24).all()
    assert all(torch.equal(d.cpu(), v) for d, v in zip(dev, (a, w, bias, g, b)))


@pytest.mark.parametrize("si", [i for i in range(1, len(gc.SETTINGS)) if any(c.setting == i for c in gc.PROJ_LN_CASES)])
def test_setting_in_child_process(cuda, si):
    n = sum(c.setting == si for c in gc.PROJ_LN_CASES)
    skipped = gc.run_setting_child(os.path.abspath(__file__), si, "test_proj_ln_case", n)
    if skipped:
        pytest.skip(f"{skipped} of {n} cases skipped in the child: the case table was written for {gc.TABLE_CUS} CUs")


def test_refusals(cuda):
    from rag import _encoder as enc
    from rag import _native as nat
    for tokens, hidden, k in [(0, 384, 384), (64, 100, 384), (64, 1088, 384), (64, 384, 100)]:
        with pytest.raises(nat.NativeError):
            enc.proj_ln_plan_describe(tokens, hidden, k)
    a = torch.zeros((64, 384), dtype=torch.float16, device=cuda)
    v = torch.zeros(384 + 4, dtype=torch.float32, device=cuda)
    x32 = torch.zeros((64, 384), dtype=torch.float32, device=cuda)
    with pytest.raises(nat.NativeError):                     # a 4-byte aligned bias
        enc.proj_ln_f16(a, torch.zeros((384, 384), dtype=torch.float16, device=cuda), v[1:385], v[:384], v[:384], EPS, x32.clone(), x32,
                        torch.zeros_like(a))
    with pytest.raises(nat.NativeError):                     # no bias
        enc.proj_ln_f16(a, torch.zeros((384, 384), dtype=torch.float16, device=cuda), None, v[:384], v[:384], EPS, x32.clone(), x32,
                        torch.zeros_like(a))
