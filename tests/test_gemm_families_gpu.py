"""GPU: every encoder GEMM kernel family launched on its own (crs_gemm_f16_routed) and compared ELEMENT BY ELEMENT with the fp64 product
of its fp16 operands, under the derived bound of tests/_gemm_ref.py -- the tiled 128 x 128 kernel and the panel kernel (enc_gemm.hip),
the 256 x 256 phase-scheduled kernel one workgroup per item, persistent, in its schedule variants and in split-K form (enc_gemm8.hip),
the 256-row pipelined kernel (enc_gemm_big.hip), the row-streaming kernel and its K = 768 split (enc_gemm_stream.hip).

Every case (tests/_gemm_cases.py) names the kernel with template arguments it must run and asserts it from crs_gemm_plan_describe BEFORE
it launches; on a device whose CU count is not the table's 256 a case whose describe differs is skipped and says so (on an MI355X
nothing skips).  The output is framed by canary rows that must keep their bits, and starts out as NaN bit patterns, so an element the
kernel does not write fails as well.  The knobs are read once per process: the cases of the default setting run here, each other
setting in one fresh child process (pytest on this file), one at a time."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _gemm_cases as gc  # noqa: E402
import _gemm_ref as gr  # noqa: E402

pytestmark = pytest.mark.gpu
SI = gc.setting_here()
HERE = [c for c in gc.GEMM_CASES if c.setting == SI]
CANARY = 8                                   # rows before and after the output: 8 rows keep it 16-byte aligned for every N
NAN16, NAN32 = 0x7E5A, 0x7FC5A5A5            # quiet NaNs

_shared = {}                                 # (m, n, k, slabs) -> inputs and fp64 products, shared by the modes of a shape


def _inputs(c):
    key = (c.m, c.n, c.k, c.slabs if c.mode == 3 else 1)
    if key not in _shared:
        if len(_shared) >= 2:                # the cases of a shape are neighbours in the table: keep little
            _shared.pop(next(iter(_shared)))
        a, w, bias, res = gr.make_inputs(c.m, c.n, c.k)
        _shared[key] = (a, w, bias, res, gr.products(a, w, key[3]))
    return _shared[key]


def framed(rows, n, dtype, device):
    """(whole buffer, view of the middle `rows` rows), every element a NaN pattern"""
    buf = torch.empty((rows + 2 * CANARY, n), dtype=dtype, device=device)
    if dtype == torch.float16:
        buf.view(torch.int16).fill_(NAN16)
    else:
        buf.view(torch.int32).fill_(NAN32)
    return buf, buf[CANARY:CANARY + rows]


def canaries_intact(buf, rows):
    v = buf.view(torch.int16 if buf.dtype == torch.float16 else torch.int32)
    want = NAN16 if buf.dtype == torch.float16 else NAN32
    return bool((v[:CANARY] == want).all()) and bool((v[CANARY + rows:] == want).all())


def expect_kernel(c, text, slabs, cus):
    """the case's kernel name (and slab count) from the describe text; a device the table was not written for skips"""
    kernel = text.split(" grid=")[0]
    if (kernel != c.kernel or slabs != c.slabs) and cus != gc.TABLE_CUS:
        pytest.skip(f"the case table was written for {gc.TABLE_CUS} CUs; this device has {cus} and plans {kernel} with {slabs} slab(s), "
                    f"not {c.kernel} with {c.slabs}")
    assert kernel == c.kernel and slabs == c.slabs, (text, slabs)
    if c.mode == 3:                          # the slab layout the reference assumes (_gemm_ref.slab_ranges)
        assert gc.slab_factor(c, text) == c.slabs, text
    if c.family == "gemm8p":                 # persistent: one workgroup per CU, items just above the CU count and no multiple of it
        items = (c.m // 256) * ((c.n + 255) // 256)
        assert gc.grid_of(text) == (cus, 1, 1) and cus < items < 2 * cus, text


@pytest.mark.parametrize("c", HERE, ids=gc.gemm_id)
def test_gemm_case(cuda, c):
    from rag import _encoder as enc
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    text, slabs = enc.gemm_plan_describe(c.m, c.n, c.k, c.mode, c.route, c.flags)
    expect_kernel(c, text, slabs, cus)
    a, w, bias, res, ps = _inputs(c)
    if not c.bias:
        bias = None
    ref, bound = gr.gemm_ref_and_bound(a, w, bias, res, c.mode, c.slabs, ps=ps)
    rows = c.m * (c.slabs if c.mode == 3 else 1)
    buf, out = framed(rows, c.n, torch.float16 if c.mode < 2 else torch.float32, cuda)
    dev = [t.to(cuda) if t is not None else None for t in (a, w, bias, res if c.mode == 2 else None)]
    enc.gemm_f16_routed(dev[0], dev[1], dev[2], dev[3], out, c.mode, c.route, c.flags)
    torch.cuda.synchronize()
    assert canaries_intact(buf, rows)
    got = out.cpu().reshape(ref.shape)
    ratio = gr.ratio(got, ref, bound)
    print(f"{gc.RATIO_TAG} {c.family} mode {c.mode} {ratio:.4f} {gc.gemm_id(c)} setting {SI}")
    assert ratio <= 1.0                      # (a NaN left in the output compares false)
    assert all(torch.equal(d.cpu(), h) for d, h in zip(dev, (a, w, bias, res)) if d is not None)   # the operands were only read


@pytest.mark.parametrize("si", [i for i in range(1, len(gc.SETTINGS)) if any(c.setting == i for c in gc.GEMM_CASES)])
def test_setting_in_child_process(cuda, si):
    n = sum(c.setting == si for c in gc.GEMM_CASES)
    skipped = gc.run_setting_child(os.path.abspath(__file__), si, "test_gemm_case", n)
    if skipped:
        pytest.skip(f"{skipped} of {n} cases skipped in the child: the case table was written for {gc.TABLE_CUS} CUs")


def test_refusals(cuda):
    """CRS_EINVAL before any launch: a route's modes, a bias with mode 3, a shape the split-K form does not take, K that has no panel
    chunk, an unaligned pointer, a missing residual."""
    from rag import _encoder as enc
    from rag import _native as nat
    a = torch.zeros((256, 192), dtype=torch.float16, device=cuda)
    w = torch.zeros((256, 192), dtype=torch.float16, device=cuda)
    bias = torch.zeros(256 + 4, dtype=torch.float32, device=cuda)
    out = torch.zeros((2, 256, 256), dtype=torch.float32, device=cuda)
    for kw in (dict(mode=3, route=0), dict(mode=2, route=1), dict(mode=0, route=2), dict(mode=3, route=2), dict(mode=0, route=3),
               dict(mode=0, route=1)):                                    # (192 = 3 x 64 has no 128-column chunk)
        with pytest.raises(nat.NativeError):
            enc.gemm_f16_routed(a, w, None, None, out, **kw)
        with pytest.raises(nat.NativeError):
            enc.gemm_plan_describe(256, 256, 192, kw["mode"], kw["route"])
    with pytest.raises(nat.NativeError):
        enc.gemm_f16_routed(a[:, :128].contiguous(), w[:, :128].contiguous(), bias[:256], None, out, mode=3, route=1)   # bias with mode 3
    with pytest.raises(nat.NativeError):
        enc.gemm_f16_routed(a, w, bias[1:257], None, out, mode=0, route=0)                                              # 4-byte aligned
    with pytest.raises(nat.NativeError):
        enc.gemm_f16_routed(a, w, bias[:256], None, out, mode=2, route=0)                                               # no residual
    torch.cuda.synchronize()
    assert not out.any()
