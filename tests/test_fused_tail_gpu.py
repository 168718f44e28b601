"""GPU: crs_cosine_topk_cert's fused tail (csrc/finish.hip) against the three-kernel chain it replaces, and the scan's
non-temporal slab stream against the default policy.

CRS_FUSED_TAIL=0 makes crs_cosine_topk_cert run crs_cosine_topk + crs_refine_f32_cert (merge, tile refine, fp32 re-rank +
certificate); the default runs the scan and ONE kernel.  Both must leave the same bits in every output: the k' candidates
(scores + ids), the k best (scores + ids), the status words and the escalation threshold in the exactness workspace.
CRS_SCAN_NT=1 / 0 forces the slab stream's cache policy; the scan's lists must not depend on it."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


class _Env:
    def __init__(self, **kv):
        self.kv = {k: str(v) for k, v in kv.items()}

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_STORES = {}


def _store(cuda, n, d, dups=0):
    """fp16 slab + fp32 shadow of n random unit rows (seeded); the last `dups` rows repeat row 7 (exact ties)"""
    import torch
    from rag import _native as nat
    key = (n, d, dups)
    if key in _STORES:
        return _STORES[key]
    _STORES.clear()
    torch.cuda.empty_cache()
    g = torch.Generator(device=cuda)
    g.manual_seed(n + d)
    pd = nat.padded_dim(d)
    slab = torch.zeros((n, pd), dtype=torch.float16, device=cuda)
    shadow = torch.empty((n, d), dtype=torch.float32, device=cuda)
    row_err = torch.zeros(1, dtype=torch.float32, device=cuda)
    for lo in range(0, n, 500_000):
        m = min(500_000, n - lo)
        x = torch.nn.functional.normalize(torch.randn((m, d), generator=g, device=cuda), dim=1)
        if dups and lo + m > n - dups:
            first = max(n - dups, lo)
            x[first - lo:] = shadow[7] if lo > 7 else x[7]
        nat.slab_append_f32(x.contiguous(), slab, lo, nat.SLAB_F16, shadow=shadow, row_err=row_err)
    st = (slab, shadow, float(row_err.item()))
    _STORES[key] = st
    return st


def _queries(cuda, shadow, nq, seed):
    import torch
    g = torch.Generator(device=cuda)
    g.manual_seed(seed)
    n, d = shadow.shape
    q = torch.randn((nq, d), generator=g, device=cuda)
    j = torch.randint(0, n, (nq,), generator=g, device=cuda)
    q[0::2] = shadow[j[0::2]] + 0.1 * q[0::2]
    return torch.nn.functional.normalize(q, dim=1).contiguous()


def _run(cuda, q32, slab, shadow, row_err, n, d, kc, k, id_base=0, cap=1024, escalate=False):
    """one crs_cosine_topk_cert call with every output buffer pre-filled with garbage; returns every output on the host"""
    import torch
    from rag import _native as nat
    nq = q32.shape[0]
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    ws = torch.full((nat.scan_workspace_bytes(nq, d, kc, n),), 0xA5, dtype=torch.uint8, device=cuda)
    ews = torch.full((nat.exact_workspace_bytes(nq, cap),), 0x5A, dtype=torch.uint8, device=cuda)
    cs = torch.full((nq, kc), 7.5, dtype=torch.float32, device=cuda)
    ci = torch.full((nq, kc), 123456789, dtype=torch.int64, device=cuda)
    os_ = torch.full((nq, k), float("nan"), dtype=torch.float32, device=cuda)
    oi = torch.full((nq, k), -987, dtype=torch.int64, device=cuda)
    stt = torch.full((nq,), 77, dtype=torch.int32, device=cuda)
    nat.cosine_topk_cert(q32, q16, slab, shadow, n, d, kc, k, row_err, ews, cap, id_base=id_base, workspace=ws, cand_scores=cs,
                         cand_ids=ci, out_scores=os_, out_ids=oi, status=stt)
    thr = ews[:nq * 4].view(torch.float32).clone()
    st0 = stt.clone()
    if escalate:
        nat.escalate_exact(q32, q16, slab, shadow, n, id_base, k, os_, oi, stt, ews, cap)
    torch.cuda.synchronize()
    out = {"cand_s": cs, "cand_i": ci, "s": os_, "i": oi, "status": st0, "status_after": stt, "ws_thr": thr}
    return {name: t.cpu().numpy() for name, t in out.items()}


def _same(a, b, what):
    for name in a:
        x, y = a[name], b[name]
        if x.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        assert np.array_equal(x, y), f"{what}: {name} differs between the fused tail and the chain"


def _both(cuda, q32, slab, shadow, row_err, n, d, kc, k, **kw):
    with _Env(CRS_FUSED_TAIL=1):
        fused = _run(cuda, q32, slab, shadow, row_err, n, d, kc, k, **kw)
    with _Env(CRS_FUSED_TAIL=0):
        chain = _run(cuda, q32, slab, shadow, row_err, n, d, kc, k, **kw)
    return fused, chain


CASES = [
    # n, d, nq, k', k, the plan takes the fused tail (None: not asserted)
    (100_000, 384, 64, 16, 10, True),
    (100_000, 384, 1, 24, 10, None),
    (1_000_000, 384, 64, 24, 10, True),
    (1_000_000, 384, 16, 32, 20, None),
    (1_000_000, 384, 200, 16, 10, None),
    (2_000_000, 384, 64, 24, 10, True),
    (2_000_000, 384, 64, 48, 20, None),
    (1_000_003, 384, 64, 24, 10, True),   # ragged last tile
    (300_001, 256, 64, 32, 20, None),     # ragged, 256-element rows
    (400_000, 640, 64, 24, 10, None),
    (250_000, 768, 64, 24, 10, False),    # 768: the chain inside the entry (finish_fits), still one call
]


@pytest.mark.parametrize("n,d,nq,kc,k,fused_plan", CASES)
def test_fused_tail_is_the_chain(cuda, n, d, nq, kc, k, fused_plan):
    from rag import _native as nat
    slab, shadow, row_err = _store(cuda, n, d)
    q32 = _queries(cuda, shadow, nq, seed=n % 97 + nq)
    plan = nat.scan_plan_describe(nq, d, kc, n)
    if fused_plan is not None:
        assert ("cert tail: fused" in plan) == fused_plan, plan
    fused, chain = _both(cuda, q32, slab, shadow, row_err, n, d, kc, k)
    _same(fused, chain, plan)
    assert (fused["status"] >= 0).all() and (fused["status"] <= 1).all()
    assert (fused["i"][:, 0] >= 0).all()


def test_fused_tail_id_base_and_ties(cuda):
    """a shard at id_base != 0 whose last 3000 rows repeat one row: exact ties at the k-th score, an unproven query escalated"""
    import torch
    n, d, nq = 600_000, 384, 64
    slab, shadow, row_err = _store(cuda, n, d, dups=3000)
    q32 = _queries(cuda, shadow, nq, seed=5)
    q32[1] = torch.nn.functional.normalize(shadow[7] + 1e-3 * q32[1], dim=0)   # thousands of identical best rows
    q32[3] = shadow[7]
    fused, chain = _both(cuda, q32.contiguous(), slab, shadow, row_err, n, d, 24, 10, id_base=1_000_000_007, cap=4096, escalate=True)
    _same(fused, chain, "ties / id_base")
    assert fused["status"][1] == 1 and fused["status"][3] == 1       # the band is deeper than the over-fetch
    assert fused["i"].min() >= 1_000_000_007
    assert fused["status_after"][1] != 2 and fused["status_after"][3] != 2   # the escalation's lists fit the cap
    for q in (1, 3):                                                 # after the escalation: exact ties in row order
        assert (fused["s"][q] == fused["s"][q][0]).all()
        assert np.all(np.diff(fused["i"][q]) > 0)


def test_fused_tail_graph_replay(cuda):
    """cosine_topk_cert + escalate_exact captured in a hipGraph and replayed give the eager results"""
    import torch
    from rag import _native as nat
    n, d, nq, kc, k, cap = 1_000_000, 384, 64, 24, 10, 1024
    slab, shadow, row_err = _store(cuda, n, d)
    q32 = _queries(cuda, shadow, nq, seed=11)
    eager = _run(cuda, q32, slab, shadow, row_err, n, d, kc, k, escalate=True)
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    ws = torch.empty(nat.scan_workspace_bytes(nq, d, kc, n), dtype=torch.uint8, device=cuda)
    ews = torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=cuda)
    cs = torch.empty((nq, kc), dtype=torch.float32, device=cuda)
    ci = torch.empty((nq, kc), dtype=torch.int64, device=cuda)
    os_ = torch.empty((nq, k), dtype=torch.float32, device=cuda)
    oi = torch.empty((nq, k), dtype=torch.int64, device=cuda)
    stt = torch.empty((nq,), dtype=torch.int32, device=cuda)

    def step():
        nat.cosine_topk_cert(q32, q16, slab, shadow, n, d, kc, k, row_err, ews, cap, workspace=ws, cand_scores=cs, cand_ids=ci,
                             out_scores=os_, out_ids=oi, status=stt)
        nat.escalate_exact(q32, q16, slab, shadow, n, 0, k, os_, oi, stt, ews, cap)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in (cs, os_):
        t.fill_(float("nan"))
    oi.fill_(-5)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for name, t in (("cand_s", cs), ("cand_i", ci), ("s", os_), ("i", oi), ("status_after", stt)):
        x, y = t.cpu().numpy(), eager[name]
        if x.dtype == np.float32:
            x, y = x.view(np.int32), y.view(np.int32)
        assert np.array_equal(x, y), f"graph replay: {name}"


@pytest.mark.parametrize("n,d,nq,k", [(2_000_000, 384, 64, 24), (2_000_000, 384, 64, 10), (100_000, 384, 64, 16)])
def test_nt_slab_stream_gives_the_same_lists(cuda, n, d, nq, k):
    from rag import _native as nat
    slab, shadow, _ = _store(cuda, n, d)
    q32 = _queries(cuda, shadow, nq, seed=3)
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    if n * nat.padded_dim(d) * 2 >= 1 << 30:
        assert " nt " in nat.scan_plan_describe(nq, d, k, n)        # the plan's own choice on a > 1 GB slab
    out = {}
    for v in (1, 0):
        with _Env(CRS_SCAN_NT=v):
            assert (" nt " in nat.scan_plan_describe(nq, d, k, n)) == (v == 1)
            s, i = nat.cosine_topk(q16, slab, n, d, k)
            out[v] = (s.cpu().numpy().view(np.int32), i.cpu().numpy())
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
