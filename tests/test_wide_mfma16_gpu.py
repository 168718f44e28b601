"""GPU: the 16x16x32 compute form of csrc/scan_wide.hip's split-list kernels (scan_wide16_kernel<384, 8, 24 | 32>), forced with
CRS_WIDE_MFMA=16, against the 32x32x16 form (CRS_WIDE_MFMA=32), against the same queries as 64-query calls, and against torch
fp64 on the fp16 slab values.

Every case scans 384-element seeded unit rows (built through slab_append_f32) with 256 workgroups x 64-row tiles:
``cosine_topk_cert`` at k' = 24 / 32, k = 10, then ``escalate_exact``.  The partial lists are read out of the caller's scan
workspace (capi.hip, "scan workspace": the ticket / threshold words, then [nq, streams, kp] scores, then [nq, streams, kp] rows,
each block 256-byte aligned).

Sizes: 64 x 256 x 2 + 1 rows (two tiles per workgroup and a one-row ragged tile; one deferred tile), 64 x 256 x 3 (three tiles),
64 x 256 x 26 + 37 (26 - 27 tiles per workgroup: a 24-slot list overflows; ragged).  The tie corpus needs 30 tiles in one
workgroup: 64 x 256 x 30 rows.  Query counts: 256; 210 (wave 6 holds a full group of 16 and a group of 2); 193 (wave 6 holds one
query, its second group is empty, wave 7 is idle); 130.

Tolerances of the list check: a tile best is a sum of 384 products whose absolute sum is <= 1 (unit rows), accumulated in fp32:
at most 384 roundings of 2^-24 each = 2.3e-5, asked as 3e-5; a tile outside a list may therefore beat the list's minimum in the
reference by twice that, 6e-5."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, NWG, TILE, K_OUT = 384, 256, 64, 10
N_TWO, N_THREE, N_LONG = TILE * NWG * 2 + 1, TILE * NWG * 3, TILE * NWG * 26 + 37
N_TIES = TILE * NWG * 30
SIZES = [N_TWO, N_THREE, N_LONG]
NQS = [256, 210, 193, 130]
C_WG = 17                        # the workgroup (static stride: tile stream) that sees every copy of the tie corpus
Q_TIES = (9, 25, 133, 150)       # wave 0 group 0, wave 0 group 1, wave 4 group 0, wave 4 group 1


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


_WORLDS = {}


def _copy_rows():
    return [C_WG * TILE + 3 + i * NWG * TILE for i in range(30)]


def _world(cuda, n):
    """slab + shadow of n seeded unit rows (the tie corpus: 30 exact copies of one row planted), 256 unit queries, and the fp64
    tile bests of the fp16 slab values [256, tiles]; one store at a time on the device, built once per size and never changed"""
    import torch
    from rag import _native as nat
    if n in _WORLDS:
        return _WORLDS[n]
    _WORLDS.clear()
    torch.cuda.empty_cache()
    g = torch.Generator(device=cuda)
    g.manual_seed(n)
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    if n == N_TIES:
        copies = _copy_rows()
        rows[copies] = rows[copies[0]].clone()
    slab = torch.zeros((n, nat.padded_dim(D)), dtype=torch.float16, device=cuda)
    shadow = torch.empty((n, D), dtype=torch.float32, device=cuda)
    row_err = torch.zeros(1, dtype=torch.float32, device=cuda)
    for lo in range(0, n, 250_000):
        nat.slab_append_f32(rows[lo:lo + 250_000].contiguous(), slab, lo, nat.SLAB_F16, shadow=shadow, row_err=row_err)
    del rows
    q = torch.randn((256, D), generator=g, device=cuda)
    j = torch.randint(0, n, (256,), generator=g, device=cuda)
    q[0::2] = shadow[j[0::2]] + 0.1 * q[0::2]                   # every second query near a row
    if n == N_TIES:
        for qi in Q_TIES:
            q[qi] = shadow[_copy_rows()[0]]                      # on the copied row
    q32 = torch.nn.functional.normalize(q, dim=1).contiguous()
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    # the reference: fp64 products of the fp16 values the scan reads, best of every 64-row tile
    n_tiles = (n + TILE - 1) // TILE
    ref = torch.full((256, n_tiles * TILE), float("-inf"), dtype=torch.float64, device=cuda)
    q64 = q16[:, :D].double()
    for lo in range(0, n, 65536):
        hi = min(n, lo + 65536)
        ref[:, lo:hi] = q64 @ slab[lo:hi, :D].double().T
    ref_tiles = ref.view(256, n_tiles, TILE).max(dim=2).values.cpu().numpy()
    del ref
    _WORLDS[n] = dict(n=n, slab=slab, shadow=shadow, row_err=float(row_err.item()), q32=q32, ref_tiles=ref_tiles)
    return _WORLDS[n]


def _buffers(cuda, nq, kc, n, cap):
    import torch
    from rag import _native as nat
    return dict(ews=torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=cuda),
                cs=torch.full((nq, kc), 7.5, dtype=torch.float32, device=cuda),
                ci=torch.full((nq, kc), -5, dtype=torch.int64, device=cuda),
                ws=torch.full((nat.scan_workspace_bytes(nq, D, kc, n),), 0x5a, dtype=torch.uint8, device=cuda))


def _parts(ws, nq, kc):
    kp = 2 * (24 if kc <= 24 else 32)
    al = lambda b: (b + 255) // 256 * 256
    o_s = al(nq * 4)
    o_r = o_s + al(NWG * nq * kp * 4)
    raw = ws.cpu().numpy()
    return (raw[o_s:o_s + NWG * nq * kp * 4].view(np.float32).reshape(nq, NWG, kp).copy(),
            raw[o_r:o_r + NWG * nq * kp * 4].view(np.int32).reshape(nq, NWG, kp).copy())


def _cert(cuda, w, q32, kc, want_parts=False, cap=1024):
    """one cosine_topk_cert + escalate_exact; outputs on the host, with the partial lists [nq, streams, kp] where asked"""
    import torch
    from rag import _native as nat
    n, nq = w["n"], q32.shape[0]
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    b = _buffers(cuda, nq, kc, n, cap)
    s, i, st = nat.cosine_topk_cert(q32, q16, w["slab"], w["shadow"], n, D, kc, K_OUT, w["row_err"], b["ews"], cap, workspace=b["ws"],
                                    cand_scores=b["cs"], cand_ids=b["ci"])
    st0 = st.clone()
    nat.escalate_exact(q32, q16, w["slab"], w["shadow"], n, 0, K_OUT, s, i, st, b["ews"], cap)
    torch.cuda.synchronize()
    out = {name: t.cpu().numpy() for name, t in {"s": s, "i": i, "cand_s": b["cs"], "cand_i": b["ci"], "st0": st0, "st1": st}.items()}
    if want_parts:
        out["part_s"], out["part_r"] = _parts(b["ws"], nq, kc)
    return out


def _plan_is_split(n, nq, kc):
    from rag import _native as nat
    plan = nat.scan_plan_describe(nq, D, kc, n)
    K = 24 if kc <= 24 else 32
    assert f"scan_wide_kernel<384,8,{K}>" in plan and f"streams={NWG} " in plan and "qblocks=1" in plan and f"kp={2 * K}" in plan, plan
    return K


def _bits(x):
    return x.view(np.int32) if x.dtype == np.float32 else x


# ---------------------------------------------------------------- 1. the two shapes agree
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", SIZES)
def test_shapes_agree(cuda, n, nq):
    w = _world(cuda, n)
    q32 = w["q32"][:nq].contiguous()
    knobs = (("static", dict(CRS_WIDE_DYN=0)), ("tickets", dict(CRS_TB_DYN_MIN=8)), ("static, no stagger", dict(CRS_WIDE_DYN=0, CRS_WIDE_STAGGER=0)))
    for kc in (24, 32):
        _plan_is_split(n, nq, kc)
        parts = [_cert(cuda, w, q32[lo:lo + 64].contiguous(), kc) for lo in range(0, nq, 64)]
        narrow = {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}
        assert not (narrow["st1"] == 2).any()
        for what, env in knobs:
            got = {}
            for shape in (16, 32):
                with _Env(CRS_WIDE_MFMA=shape, **env):
                    got[shape] = _cert(cuda, w, q32, kc)
            a, b = got[16], got[32]
            tag = f"n={n} nq={nq} k'={kc} {what}"
            print(f"{tag}: status-1 {int((a['st0'] == 1).sum())} / {int((b['st0'] == 1).sum())} / 64-query calls {int((narrow['st0'] == 1).sum())}")
            for name in ("s", "i", "st0", "st1"):                     # finals and both status words: bit-identical
                assert np.array_equal(_bits(a[name]), _bits(b[name])), (tag, name)
            assert not (a["st1"] == 2).any(), tag
            assert np.array_equal(np.sort(a["cand_i"], axis=1), np.sort(b["cand_i"], axis=1)), tag
            for shape in (16, 32):                                    # ... and equal to the 64-query calls
                for name in ("s", "i", "st0", "st1"):
                    assert np.array_equal(_bits(got[shape][name]), _bits(narrow[name])), (tag, shape, name)
                assert np.array_equal(np.sort(got[shape]["cand_i"], axis=1), np.sort(narrow["cand_i"], axis=1)), (tag, shape)


# ---------------------------------------------------------------- 2. the lists are right
def _check_lists(w, part_s, part_r, K, nq, tag):
    n = w["n"]
    n_tiles = (n + TILE - 1) // TILE
    J = (n_tiles + NWG - 1) // NWG
    ref = np.full((nq, J * NWG), -np.inf)
    ref[:, :n_tiles] = w["ref_tiles"][:nq]
    ref = ref.reshape(nq, J, NWG).transpose(0, 2, 1)                  # [q, workgroup, j]: tile j * 256 + workgroup
    assert np.isneginf(part_s[:, :, K:]).all() and (part_r[:, :, K:] == -1).all(), f"{tag}: the K trailing slots"
    s, r = part_s[:, :, :K].astype(np.float64), part_r[:, :, :K]
    empty = r == -1
    assert np.array_equal(empty, np.isneginf(s)), f"{tag}: empty slots"
    per_wg = np.array([len(range(b, n_tiles, NWG)) for b in range(NWG)])
    assert np.array_equal((~empty).sum(axis=2), np.broadcast_to(np.minimum(per_wg, K)[None, :], empty.shape[:2])), f"{tag}: entries per list"
    assert (empty[:, :, 1:] >= empty[:, :, :-1]).all(), f"{tag}: an entry behind an empty slot"
    assert ((r[~empty] >= 0) & (r[~empty] < n) & (r[~empty] % TILE == 0)).all(), f"{tag}: rows"
    tile = np.where(empty, 0, r // TILE)
    assert (empty | (tile % NWG == np.arange(NWG)[None, :, None])).all(), f"{tag}: a tile of another workgroup's stream"
    j = tile // NWG
    stand_in = np.where(empty, -1 - np.arange(K)[None, None, :], j)    # distinct stand-ins for the empty slots
    assert (np.diff(np.sort(stand_in, axis=2), axis=2) != 0).all(), f"{tag}: a tile twice"
    assert (s[:, :, 1:] <= s[:, :, :-1]).all(), f"{tag}: order"
    tie = (s[:, :, 1:] == s[:, :, :-1]) & ~empty[:, :, 1:]
    assert (~tie | (r[:, :, 1:] > r[:, :, :-1])).all(), f"{tag}: equal scores, later tile first"
    want = np.take_along_axis(ref, j, axis=2)
    err = np.abs(np.where(empty, 0.0, s - want))
    print(f"{tag}: max |score - fp64 tile best| {err.max():.3e}")
    assert err.max() <= 3e-5, f"{tag}: score off by {err.max()}"
    outside = ref.copy()
    np.put_along_axis(outside, np.where(empty, j[:, :, :1], j), -np.inf, axis=2)      # (an empty slot points at a listed tile)
    best_out = outside.max(axis=2)
    lo = np.where(empty.any(axis=2), -np.inf, s.min(axis=2))
    full = ~empty.any(axis=2)
    assert np.isneginf(best_out[~full]).all(), f"{tag}: a tile missing from a list with room"
    gap = best_out[full] - lo[full]
    print(f"{tag}: best tile outside a full list - list minimum {gap.max() if gap.size else float('nan'):.3e}")
    assert (gap <= 6e-5).all(), f"{tag}: a better tile was left out"


@pytest.mark.parametrize("kc", [24, 32])
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", SIZES)
def test_lists_are_right(cuda, n, nq, kc):
    w = _world(cuda, n)
    K = _plan_is_split(n, nq, kc)
    with _Env(CRS_WIDE_MFMA=16, CRS_WIDE_DYN=0):
        got = _cert(cuda, w, w["q32"][:nq].contiguous(), kc, want_parts=True)
    _check_lists(w, got["part_s"], got["part_r"], K, nq, f"n={n} nq={nq} k'={kc}")


# ---------------------------------------------------------------- 3. ties
def test_ties_keep_the_lower_rows_in_row_order(cuda):
    w = _world(cuda, N_TIES)
    K = _plan_is_split(N_TIES, 256, 24)
    copies = _copy_rows()
    with _Env(CRS_WIDE_MFMA=16, CRS_WIDE_DYN=0):
        got = _cert(cuda, w, w["q32"], 24, want_parts=True)
    _check_lists(w, got["part_s"], got["part_r"], K, 256, "ties")
    for qi in Q_TIES:     # the 24 lowest copies, in row order, bit-equal scores, across the 11 / 12 and the 23 / 24 boundary
        assert got["part_r"][qi, C_WG, :K].tolist() == [r - 3 for r in copies[:K]], (qi, got["part_r"][qi, C_WG, :K].tolist())
        assert len(set(got["part_s"][qi, C_WG, :K].view(np.int32).tolist())) == 1, qi
        assert got["i"][qi].tolist() == copies[:K_OUT], (qi, got["i"][qi].tolist())
        assert sorted(got["cand_i"][qi].tolist()) == copies[:24], qi


# ---------------------------------------------------------------- 4. a representative is its row's re-score
def _best_and_top(cuda, w, nq, shape):
    """per query: the best rank-0 representative over all workgroups under CRS_WIDE_MFMA=shape (None: the library's own choice),
    the partial-list scores, and the top score of cosine_topk in 64-query calls (tile_rescore_f16's arithmetic)"""
    import torch
    from rag import _native as nat
    n = w["n"]
    q32 = w["q32"][:nq].contiguous()
    env = dict(CRS_WIDE_DYN=0) if shape is None else dict(CRS_WIDE_DYN=0, CRS_WIDE_MFMA=shape)
    with _Env(**env):
        got = _cert(cuda, w, q32, 24, want_parts=True)
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    top = []
    for lo in range(0, nq, 64):
        s, _ = nat.cosine_topk(q16[lo:lo + 64].contiguous(), w["slab"], n, D, K_OUT)
        top.append(s[:, 0].clone())
    torch.cuda.synchronize()
    return got["part_s"][:, :, 0].max(axis=1), got["part_s"], torch.cat(top).cpu().numpy()


@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", SIZES)
def test_best_representative_is_the_re_scored_top_score(cuda, n, nq):
    w = _world(cuda, n)
    _plan_is_split(n, nq, 24)
    best, _, top = _best_and_top(cuda, w, nq, 16)
    differ = best.view(np.int32) != top.view(np.int32)
    print(f"n={n} nq={nq}: {int(differ.sum())} of {nq} best representatives differ from the re-scored top score; max |diff| {np.abs(best - top).max():.3e}")
    assert not differ.any()


def _kernels_launched(cuda, w, shape):
    """names of the device kernels one cosine_topk_cert of 256 queries launches under CRS_WIDE_MFMA=shape (None: no knob)"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    env = dict(CRS_WIDE_DYN=0) if shape is None else dict(CRS_WIDE_DYN=0, CRS_WIDE_MFMA=shape)
    with _Env(**env):
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _cert(cuda, w, w["q32"], 24)
            torch.cuda.synchronize()
    return sorted({e.name for e in prof.events() if "scan_wide" in e.name})


def test_the_knob_picks_the_kernel(cuda):
    """CRS_WIDE_MFMA is honoured, so the comparisons of the two shapes above compare two kernels.  The outputs cannot show it: on
    these corpora the two shapes' list scores are bit-identical (measured: 0 of 3 145 728 differ at 426 021 rows x 256 queries, and
    under =32 every best representative equals its row's re-score too), so the kernel names of the launches are read from the
    profiler's trace.  Without the knob a 384-element launch runs the 16x16x32 kernel."""
    w = _world(cuda, N_LONG)
    _plan_is_split(N_LONG, 256, 24)
    seen = {shape: _kernels_launched(cuda, w, shape) for shape in (16, 32, None)}
    print(seen)
    for shape, want, other in ((16, "scan_wide16_kernel<384, 8, 24>", "scan_wide_kernel<"), (32, "scan_wide_kernel<384, 8, 24>", "scan_wide16_kernel<"),
                               (None, "scan_wide16_kernel<384, 8, 24>", "scan_wide_kernel<")):
        assert any(want in k for k in seen[shape]), (shape, seen[shape])
        assert not any(other in k for k in seen[shape]), (shape, seen[shape])
    best16, part16, top = _best_and_top(cuda, w, 256, 16)
    _, part_default, _ = _best_and_top(cuda, w, 256, None)
    assert np.array_equal(part_default.view(np.int32), part16.view(np.int32))


# ---------------------------------------------------------------- 5. hipGraph replay
def test_graph_replay_is_the_eager_call(cuda):
    import torch
    from rag import _native as nat
    n, nq, kc, cap = N_THREE, 256, 24, 1024
    w = _world(cuda, n)
    _plan_is_split(n, nq, kc)
    q32 = w["q32"]
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    with _Env(CRS_WIDE_MFMA=16):
        eager = _cert(cuda, w, q32, kc, want_parts=True)
        b = _buffers(cuda, nq, kc, n, cap)
        os_ = torch.empty((nq, K_OUT), dtype=torch.float32, device=cuda)
        oi = torch.empty((nq, K_OUT), dtype=torch.int64, device=cuda)
        stt = torch.empty((nq,), dtype=torch.int32, device=cuda)

        def step():
            nat.cosine_topk_cert(q32, q16, w["slab"], w["shadow"], n, D, kc, K_OUT, w["row_err"], b["ews"], cap, workspace=b["ws"],
                                 cand_scores=b["cs"], cand_ids=b["ci"], out_scores=os_, out_ids=oi, status=stt)
            nat.escalate_exact(q32, q16, w["slab"], w["shadow"], n, 0, K_OUT, os_, oi, stt, b["ews"], cap)

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            step()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):      # the shape is chosen when the launch is recorded
            step()
    for t in (b["cs"], os_):
        t.fill_(float("nan"))
    oi.fill_(-5)
    b["ws"].fill_(0x5a)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    part_s, part_r = _parts(b["ws"], nq, kc)
    for name, t in (("cand_s", b["cs"]), ("cand_i", b["ci"]), ("s", os_), ("i", oi), ("st1", stt), ("part_s", part_s), ("part_r", part_r)):
        x = t if isinstance(t, np.ndarray) else t.cpu().numpy()
        assert np.array_equal(_bits(x), _bits(eager[name])), f"graph replay: {name}"
