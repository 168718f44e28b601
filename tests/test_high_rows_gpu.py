"""GPU: every row-indexed kernel at rows past the 2^31 / 2^32 byte and element offsets of its arrays (tests/_high_rows.py).

One store of N = 2^22 + 1061 rows x 1024 dimensions is built on the device with plain torch: fp32 shadow 17.2 GB, fp16 slab 8.6 GB,
int8 slab 4.3 GB.  Planted rows sit on both sides of every line (r - 1, r, r + 1), every background row scores at most 0.2 against
the queries by Cauchy-Schwarz, and tests/test_high_rows_cpu.py shows that the row a wrapped offset reaches never carries a planted
row's score.  A kernel that drops a 64-bit cast therefore returns another list (readers) or changes a snapshot row (writers).

Readers compute their expectation in fp64 from host copies of the rows involved; id lists are compared with array_equal wherever
the fp64 gaps make the order unique (asserted first), and by the near-tie rule of tests/topk_check.py where a list runs deep into
the background (top_k 100 / 1024: neighbouring background scores are closer than fp32 resolves).  Score tolerances are those of
the small-shape tests of the same entry points.  Writers compare bit for bit with the same vectors stored by the same entry point
into a 64-row store, and check that neighbouring and alias rows keep their bits.

The module skips only on a device of less than 64 GB (not an MI355X)."""
import os
import time

import numpy as np
import pytest

import _high_rows as hr
import _join_ref as jr
import _mmr_ref as mr
import _space_build_ref as br
import _space_ref as sr
from topk_check import TIGHT_TOL

pytestmark = pytest.mark.gpu

F16, I8 = 0, 1
N, DIM = hr.N, hr.DIM
SCORE_TOL32 = 1e-5              # fp32 re-rank against fp64: tests/test_refine_gpu.py, tests/test_exact_gpu.py, tests/topk_check.py::assert_topk
NEAR_TIE = 3e-7                 # tests/test_large_k_gpu.py TOL: fp64 gap below which two rows may change places in an fp32 ranking
U = 2.0 ** -24
ID_BASE = 2 ** 40 + 5           # the refiners' view: ids are rows + ID_BASE
PEAK_LIMIT = 40e9


@pytest.fixture(scope="module")
def store(cuda):
    import torch
    from rag import _native as nat
    total = torch.cuda.get_device_properties(cuda).total_memory
    if total < 64e9:
        pytest.skip(f"device memory {total / 1e9:.0f} GB: not an MI355X")
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.time()
    st = hr.Store(cuda, nat.padded_dim(DIM, F16), nat.padded_dim(DIM, I8))
    st.geometry = hr.arrays(nat.padded_dim(DIM, F16), nat.padded_dim(DIM, I8))
    st.base_bytes = base
    st.cache = {}
    print(f"high-row store built in {time.time() - t0:.1f} s")
    yield st
    torch.cuda.synchronize()
    print(f"high-row module: peak device memory {(torch.cuda.max_memory_allocated() - base) / 1e9:.2f} GB above the {base / 1e9:.2f} GB held before, "
          f"{time.time() - t0:.1f} s from the fixture's start")
    st.free()
    del st
    torch.cuda.empty_cache()


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


# ------------------------------------------------------------------------------------------------------------------ helpers
def _idx(rows, dev):
    import torch
    return torch.as_tensor(np.asarray(rows, dtype=np.int64), device=dev)


def _host(t, rows):
    """rows of a device array as numpy: tensor[index].cpu(), never the array."""
    return t[_idx(rows, t.device)].cpu().numpy()


def _bits(t):
    import torch
    return t.view({torch.float32: torch.int32, torch.float16: torch.int16}.get(t.dtype, t.dtype))


def _same_bits(a, b):
    import torch
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(_bits(a), _bits(b)))


def _queries(cuda, nq, st):
    """(q32 host, q32 device, q16 device, q16 host) of the first nq queries."""
    import torch
    from rag import _native as nat
    q = hr.queries(nq)
    qd = torch.from_numpy(q).to(cuda)
    q16 = nat.queries_to_f16(qd, st)
    return q, qd, q16, q16.cpu().numpy()


def _planted_host(store):
    return _host(store.shadow, hr.PLANTED_ROWS)


def _slab_scores64(q16_h, slab_rows_h, scales_h, st):
    """fp64 scores of host copies of slab rows, as the scan of that slab type defines them."""
    from oracle import scan_ref
    if st == I8:
        return (scan_ref.dequantized_queries(q16_h) @ slab_rows_h.astype(np.float64).T) * scales_h.astype(np.float64)[None, :]
    return q16_h.astype(np.float64) @ slab_rows_h.astype(np.float64).T


def _near_tie_errors(got_i, ref_i, s_got, s_ref, k, tol):
    """The id rule of tests/topk_check.py::topk_errors on fp64 scores the caller gathered: {query: reason}."""
    errs = {}
    for r in range(got_i.shape[0]):
        if (got_i[r] < 0).any() or len(set(got_i[r].tolist())) != k:
            errs[r] = f"got rows {got_i[r].tolist()[:20]}"
            continue
        kth = s_ref[r, k - 1]
        for a, b, sa, sb in zip(got_i[r], ref_i[r], s_got[r], s_ref[r]):
            if a != b and not abs(sa - sb) < tol:
                errs[r] = f"got row {a} ({sa!r}), reference row {b} ({sb!r})"
                break
        else:
            if not (s_got[r] >= kth - tol).all():
                errs[r] = "holds a row below the k-th best"
    return errs


class _Snap:
    """Device clones of rows of all four arrays of the store, taken before a write."""
    NAMES = ("shadow", "slab", "slab8", "scales")

    def __init__(self, store, rows):
        self.rows = sorted({int(r) for r in rows if 0 <= int(r) < N})
        self.idx = _idx(self.rows, store.device)
        self.data = {n: getattr(store, n)[self.idx].clone() for n in self.NAMES}
        self.pos = {r: i for i, r in enumerate(self.rows)}

    def of(self, name, rows):
        return self.data[name][_idx([self.pos[int(r)] for r in rows], self.idx.device)]

    def assert_unchanged(self, store, rows, what):
        rows = [int(r) for r in rows if int(r) in self.pos]
        idx = _idx(rows, store.device)
        for n in self.NAMES:
            assert _same_bits(getattr(store, n)[idx], self.of(n, rows)), f"{what}: {n} changed at a row that was not written"

    def restore(self, store):
        for n in self.NAMES:
            getattr(store, n)[self.idx] = self.data[n]


def _around(rows, reach=2):
    return sorted({r + o for r in rows for o in range(-reach, reach + 1) if 0 <= r + o < N})


# ================================================================================================================== readers
@pytest.mark.parametrize("slab", ["f16", "i8"])
def test_scan_returns_the_planted_rows_in_fp64_order(store, cuda, slab):
    """crs_cosine_topk over the whole slab, nq 1 / 16 / 64 / 256, k 10 / 15, then on the view slab[2^21 + 17:] with id_base.
    Kernel families reached at N x 1024 (crs_scan_plan_describe over nq 1 .. 1024, k 10 .. 24): fp16 scan_tb_kernel<1024,16,4,kp>
    (TileBest, 4 waves, nq <= 64; nt stream), scan_tb_kernel<1024,16,8,kp> (TileBest, 8 waves, several query blocks, nq > 64);
    int8 scan_i8_kernel<1024,32,16,kp> with one and with several query blocks.  No query count reaches another family at this
    row length (the Wide, W1 and Classic forms do not take 1024-element rows of a shard this long), so 1 / 16 / 64 / 256 cover them."""
    import torch
    from rag import _native as nat
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    planted_h = _planted_host(store)
    stored_h = _host(sl, hr.PLANTED_ROWS)
    scales_h = _host(sc, hr.PLANTED_ROWS) if sc is not None else None
    col = {r: c for c, r in enumerate(hr.PLANTED_ROWS)}
    kernel = "scan_i8_kernel<1024" if st == I8 else "scan_tb_kernel<1024"
    for nq in (1, 16, 64, 256):
        q, qd, q16, q16_h = _queries(cuda, nq, st)
        want = hr.planted_order(q, planted_h)
        full = _slab_scores64(q16_h, stored_h, scales_h, st)
        for k in (10, 15):
            assert kernel in nat.scan_plan_describe(nq, DIM, k, N, st)
            s, i = nat.cosine_topk(q16, sl, N, DIM, k, slab_type=st, scales=sc)
            torch.cuda.synchronize()
            s, i = s.cpu().numpy(), i.cpu().numpy()
            assert np.array_equal(i, want[:, :k]), (slab, nq, k, i[0].tolist(), want[0, :k].tolist())
            exp = np.stack([full[j, [col[int(r)] for r in i[j]]] for j in range(nq)])
            print(f"{slab} nq {nq} k {k}: max |score - fp64| = {np.abs(s - exp).max():.3e}")
            assert np.abs(s - exp).max() <= TIGHT_TOL, (slab, nq, k)
    # the view: rows below VIEW_FIRST are not in it; the five planted rows above come first, then background rows of the view
    h = hr.VIEW_FIRST
    inside = [r for r in hr.PLANTED_ROWS if r >= h]
    assert len(inside) == 5
    for nq in (16, 256):
        q, qd, q16, q16_h = _queries(cuda, nq, st)
        want = hr.planted_order(q, planted_h[[col[r] for r in inside]], rows=inside)
        for k in (10, 15):
            s, i = nat.cosine_topk(q16, sl[h:], N - h, DIM, k, slab_type=st, scales=None if sc is None else sc[h:], id_base=h)
            torch.cuda.synchronize()
            s, i = s.cpu().numpy(), i.cpu().numpy()
            assert np.array_equal(i[:, :5], want), (slab, nq, k, i[0].tolist())
            rest = i[:, 5:]
            assert ((rest >= h) & (rest < N)).all() and not np.isin(rest, hr.PLANTED_ROWS).any()
            # (slab scores: an int8 row is off by at most scale / 2 = 0.2 / 254 per coordinate, |q|_1 <= 8 on 64 coordinates: 6.3e-3)
            assert (s[:, 5:] <= hr.BACKGROUND_MAX + 1e-2).all() and (s[:, :5] >= hr.MIN_PLANTED - 1e-2).all()


def _check_cert(what, s, i, status, want_ids, q, rows_h, col, scale=1):
    """status certified, ids the fp64 order, scores within SCORE_TOL32 of the fp64 dot of the shadow rows."""
    s, i, status = s.cpu().numpy(), i.cpu().numpy(), status.cpu().numpy()
    assert (status == 0).all(), (what, status.tolist())
    assert np.array_equal(i, want_ids), (what, i[0].tolist(), want_ids[0].tolist())
    full = hr.scores64(q, rows_h)
    exp = np.stack([full[j, [col[int(r) // scale] for r in i[j]]] for j in range(i.shape[0])])
    assert np.abs(s - exp).max() < SCORE_TOL32, (what, np.abs(s - exp).max())


@pytest.mark.parametrize("slab", ["f16", "i8"])
def test_certified_search_chain_and_escalation(store, cuda, slab):
    """crs_cosine_topk_cert on the whole store (1024-element rows always take the three-kernel chain, with CRS_FUSED_TAIL on or off)
    and crs_escalate_exact: k' = 24, k_out = 10, row error = the analytic bound.  The escalation is made to run by marking every
    query uncertified after the certificate published its thresholds: it must rebuild the same lists from one more sweep."""
    import torch
    from rag import _native as nat
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    planted_h = _planted_host(store)
    col = {r: c for c, r in enumerate(hr.PLANTED_ROWS)}
    E = nat.exact_row_error_bound(DIM, st)
    k_in, k_out = 24, 10
    for nq in (16, 256) if st == F16 else (16,):
        q, qd, q16, _ = _queries(cuda, nq, st)
        want = hr.planted_order(q, planted_h)[:, :k_out]
        assert "cert tail: chain" in nat.scan_plan_describe(nq, DIM, k_in, N, st)
        for fused in (1, 0):
            ws = torch.empty(nat.exact_workspace_bytes(nq), dtype=torch.uint8, device=cuda)
            with _Env(CRS_FUSED_TAIL=fused):
                s, i, status = nat.cosine_topk_cert(qd, q16, sl, store.shadow, N, DIM, k_in, k_out, E, ws, scales=sc)
            torch.cuda.synchronize()
            _check_cert((slab, nq, fused), s, i, status, want, q, planted_h, col)
        # the escalation, on the workspace of the last call
        status.fill_(1)
        i.fill_(-1)
        s.fill_(float("-inf"))
        nat.escalate_exact(qd, q16, sl, store.shadow, N, 0, k_out, s, i, status, ws, scales=sc)
        torch.cuda.synchronize()
        assert (status.cpu().numpy() == 1).all(), status.tolist()            # escalated, no list overflow
        status.fill_(0)
        _check_cert((slab, nq, "escalated"), s, i, status, want, q, planted_h, col)


def test_certified_search_fused_tail_on_half_rows(store, cuda):
    """The fused tail (csrc/finish.hip) takes rows of at most 640 elements, so it cannot run on 1024-element rows.  The same memory
    viewed as 2 N rows of 512 elements reaches it: the queries live on the first 64 coordinates, so the even half-rows score what
    the whole rows score and the odd ones score 0 -- the expected list is the planted order with doubled row numbers.  In this view
    the fp16 slab crosses 2^32 bytes at half-row 2^22 and 2^32 elements at 2^23; the shadow crosses every line at half the rows."""
    import torch
    from rag import _native as nat
    n2, d2 = 2 * N, DIM // 2
    slab2, shadow2 = store.slab.view(n2, d2), store.shadow.view(n2, d2)
    planted_h = _planted_host(store)[:, :d2]
    col = {r: c for c, r in enumerate(hr.PLANTED_ROWS)}
    E = nat.exact_row_error_bound(d2, F16)
    k_in, k_out = 24, 10
    for nq in (16, 64):
        q = np.ascontiguousarray(hr.queries(nq)[:, :d2])
        qd = torch.from_numpy(q).to(cuda)
        q16 = nat.queries_to_f16(qd, F16)
        want = 2 * hr.planted_order(q, planted_h)[:, :k_out]
        got = {}
        plan = nat.scan_plan_describe(nq, d2, k_in, n2, F16)
        assert "cert tail: fused" in plan, plan                 # the plan fits the fused tail; CRS_FUSED_TAIL=0 forces the chain per call
        for fused in (1, 0):
            ws = torch.empty(nat.exact_workspace_bytes(nq), dtype=torch.uint8, device=cuda)
            with _Env(CRS_FUSED_TAIL=fused):
                s, i, status = nat.cosine_topk_cert(qd, q16, slab2, shadow2, n2, d2, k_in, k_out, E, ws)
            torch.cuda.synchronize()
            _check_cert(("half rows", nq, fused), s, i, status, want, q, planted_h, col, scale=2)
            got[fused] = (s.cpu().numpy(), i.cpu().numpy())
        assert np.array_equal(got[1][0].view(np.int32), got[0][0].view(np.int32)) and np.array_equal(got[1][1], got[0][1])


def _reference_topk(store, qd, kk):
    """Chunked torch fp64 top-kk of the shadow on the device (the one device-side reference): (scores fp64, ids) sorted."""
    import torch
    key = ("ref", kk, qd.shape[0])
    if key not in store.cache:
        q64 = qd.double()
        best_s = torch.empty((qd.shape[0], 0), dtype=torch.float64, device=qd.device)
        best_i = torch.empty((qd.shape[0], 0), dtype=torch.int64, device=qd.device)
        for lo in range(0, N, hr.CHUNK):
            hi = min(N, lo + hr.CHUNK)
            s = q64 @ store.shadow[lo:hi].double().T
            ts, ti = torch.topk(s, min(kk, hi - lo), dim=1)
            best_s, best_i = torch.cat([best_s, ts], dim=1), torch.cat([best_i, ti + lo], dim=1)
            ts, at = torch.topk(best_s, min(kk, best_s.shape[1]), dim=1)
            best_s, best_i = ts, torch.gather(best_i, 1, at)
            del s
        store.cache[key] = (best_s.cpu().numpy(), best_i.cpu().numpy())
    return store.cache[key]


@pytest.mark.parametrize("k_out", [100, 1024])
def test_large_k_certified_search(store, cuda, k_out):
    """crs_cosine_topk_large_cert (+ crs_escalate_exact for what the partitioned over-fetch cannot prove): the first 15 entries are
    the planted order; the whole list against the chunked torch fp64 ranking of the shadow, by the near-tie rule of
    tests/test_large_k_gpu.py (3e-7: at rank 1000 of 4 M background rows neighbouring fp64 scores are ~1e-8 apart)."""
    import torch
    from rag import _native as nat
    nq, cap = 2, 4096
    q, qd, q16, _ = _queries(cuda, nq, F16)
    ref_s, ref_i = _reference_topk(store, qd, 1024)
    E = nat.exact_row_error_bound(DIM, F16)
    ws = torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=cuda)
    s, i, status = nat.cosine_topk_large_cert(qd, q16, store.slab, store.shadow, N, DIM, k_out, E, ws, cap)
    torch.cuda.synchronize()
    st0 = status.cpu().numpy().copy()
    assert set(st0.tolist()) <= {0, 1}
    nat.escalate_exact(qd, q16, store.slab, store.shadow, N, 0, k_out, s, i, status, ws, cap)
    torch.cuda.synchronize()
    assert (status.cpu().numpy() != 2).all(), status.tolist()
    print(f"large k {k_out}: status before the escalation {st0.tolist()}")
    got_i, got_s = i.cpu().numpy(), s.cpu().numpy()
    want = hr.planted_order(q, _planted_host(store))
    assert np.array_equal(got_i[:, :15], want) and np.array_equal(ref_i[:, :15], want)
    got64 = torch.stack([store.shadow[i[j]].double() @ qd[j].double() for j in range(nq)]).cpu().numpy()
    errs = _near_tie_errors(got_i, ref_i[:, :k_out], got64, ref_s[:, :k_out], k_out, NEAR_TIE)
    assert not errs, errs
    assert np.abs(got_s - got64).max() < SCORE_TOL32
    assert (got_s[:, :-1] >= got_s[:, 1:]).all()


# ---- the refiners -----------------------------------------------------------------------------------------------------------------
def _pool_rows():
    """Background rows just around each line (and the end of the store)."""
    near = {x + o for x in hr.LINES for o in range(-20, 21)} | {N - 1 - o for o in range(1, 20)}
    return sorted(r for r in near if 0 <= r < N and r not in hr.PLANTED_ROWS)


def _pick_separated(value, tol, fixed, pool, want, rng):
    """Indices: `fixed` + `want` of `pool` (in random order) such that all chosen values are pairwise further apart than twice the
    sum of their tolerances: the fp64 order of the chosen rows is then the order of any arithmetic inside the tolerance."""
    chosen = list(fixed)
    for a in range(len(chosen)):
        for b in range(a):
            assert abs(value[chosen[a]] - value[chosen[b]]) > 2.0 * (tol[chosen[a]] + tol[chosen[b]]), "planted rows do not separate"
    for c in rng.permutation(pool).tolist():
        if len(chosen) == len(fixed) + want:
            break
        if all(abs(value[c] - value[e]) > 2.0 * (tol[c] + tol[e]) for e in chosen):
            chosen.append(c)
    assert len(chosen) == len(fixed) + want, "the pool does not hold enough separated background rows"
    return chosen


def _candidate_lists(rows, value, tol, seed):
    """Per query a shuffled list of all planted rows, 20 separated background rows from around the lines, four -1 slots and one
    id outside the view.  rows: the store rows of the columns of value / tol [nq, n] (planted first).  Returns (ids int64 [nq, 40],
    the valid columns per query in expected order (value ascending or descending is the caller's business))."""
    rng = np.random.default_rng(seed)
    nq = value.shape[0]
    ids = np.empty((nq, 40), dtype=np.int64)
    cols = []
    for j in range(nq):
        chosen = _pick_separated(value[j], tol[j], list(range(hr.N_PLANTED)), np.arange(hr.N_PLANTED, len(rows)), 20, rng)
        entries = [rows[c] + ID_BASE for c in chosen] + [-1] * 4 + [ID_BASE - 3 - j]
        ids[j] = np.asarray(entries, dtype=np.int64)[rng.permutation(40)]
        cols.append(chosen)
    return ids, cols


def _gathered(store):
    """(rows, fp32 host copies of their shadow rows): the planted rows first, then the pool."""
    if "gathered" not in store.cache:
        rows = list(hr.PLANTED_ROWS) + _pool_rows()
        store.cache["gathered"] = (rows, _host(store.shadow, rows))
    return store.cache["gathered"]


def test_fp32_refiners_on_candidate_lists(store, cuda):
    """crs_refine_f32, crs_score_rows_f32 and crs_rescore_f32 on lists that hold every planted row, background rows from around each
    line, empty slots and a foreign id; ids are rows + 2^40 + 5."""
    import torch
    from rag import _native as nat
    nq = 5
    q = hr.queries(nq)
    qd = torch.from_numpy(q).to(cuda)
    rows, rows_h = _gathered(store)
    prod_abs = np.abs(q.astype(np.float64))[:, None, :] * np.abs(rows_h.astype(np.float64))[None, :, :]
    s64, tol = hr.scores64(q, rows_h), (DIM + 2) * U * prod_abs.sum(axis=2)      # the worst case of an fp32 dot: what separates the lists
    ids, cols = _candidate_lists(rows, s64, tol, seed=4)
    ids_d = torch.from_numpy(ids).to(cuda)
    want_i, want_s = [], []
    for j in range(nq):
        order = sorted(cols[j], key=lambda c: (-s64[j, c], rows[c]))
        want_i.append([rows[c] + ID_BASE for c in order])
        want_s.append([s64[j, c] for c in order])
    want_i, want_s = np.asarray(want_i, dtype=np.int64), np.asarray(want_s)
    # crs_refine_f32: the 35 valid candidates in order, then (-inf, -1)
    for k_out in (10, 38):
        s, i = nat.refine_f32(qd, store.shadow, N, ID_BASE, ids_d, k_out)
        torch.cuda.synchronize()
        s, i = s.cpu().numpy(), i.cpu().numpy()
        m = min(k_out, 35)
        assert np.array_equal(i[:, :m], want_i[:, :m]), (k_out, i[0].tolist())
        assert np.abs(s[:, :m] - want_s[:, :m]).max() < SCORE_TOL32
        assert (i[:, m:] == -1).all() and np.isneginf(s[:, m:]).all()
    # crs_score_rows_f32: slot by slot; -1 -> -inf, the foreign id keeps the wrapper's -inf
    sc = nat.score_rows_f32(qd, store.shadow, N, ID_BASE, ids_d)
    torch.cuda.synchronize()
    sc = sc.cpu().numpy()
    at = {r: c for c, r in enumerate(rows)}
    for j in range(nq):
        for slot, gid in enumerate(ids[j].tolist()):
            row = gid - ID_BASE
            if 0 <= row < N and gid >= 0:
                assert abs(sc[j, slot] - s64[j, at[row]]) < SCORE_TOL32, (j, slot, row)
            else:
                assert np.isneginf(sc[j, slot]), (j, slot, gid)
    # crs_rescore_f32: in place; the foreign id's pre-filled 0.5 sorts between the planted (>= 0.6) and the background (<= 0.2) rows
    pre = torch.full(ids.shape, 0.5, dtype=torch.float32, device=cuda)
    ids_io = ids_d.clone()
    nat.rescore_f32(qd, store.shadow, N, ID_BASE, pre, ids_io)
    torch.cuda.synchronize()
    s, i = pre.cpu().numpy(), ids_io.cpu().numpy()
    for j in range(nq):
        exp_i = want_i[j, :15].tolist() + [ID_BASE - 3 - j] + want_i[j, 15:].tolist()
        exp_s = want_s[j, :15].tolist() + [0.5] + want_s[j, 15:].tolist()
        assert i[j, :36].tolist() == exp_i, (j, i[j].tolist())
        assert np.abs(s[j, :36] - np.asarray(exp_s)).max() < SCORE_TOL32 and s[j, 15] == np.float32(0.5)
        assert (i[j, 36:] == -1).all() and np.isneginf(s[j, 36:]).all()


def test_certificates_on_scan_candidates_with_an_id_base(store, cuda):
    """crs_refine_f32_cert on the scan's 24 candidates, and crs_refine_large_cert on the [parts, nq, 64] block of per-chunk scans,
    both with ids = rows + 2^40 + 5: the re-rank reads the shadow at every line."""
    import torch
    from rag import _native as nat
    nq = 2
    q, qd, q16, _ = _queries(cuda, nq, F16)
    planted_h = _planted_host(store)
    col = {r + ID_BASE: c for c, r in enumerate(hr.PLANTED_ROWS)}
    want = hr.planted_order(q, planted_h) + ID_BASE
    E = nat.exact_row_error_bound(DIM, F16)
    cs, ci = nat.cosine_topk(q16, store.slab, N, DIM, 24, id_base=ID_BASE)
    ws = torch.empty(nat.exact_workspace_bytes(nq), dtype=torch.uint8, device=cuda)
    s, i, status = nat.refine_f32_cert(qd, q16, store.shadow, N, ID_BASE, ci, cs, 10, E, F16, ws)
    torch.cuda.synchronize()
    _check_cert("refine_f32_cert", s, i, status, want[:, :10], q, planted_h, col)
    # the partitioned over-fetch by hand: chunk p = rows [p chunk_rows, (p + 1) chunk_rows), its slab top-64
    k_out, cap = 100, 4096
    parts, chunk_rows = nat.large_k_plan(k_out, N)
    cand_s = torch.empty((parts, nq, 64), dtype=torch.float32, device=cuda)
    cand_i = torch.empty((parts, nq, 64), dtype=torch.int64, device=cuda)
    for p in range(parts):
        lo, hi = p * chunk_rows, min(N, (p + 1) * chunk_rows)
        nat.cosine_topk(q16, store.slab[lo:hi], hi - lo, DIM, 64, id_base=ID_BASE + lo, out_scores=cand_s[p], out_ids=cand_i[p])
    ws = torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=cuda)
    s, i, status = nat.refine_large_cert(qd, q16, store.shadow, N, ID_BASE, cand_i, cand_s, chunk_rows, k_out, E, F16, ws, cap)
    torch.cuda.synchronize()
    s, i = s.cpu().numpy(), i.cpu().numpy()
    assert set(status.cpu().numpy().tolist()) <= {0, 1}
    assert np.array_equal(i[:, :15], want), i[0, :15].tolist()
    # fp64 from the gathered shadow rows: every candidate of the block, ranked on the host
    cand_h = cand_i.cpu().numpy()
    for j in range(nq):
        ids_j = np.unique(cand_h[:, j, :].reshape(-1))
        ids_j = ids_j[ids_j >= 0]
        rows_h = _host(store.shadow, ids_j - ID_BASE)
        s64 = hr.scores64(q[j:j + 1], rows_h)[0]
        order = np.lexsort((ids_j, -s64))
        ref_i, ref_s = ids_j[order][:k_out], s64[order][:k_out]
        score = dict(zip(ids_j.tolist(), s64.tolist()))
        got64 = np.asarray([score[int(x)] for x in i[j]])
        errs = _near_tie_errors(i[j:j + 1], ref_i[None, :], got64[None, :], ref_s[None, :], k_out, NEAR_TIE)
        assert not errs, (j, errs)
        assert np.abs(s[j] - got64).max() < SCORE_TOL32


@pytest.mark.parametrize("space", ["ip", "l2"])
def test_space_distances_at_the_lines(store, cuda, space):
    """crs_space_distances on the shadow read as an ip store of dimension 1024 and as an l2 store of dimension 1023 (the stored
    dimension is 1024 in both), scale 1: the distances of lists like the refiners', from the recovered vectors, against fp64."""
    import torch
    from rag import _native as nat
    nq = 4
    code = nat.SPACE_IP if space == "ip" else nat.SPACE_L2
    d = DIM if space == "ip" else DIM - 1
    q = np.ascontiguousarray((hr.queries(nq) * np.asarray([0.7, 1.0, 1.2, 1.4], dtype=np.float32)[:, None])[:, :d])
    rows, rows_h = _gathered(store)
    x = sr.recover(rows_h, space, 1.0)                                       # the caller's vectors: u (ip), 2 v (l2)
    metric = np.stack([sr.metric64_rows(q[j], x, space) for j in range(nq)])
    tol = np.stack([br.distance_tol_full(q[j], x, space) for j in range(nq)])
    ids, cols = _candidate_lists(rows, metric, tol, seed=5 + (space == "l2"))
    R = torch.ones(1, dtype=torch.float32, device=cuda)
    dist, out_i = nat.space_distances(torch.from_numpy(q).to(cuda), code, store.shadow, N, ID_BASE, R, torch.from_numpy(ids).to(cuda))
    torch.cuda.synchronize()
    dist, out_i = dist.cpu().numpy(), out_i.cpu().numpy()
    for j in range(nq):
        order = sorted(cols[j], key=lambda c: (metric[j, c], rows[c]))
        assert out_i[j, :35].tolist() == [rows[c] + ID_BASE for c in order], (space, j, out_i[j].tolist())
        assert (np.abs(dist[j, :35] - metric[j, order]) <= tol[j, order]).all(), (space, j)
        assert (out_i[j, 35:] == -1).all() and np.isposinf(dist[j, 35:]).all()


def test_mmr_order_on_rows_at_the_lines(store, cuda):
    """crs_mmr_order with vecs = the shadow: lists of the planted rows and background rows from around the lines, against
    tests/_mmr_ref.py by the rule of tests/test_mmr_gpu.py (every pick within eps of the round's best; the fp64 order itself where
    the smallest margin exceeds eps)."""
    import torch
    from rag import _native as nat
    rows, rows_h = _gathered(store)
    lam, m_max = 0.7, 32
    q = hr.queries(3).astype(np.float64)
    rng = np.random.default_rng(6)
    counts = np.asarray([32, 20, 2], dtype=np.int32)
    lists = np.full((3, m_max), -1, dtype=np.int64)
    rel = np.zeros((3, m_max), dtype=np.float64)
    vec_of = []
    for j in range(3):
        cols = list(range(hr.N_PLANTED)) + rng.choice(np.arange(hr.N_PLANTED, len(rows)), m_max - hr.N_PLANTED, replace=False).tolist()
        v = rows_h[cols].astype(np.float64)
        cos = (v / np.sqrt((v * v).sum(axis=1, keepdims=True))) @ q[j]
        best = np.argsort(-cos, kind="stable")[:counts[j]]
        lists[j, :counts[j]] = [rows[cols[b]] for b in best]
        rel[j, :counts[j]] = mr.store_score(cos[best])
        vec_of.append(v[best])
    order = nat.mmr_order(store.shadow, N, torch.from_numpy(lists).to(cuda), torch.from_numpy(rel).to(cuda), torch.from_numpy(counts).to(cuda), lam)
    torch.cuda.synchronize()
    order = order.cpu().numpy()
    eps = mr.eps_for(DIM, lam)
    exact = 0
    for j in range(3):
        c = int(counts[j])
        got = order[j, :c].tolist()
        assert sorted(got) == list(range(c)) and got[0] == 0 and (order[j, c:] == -1).all(), (j, order[j].tolist())
        assert mr.replay_ok(got, vec_of[j], rel[j, :c], lam, eps), (j, got)
        if mr.min_margin(vec_of[j], rel[j, :c], lam) >= eps:
            exact += 1
            assert got == mr.mmr_order_ref(vec_of[j], rel[j, :c], lam), (j, got)
    assert exact >= 1, "no list with a clear margin: the order itself was never compared"


@pytest.mark.parametrize("case", ["across 2^21", "low rows against the last rows"])
def test_near_duplicate_join_in_absolute_rows(store, cuda, case):
    """crs_pairs_above_f16 then crs_pairs_verify_f32 at threshold 0.4 over row ranges at the lines: a = b = [2^21 - 300, 2^21 + 300),
    and a = [0, 600) against b = [2^22 - 200, N).  join.hip forms 32-bit lane offsets from tile-relative rows: an absolute row there
    would read another tile.  The expectation is tests/_join_ref.py on host copies of the ranges' rows."""
    import torch
    from rag import _native as nat
    t, cap = 0.4, 4096
    if case == "across 2^21":
        a_abs = b_abs = (2 ** 21 - 300, 600)
        local_rows = np.arange(a_abs[0], a_abs[0] + 600)
        a_loc = b_loc = (0, 600)
    else:
        a_abs, b_abs = (0, 600), (2 ** 22 - 200, N - (2 ** 22 - 200))
        local_rows = np.concatenate([np.arange(0, 600), np.arange(b_abs[0], N)])
        a_loc, b_loc = (0, 600), (600, b_abs[1])
    to_local = {int(r): c for c, r in enumerate(local_rows)}
    slab_h, shadow_h = _host(store.slab, local_rows), _host(store.shadow, local_rows)
    pdim = store.slab.shape[1]
    E = nat.exact_row_error_bound(DIM, F16)
    assert jr.row_error_max(slab_h, shadow_h) <= E
    eps = nat.pairs_epsilon(E, pdim)
    jr.check_epsilon(eps, E, pdim)
    thr1, thr2 = nat.pairs_thresholds(t, eps)
    G = jr.gram64(shadow_h)
    jr.check_no_pair_near(G, (t,), eps, a_loc, b_loc)
    pairs, scores, count = nat.pairs_above(store.slab, N, DIM, a_abs, b_abs, thr1, cap)
    torch.cuda.synchronize()
    c = int(count.item())
    assert 0 < c <= cap
    p_abs, sc = pairs[:c].cpu().numpy(), scores[:c].cpu().numpy()
    in_a = (p_abs[:, 0] >= a_abs[0]) & (p_abs[:, 0] < a_abs[0] + a_abs[1])
    in_b = (p_abs[:, 1] >= b_abs[0]) & (p_abs[:, 1] < b_abs[0] + b_abs[1])
    assert in_a.all() and in_b.all(), "stage 1 lists rows that are not absolute row numbers of the ranges"
    p_loc = np.asarray([[to_local[int(x)], to_local[int(y)]] for x, y in p_abs], dtype=np.int64)
    jr.check_stage1(p_loc, sc, c, cap, slab_h, shadow_h, t, eps, thr1, a_loc, b_loc)
    # the hit count itself: no slab score lies within the accumulation term of thr1, so the count is the host's
    S = jr.gram64(slab_h)
    mask = jr._range_mask(len(local_rows), a_loc, b_loc)
    arith = (1.5 * pdim + 8.0) * 2.0 ** -23
    assert not (mask & (np.abs(S - thr1) <= arith)).any()
    assert c == int((mask & (S >= thr1)).sum()), (c, int((mask & (S >= thr1)).sum()))
    ra, rb, sims, kept = nat.pairs_verify(pairs[:c].contiguous(), store.shadow, N, thr2)
    torch.cuda.synchronize()
    k = int(kept.item())
    a, b, s = ra[:k].cpu().numpy(), rb[:k].cpu().numpy(), sims[:k].cpu().numpy()
    planted = set(hr.PLANTED_ROWS)
    assert k > 0 and all(int(x) in planted and int(y) in planted for x, y in zip(a, b)), (a.tolist(), b.tolist())
    la = np.asarray([to_local[int(x)] for x in a], dtype=np.int64)
    lb = np.asarray([to_local[int(x)] for x in b], dtype=np.int64)
    order = np.lexsort((lb, la))
    jr.check_exact_set({"rows_a": la[order], "rows_b": lb[order], "similarities": s[order]}, shadow_h, t, a_loc, b_loc, G=G)


def test_rows_norm_max_finds_the_last_row(store, cuda):
    """crs_rows_norm_max with emb = the shadow: row N - 1, scaled by 3 with torch, holds the maximum."""
    import torch
    from rag import _native as nat
    keep = store.shadow[N - 1].clone()
    try:
        store.shadow[N - 1] = keep * 3.0
        row = store.shadow[N - 1].cpu().numpy().astype(np.float64)
        true = float(np.sqrt((row * row).sum()))
        got = nat.rows_norm_max(store.shadow)
        assert 2.99 < true < 3.01 and abs(got - true) <= br.norm_max_rel_tol(DIM) * true, (got, true)
    finally:
        store.shadow[N - 1] = keep
        torch.cuda.synchronize()


# ================================================================================================================== writers
SPACES = {"cosine": 0, "ip": 1, "l2": 2}


def _new_vectors(m, space, seed, cuda):
    """m fp32 vectors of the dimension the space takes (1023 under l2: one more coordinate is stored), norms in (0.3, 1.9)."""
    import torch
    g = torch.Generator(device=cuda)
    g.manual_seed(seed)
    d = DIM - 1 if space == "l2" else DIM
    x = torch.randn((m, d), generator=g, device=cuda)
    x = x / x.norm(dim=1, keepdim=True) * torch.linspace(0.3, 1.9, m, device=cuda)[:, None]
    return x.contiguous()


class _Small:
    """A 64-row store of the same layout, zeroed."""

    def __init__(self, st, cuda):
        import torch
        self.slab = torch.zeros((64, DIM), dtype=torch.int8 if st == I8 else torch.float16, device=cuda)
        self.scales = torch.zeros(64, dtype=torch.float32, device=cuda) if st == I8 else None
        self.shadow = torch.zeros((64, DIM), dtype=torch.float32, device=cuda)
        self.err = torch.zeros(1, dtype=torch.float32, device=cuda)


def _append(space, emb, slab, row0, st, scales, shadow, err, R):
    from rag import _native as nat
    if space == "cosine":
        nat.slab_append_f32(emb, slab, row0, st, scales=scales, shadow=shadow, row_err=err)
    else:
        nat.slab_append_space_f32(emb, SPACES[space], R, slab, row0, scales=scales, shadow=shadow, row_err=err)


def _scatter(space, emb, rows, slab, n_rows, scales, shadow, err, R):
    from rag import _native as nat
    if space == "cosine":
        nat.slab_write_rows_f32(emb, rows, slab, n_rows, scales=scales, shadow=shadow, row_err=err)
    else:
        nat.slab_write_rows_space_f32(emb, rows, SPACES[space], R, slab, n_rows, scales=scales, shadow=shadow, row_err=err)


def _assert_written(store, st, rows, small, err, what):
    """rows `rows` of the store equal rows 0.. of the small store, bit for bit, in every array the writer owns."""
    sl, sc = store.arrays_of(st)
    idx = _idx(rows, store.device)
    m = len(rows)
    assert _same_bits(sl[idx], small.slab[:m]), f"{what}: slab rows differ from the small store's"
    assert _same_bits(store.shadow[idx], small.shadow[:m]), f"{what}: shadow rows differ from the small store's"
    if st == I8:
        assert _same_bits(sc[idx], small.scales[:m]), f"{what}: int8 scales differ from the small store's"
    assert float(small.err.item()) > 0.0 and _same_bits(err, small.err), f"{what}: row error {err.item()!r} vs {small.err.item()!r}"


@pytest.mark.parametrize("slab", ["f16", "i8"])
@pytest.mark.parametrize("space", ["cosine", "ip", "l2"])
def test_append_of_eight_rows_across_each_line(store, cuda, space, slab):
    """crs_slab_append_f32 / crs_slab_append_space_f32: 8 rows at row0 = X - 3 for every line X, with shadow and row error."""
    import torch
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    R = torch.full((1,), 2.0, dtype=torch.float32, device=cuda)
    for n_line, X in enumerate(hr.LINES):
        rows = list(range(X - 3, X + 5))
        near = [r for r in _around(rows) if r not in rows]
        alias = hr.alias_rows(rows, store.geometry)
        assert near and alias and not set(alias) & set(rows)
        snap = _Snap(store, rows + near + alias)
        emb = _new_vectors(8, space, 100 + n_line, cuda)
        small = _Small(st, cuda)
        err = torch.zeros(1, dtype=torch.float32, device=cuda)
        try:
            _append(space, emb, sl, X - 3, st, sc, store.shadow, err, R)
            _append(space, emb, small.slab, 0, st, small.scales, small.shadow, small.err, R)
            torch.cuda.synchronize()
            _assert_written(store, st, rows, small, err, (space, slab, X))
            snap.assert_unchanged(store, near + alias, (space, slab, X))
        finally:
            snap.restore(store)
            torch.cuda.synchronize()


@pytest.mark.parametrize("slab", ["f16", "i8"])
@pytest.mark.parametrize("space", ["cosine", "ip", "l2"])
def test_scatter_to_all_line_rows_in_one_call(store, cuda, space, slab):
    """crs_slab_write_rows_f32 / crs_slab_write_rows_space_f32 to the 13 line rows in shuffled order."""
    import torch
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    R = torch.full((1,), 2.0, dtype=torch.float32, device=cuda)
    rows = np.random.default_rng(9).permutation(np.asarray(hr.LINE_ROWS)).tolist()
    assert rows != sorted(rows)
    near = [r for r in _around(rows) if r not in rows]
    alias = hr.alias_rows(rows, store.geometry)                 # (aliases that are written rows themselves are not in it)
    snap = _Snap(store, rows + near + alias)
    emb = _new_vectors(len(rows), space, 200, cuda)
    small = _Small(st, cuda)
    err = torch.zeros(1, dtype=torch.float32, device=cuda)
    try:
        _scatter(space, emb, _idx(rows, cuda), sl, N, sc, store.shadow, err, R)
        _scatter(space, emb, torch.arange(len(rows), device=cuda), small.slab, 64, small.scales, small.shadow, small.err, R)
        torch.cuda.synchronize()
        _assert_written(store, st, rows, small, err, (space, slab))
        snap.assert_unchanged(store, near + alias, (space, slab))
    finally:
        snap.restore(store)
        torch.cuda.synchronize()


@pytest.mark.parametrize("slab", ["f16", "i8"])
def test_whole_store_append_from_the_shadow(store, cuda, slab):
    """crs_slab_append_f32(emb = shadow, row0 = 0, n = N): the source offset r * dim crosses every line as well (the shadow is also
    the destination's shadow: slab_row.h reads a row before it writes it).  The line rows equal the same fp32 rows appended into a
    small store; the scan returns the planted list afterwards."""
    import torch
    from rag import _native as nat
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    rows = sorted(hr.LINE_ROWS)
    old = store.shadow[_idx(rows, cuda)].clone()
    small = _Small(st, cuda)
    err = torch.zeros(1, dtype=torch.float32, device=cuda)
    try:
        nat.slab_append_f32(store.shadow, sl, 0, st, scales=sc, shadow=store.shadow, row_err=err)
        nat.slab_append_f32(old, small.slab, 0, st, scales=small.scales, shadow=small.shadow, row_err=small.err)
        torch.cuda.synchronize()
        idx = _idx(rows, cuda)
        assert _same_bits(sl[idx], small.slab[:len(rows)]) and _same_bits(store.shadow[idx], small.shadow[:len(rows)])
        if st == I8:
            assert _same_bits(sc[idx], small.scales[:len(rows)])
        assert float(small.err.item()) <= float(err.item()) <= nat.exact_row_error_bound(DIM, st)
        q, qd, q16, _ = _queries(cuda, 16, st)
        s, i = nat.cosine_topk(q16, sl, N, DIM, 15, slab_type=st, scales=sc)
        torch.cuda.synchronize()
        assert np.array_equal(i.cpu().numpy(), hr.planted_order(q, _planted_host(store)))
    finally:
        store.rebuild()


@pytest.mark.parametrize("slab", ["f16", "i8"])
def test_rescale_of_the_whole_store(store, cuda, slab):
    """crs_slab_rescale_space (ip, shift 1) over all N rows: at the sampled rows the shadow is the old row x 0.5 exactly and the slab
    (and the int8 scale) is the image of the old row stored under R = 2 in a small store."""
    import torch
    from rag import _native as nat
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    rows = sorted(set(_around(hr.LINE_ROWS)) | {5, 2 ** 22 + 300})
    assert len(rows) <= 64
    idx = _idx(rows, cuda)
    old = store.shadow[idx].clone()
    small = _Small(st, cuda)
    err = torch.zeros(1, dtype=torch.float32, device=cuda)
    try:
        nat.slab_rescale_space(N, DIM, nat.SPACE_IP, 1, sl, store.shadow, scales=sc, row_err=err)
        nat.slab_append_space_f32(old, nat.SPACE_IP, torch.full((1,), 2.0, device=cuda), small.slab, 0, scales=small.scales,
                                  shadow=small.shadow, row_err=small.err)
        torch.cuda.synchronize()
        assert _same_bits(store.shadow[idx], old * 0.5), "shadow is not the old row x 0.5"
        assert _same_bits(store.shadow[idx], small.shadow[:len(rows)])
        assert _same_bits(sl[idx], small.slab[:len(rows)]), "slab rows differ from the small store's image"
        if st == I8:
            assert _same_bits(sc[idx], small.scales[:len(rows)])
        assert 0.0 < float(small.err.item()) <= float(err.item()) <= nat.exact_row_error_bound(DIM, st)
    finally:
        store.rebuild()


DEAD = np.asarray(sorted({7, 2 ** 20 + 5, 2 ** 21 - 2, 2 ** 22 + 9} | set(range(2 ** 19, 2 ** 19 + 100))), dtype=np.int64)


@pytest.mark.parametrize("slab,bounce", [("f16", "default"), ("f16", "minimum"), ("i8", "minimum")])
def test_compaction_moves_every_row_across_the_lines(store, cuda, slab, bounce):
    """crs_slab_compact with shadow, scales and rows_global, 104 dead rows from row 7 on: every later row moves, through a bounce
    buffer of compact_bounce_size (one window of 43 584 rows at a time) and through the smallest legal one (1024 rows: thousands of
    windows that start above the lines).  Destination rows [X - 110, X + 3) around every line, the head and the last survivor equal
    the snapshot of their source rows in all four arrays; the scan returns the surviving planted rows at their new numbers."""
    import torch
    from rag import _native as nat
    st = I8 if slab == "i8" else F16
    sl, sc = store.arrays_of(st)
    scales = store.scales                                      # (an fp16 store carries no scales; the kernel moves them all the same)
    n_out = N - len(DEAD)
    dst = sorted({d for X in hr.LINES for d in range(X - 110, X + 3)} | set(range(0, 10)) | {n_out - 1})
    src = [hr.source_row(d, DEAD) for d in dst]
    assert src[-1] == N - 1 and not set(src) & set(DEAD.tolist()) and sum(s != d for s, d in zip(src, dst)) > 400
    si, di = _idx(src, cuda), _idx(dst, cuda)
    rows_global = torch.arange(N, device=cuda) * 3 + 7
    snap = [a[si].clone() for a in (sl, scales, store.shadow, rows_global)]
    if bounce == "default":
        nbytes, first = nat.compact_bounce_size(N, DIM, st, True), int(DEAD[0])
    else:
        nbytes, first = nat.slab_compact_bounce_bytes(DIM, st, True), 0
        assert nat.slab_compact_window_rows(DIM, st, True, nbytes) == 1024
    buf = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    try:
        nat.slab_compact(torch.from_numpy(DEAD).to(cuda), N, sl, scales=scales, shadow=store.shadow, rows_global=rows_global, bounce=buf,
                         first_row=first)
        torch.cuda.synchronize()
        for name, arr, want in zip(("slab", "scales", "shadow", "rows_global"), (sl, scales, store.shadow, rows_global), snap):
            assert _same_bits(arr[di], want), f"{name}: a destination row is not its source row"
        q, qd, q16, _ = _queries(cuda, 16, st)
        s, i = nat.cosine_topk(q16, sl, n_out, DIM, 15, slab_type=st, scales=sc)
        torch.cuda.synchronize()
        i = i.cpu().numpy()
        alive = [r for r in hr.PLANTED_ROWS if r not in set(DEAD.tolist())]
        assert len(alive) == 13                                 # rows 2^19 and 2^19 + 1 are among the dead
        col = {r: c for c, r in enumerate(hr.PLANTED_ROWS)}
        planted_h = hr.planted_vectors()[[col[r] for r in alive]]
        want = hr.planted_order(q, planted_h, rows=alive)
        want = np.vectorize(lambda r: hr.shifted_row(int(r), DEAD))(want)
        assert np.array_equal(i[:, :13], want), (i[0].tolist(), want[0].tolist())
        assert not np.isin(i[:, 13:], want[0]).any() and ((i[:, 13:] >= 0) & (i[:, 13:] < n_out)).all()
    finally:
        del buf, snap, rows_global
        store.rebuild()


def test_peak_memory_stays_under_40_gb(store, cuda):
    """Runs last: the peak of everything this module allocated so far, above what the process held before the fixture."""
    import torch
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - store.base_bytes
    print(f"peak device memory of the high-row module: {peak / 1e9:.2f} GB")
    assert peak < PEAK_LIMIT, peak
