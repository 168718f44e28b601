"""GPU: the split list of csrc/scan_wide.hip's 24- / 32-slot forms (one K-slot list per lane pair, ranks 0 .. K/2 - 1 in the
lower half and K/2 .. K - 1 in the upper one) and the stagger of scan_wide_kernel<384, 8, 24>.

Every case scans 384-element rows with 256 workgroups x 64-row tiles.  ``cosine_topk_cert`` at k' = 24 / 32, k = 10, then
``escalate_exact``, against the same queries as 64-query calls (scan_tb.hip) and against oracle/scan_ref.py on the fp32 rows:
final ids equal, final scores bit for bit, candidate id sets equal, no status 2.

Corpora, planted under a handful of queries each on top of seeded unit rows:
  (a) one planted row per tile whose score under query direction A rises with the row index: every tile enters a workgroup's list
      at rank 0, every insertion pushes the lower half's last entry into the upper half;
  (b) the same under direction B, falling: after the fill every tile goes to the upper half or nowhere;
  (c) 30 exact copies of one row in 30 tiles of ONE workgroup (rows at a stride of 256 x 64 under the static stride): equal scores
      over ranks 0 .. 23, straddling 11 / 12 and 23 / 24 -- the lower rows win, in row order;
  (d) n = 64 x 256 x 12 + 5: twelve tiles per workgroup, the upper half stays empty (workgroup 0, with the ragged 13th tile, has
      exactly one entry in it);
  (e) n = 64 x 256 x 2 + 1 and 64 x 256 x 3: two / three tiles per workgroup -- one deferred tile, even and odd counts.

The partial lists are read out of the caller's scan workspace, whose layout capi.hip states ("scan workspace": the ticket /
threshold words, then [nq, streams, kp] scores, then [nq, streams, kp] rows, each block 256-byte aligned).

Knobs: CRS_WIDE_STAGGER=0 x CRS_WIDE_DYN=0 / forced tickets (CRS_TB_DYN_MIN=8).  Candidates, finals and both status words are
bit-identical over the four combinations.  The partial lists are bit-identical between the two stagger settings under the
static stride; under tickets a workgroup's tiles depend on the order the counter was drawn in, so what is compared there is
what the merge reads: the K best (score desc, row asc) of a query's pooled lists, which every assignment leaves the same."""
import os

import numpy as np
import pytest

from oracle import scan_ref
from topk_check import assert_topk

pytestmark = pytest.mark.gpu

D, NWG, TILE, K_OUT = 384, 256, 64, 10
N_MAIN = 600_011                       # 9376 tiles, 36 or 37 per workgroup: a 24-slot and a 32-slot list overflow
N_HALF = TILE * NWG * 12 + 5           # (d)
N_TWO, N_THREE = TILE * NWG * 2 + 1, TILE * NWG * 3    # (e)
C_WG = 17                              # the workgroup (static stride: tile stream) that sees every copy of corpus (c)
Q_A, Q_B, Q_C = (2, 37, 100, 190), (5, 66, 133, 180), (9, 75, 150, 192)    # queries on (a), (b), (c): all below 193, every wave pair


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


def _copy_rows(n):
    return [r for r in (C_WG * TILE + 3 + i * NWG * TILE for i in range(30)) if r < n]


def _world(cuda, n):
    """slab + shadow of n seeded unit rows with (a), (b), (c) planted, 256 queries, the oracle's top-10 of all of them; one
    store at a time on the device, built once per size"""
    import torch
    from rag import _native as nat
    if n in _WORLDS:
        return _WORLDS[n]
    _WORLDS.clear()
    torch.cuda.empty_cache()
    g = torch.Generator(device=cuda)
    g.manual_seed(n)
    rows = torch.nn.functional.normalize(torch.randn((n, D), generator=g, device=cuda), dim=1)
    dirs = torch.nn.functional.normalize(torch.randn((2, D), generator=g, device=cuda), dim=1)
    n_tiles = (n + TILE - 1) // TILE
    t = torch.arange(n_tiles, device=cuda, dtype=torch.float32) / max(n_tiles - 1, 1)
    # a seeded unit row scores N(0, 1/384) under any direction: 0.3 is six sigma, above the best of 600 k rows; between
    # consecutive tiles of a workgroup (256 tiles apart) the planted scores differ by >= 0.6 * 256 / 9376 = 0.016, or by 0.2 and
    # more on the short streams -- far above the fp16 rounding of a row (5e-4)
    for which, (off, alpha) in enumerate(((5, 0.3 + 0.6 * t), (9, 0.9 - 0.6 * t))):
        at = torch.arange(n_tiles, device=cuda) * TILE + off
        keep = at < n
        at, al = at[keep], alpha[keep][:, None]
        noise = rows[at] - (rows[at] @ dirs[which])[:, None] * dirs[which]
        noise = torch.nn.functional.normalize(noise, dim=1)
        rows[at] = torch.nn.functional.normalize(al * dirs[which] + torch.sqrt(1 - al * al) * noise, dim=1)
    copies = _copy_rows(n)
    rows[copies] = rows[copies[0]].clone()
    slab = torch.zeros((n, nat.padded_dim(D)), dtype=torch.float16, device=cuda)
    shadow = torch.empty((n, D), dtype=torch.float32, device=cuda)
    row_err = torch.zeros(1, dtype=torch.float32, device=cuda)
    for lo in range(0, n, 250_000):
        nat.slab_append_f32(rows[lo:lo + 250_000].contiguous(), slab, lo, nat.SLAB_F16, shadow=shadow, row_err=row_err)
    q = torch.randn((256, D), generator=g, device=cuda)
    j = torch.randint(0, n, (256,), generator=g, device=cuda)
    q[0::2] = shadow[j[0::2]] + 0.1 * q[0::2]                   # every second query near a row
    for qs, centre in ((Q_A, dirs[0]), (Q_B, dirs[1]), (Q_C, shadow[copies[0]])):
        for i, qi in enumerate(qs):
            q[qi] = centre + (0.0 if i == 0 else 0.02) * q[qi]   # the first of each handful sits exactly on the direction
    q32 = torch.nn.functional.normalize(q, dim=1).contiguous()
    rows_h, q_h = shadow.cpu().numpy(), q32.cpu().numpy()
    ref = scan_ref.cosine_topk_ref(q_h, rows_h, K_OUT)
    _WORLDS[n] = dict(n=n, slab=slab, shadow=shadow, row_err=float(row_err.item()), q32=q32, rows_h=rows_h, q_h=q_h, ref=ref, copies=copies)
    return _WORLDS[n]


def _cert(cuda, w, q32, kc, want_parts=False, cap=1024):
    """one cosine_topk_cert + escalate_exact; outputs on the host, with the partial lists [nq, streams, kp] where asked"""
    import torch
    from rag import _native as nat
    n, nq = w["n"], q32.shape[0]
    q16 = nat.queries_to_f16(q32, nat.SLAB_F16)
    ews = torch.empty(nat.exact_workspace_bytes(nq, cap), dtype=torch.uint8, device=cuda)
    cs = torch.full((nq, kc), 7.5, dtype=torch.float32, device=cuda)
    ci = torch.full((nq, kc), -5, dtype=torch.int64, device=cuda)
    ws = torch.full((nat.scan_workspace_bytes(nq, D, kc, n),), 0x5a, dtype=torch.uint8, device=cuda)
    s, i, st = nat.cosine_topk_cert(q32, q16, w["slab"], w["shadow"], n, D, kc, K_OUT, w["row_err"], ews, cap, workspace=ws,
                                    cand_scores=cs, cand_ids=ci)
    st0 = st.clone()
    nat.escalate_exact(q32, q16, w["slab"], w["shadow"], n, 0, K_OUT, s, i, st, ews, cap)
    torch.cuda.synchronize()
    out = {name: t.cpu().numpy() for name, t in {"s": s, "i": i, "cand_s": cs, "cand_i": ci, "st0": st0, "st1": st}.items()}
    if want_parts:
        kp = 2 * (24 if kc <= 24 else 32)
        al = lambda b: (b + 255) // 256 * 256
        o_s = al(nq * 4)
        o_r = o_s + al(NWG * nq * kp * 4)
        raw = ws.cpu().numpy()
        out["part_s"] = raw[o_s:o_s + NWG * nq * kp * 4].view(np.float32).reshape(nq, NWG, kp).copy()
        out["part_r"] = raw[o_r:o_r + NWG * nq * kp * 4].view(np.int32).reshape(nq, NWG, kp).copy()
    return out


def _plan_is_split(n, nq, kc):
    from rag import _native as nat
    plan = nat.scan_plan_describe(nq, D, kc, n)
    K = 24 if kc <= 24 else 32
    assert f"scan_wide_kernel<384,8,{K}>" in plan and f"streams={NWG} " in plan and "qblocks=1" in plan and f"kp={2 * K}" in plan, plan
    return K


def _check_against_64_and_oracle(cuda, w, nq, kc, wide=None):
    n = w["n"]
    q32 = w["q32"][:nq].contiguous()
    wide = wide if wide is not None else _cert(cuda, w, q32, kc)
    parts = [_cert(cuda, w, q32[lo:lo + 64].contiguous(), kc) for lo in range(0, nq, 64)]
    narrow = {name: np.concatenate([p[name] for p in parts]) for name in parts[0]}
    print(f"n={n} nq={nq} k'={kc}: status-1 wide {int((wide['st0'] == 1).sum())} / 64-query calls {int((narrow['st0'] == 1).sum())}; "
          f"ids equal {(wide['i'] == narrow['i']).mean():.6f}")
    assert not (wide["st1"] == 2).any() and not (narrow["st1"] == 2).any()
    assert set(np.unique(wide["st0"])) <= {0, 1}
    assert np.array_equal(wide["i"], narrow["i"])
    assert np.array_equal(wide["s"].view(np.int32), narrow["s"].view(np.int32))
    assert np.array_equal(np.sort(wide["cand_i"], axis=1), np.sort(narrow["cand_i"], axis=1))
    assert_topk(wide["s"], wide["i"], w["q_h"][:nq], w["rows_h"], K_OUT, f"n={n} nq={nq} k'={kc}", ref=(w["ref"][0][:nq], w["ref"][1][:nq]))
    copies = w["copies"]
    for qi in Q_C:      # exact ties: the lower rows win, in row order -- in the finals and in the candidates
        m = min(K_OUT, len(copies))
        assert wide["i"][qi][:m].tolist() == copies[:m], (qi, wide["i"][qi].tolist())
        m = min(kc, len(copies))
        assert set(copies[:m]) <= set(wide["cand_i"][qi].tolist()), (qi, sorted(wide["cand_i"][qi].tolist()))
        if len(copies) >= kc:
            assert sorted(wide["cand_i"][qi].tolist()) == copies[:kc]
    return wide


@pytest.mark.parametrize("kc", [24, 32])
@pytest.mark.parametrize("nq", [256, 193])
def test_split_list_is_the_64_query_calls(cuda, nq, kc):
    w = _world(cuda, N_MAIN)
    _plan_is_split(N_MAIN, nq, kc)
    _check_against_64_and_oracle(cuda, w, nq, kc)


def _lists_are_well_formed(part_s, part_r, K, n, what):
    """ranks 0 .. K - 1: score desc, empty slots (-inf, -1) last, rows are distinct first rows of tiles; ranks K .. 2 K - 1: the pad"""
    assert np.isneginf(part_s[:, :, K:]).all() and (part_r[:, :, K:] == -1).all(), f"{what}: pad"
    s, r = part_s[:, :, :K], part_r[:, :, :K]
    assert (s[:, :, 1:] <= s[:, :, :-1]).all(), f"{what}: order"
    empty = r == -1
    assert np.array_equal(empty, np.isneginf(s)), f"{what}: empty slots"
    assert ((r[~empty] >= 0) & (r[~empty] < n) & (r[~empty] % TILE == 0)).all(), f"{what}: rows"
    rs = np.sort(np.where(empty, np.arange(K)[None, None, :] - 2 * K, r), axis=2)      # distinct negative stand-ins for empty slots
    assert (np.diff(rs, axis=2) != 0).all(), f"{what}: a tile twice"
    return empty


@pytest.mark.parametrize("kc", [24, 32])
def test_partial_lists_hold_one_sorted_list_and_the_pad(cuda, kc):
    w = _world(cuda, N_MAIN)
    K = _plan_is_split(N_MAIN, 256, kc)
    with _Env(CRS_WIDE_DYN=0):
        got = _cert(cuda, w, w["q32"], kc, want_parts=True)
    empty = _lists_are_well_formed(got["part_s"], got["part_r"], K, N_MAIN, f"k'={kc}")
    assert not empty.any()                          # 36 tiles and more per workgroup: both halves are full
    stream = got["part_r"][:, :, :K] // TILE % NWG      # static stride: workgroup b keeps tiles of its own stream only
    assert (stream == np.arange(NWG)[None, :, None]).all()
    tiles = (N_MAIN + TILE - 1) // TILE
    for qi in (Q_A[0], Q_B[0]):                     # (a): the K LAST tiles of every stream, latest first; (b): the K FIRST, in order
        for b in (0, C_WG, NWG - 1):
            mine = np.arange(b, tiles, NWG) * TILE
            want = mine[::-1][:K] if qi == Q_A[0] else mine[:K]
            assert got["part_r"][qi, b, :K].tolist() == want.tolist(), (qi, b)
    for qi in Q_C:                                  # (c): the first K copies, in row order, in the one workgroup that sees them
        m = min(K, len(w["copies"]))
        assert got["part_r"][qi, C_WG, :m].tolist() == [r - 3 for r in w["copies"][:m]]
        assert len(set(got["part_s"][qi, C_WG, :m].view(np.int32).tolist())) == 1


@pytest.mark.parametrize("kc", [24, 32])
@pytest.mark.parametrize("n", [N_HALF, N_TWO, N_THREE])
def test_short_streams_leave_the_upper_half_empty(cuda, n, kc):
    """(d), (e): fewer tiles per workgroup than the lower half holds; 2 / 3 tiles per workgroup with and without the stagger"""
    w = _world(cuda, n)
    K = _plan_is_split(n, 256, kc)
    got = _cert(cuda, w, w["q32"], kc, want_parts=True)
    with _Env(CRS_WIDE_STAGGER=0):
        plain = _cert(cuda, w, w["q32"], kc, want_parts=True)
    for name in got:
        assert np.array_equal(got[name].view(np.int32) if got[name].dtype == np.float32 else got[name],
                              plain[name].view(np.int32) if plain[name].dtype == np.float32 else plain[name]), name
    empty = _lists_are_well_formed(got["part_s"], got["part_r"], K, n, f"n={n} k'={kc}")
    tiles = (n + TILE - 1) // TILE
    per_wg = np.array([len(range(b, tiles, NWG)) for b in range(NWG)])
    assert np.array_equal((~empty).sum(axis=2), np.broadcast_to(np.minimum(per_wg, K)[None, :], empty.shape[:2]))
    if n == N_HALF and kc == 24:      # twelve tiles: the upper half holds nothing, but for the 13th (ragged) tile of workgroup 0
        assert per_wg.tolist() == [13] + [12] * (NWG - 1)
        assert empty[:, 1:, K // 2:].all() and not empty[:, :, :K // 2].any()
        assert not empty[:, 0, K // 2].any() and empty[:, 0, K // 2 + 1:].all()
    _check_against_64_and_oracle(cuda, w, 256, kc, wide=got)


def _pooled_best(part_s, part_r, K):
    """what the merge reads: per query the K best (score desc, row asc) entries over all workgroups' lists"""
    nq = part_s.shape[0]
    s, r = part_s.reshape(nq, -1), part_r.reshape(nq, -1)
    out_s, out_r = np.empty((nq, K), np.float32), np.empty((nq, K), np.int32)
    for q in range(nq):
        o = np.lexsort((r[q], -s[q]))[:K]
        out_s[q], out_r[q] = s[q][o], r[q][o]
    return out_s, out_r


def test_stagger_and_schedule_knobs_leave_every_list_bit_identical(cuda):
    w = _world(cuda, N_MAIN)
    K = _plan_is_split(N_MAIN, 256, 24)
    runs = {}
    for stagger in ("default", "0"):
        for sched, env in (("static", dict(CRS_WIDE_DYN=0)), ("tickets", dict(CRS_TB_DYN_MIN=8))):
            if stagger == "0":
                env = dict(env, CRS_WIDE_STAGGER=0)
            with _Env(**env):
                runs[(stagger, sched)] = _cert(cuda, w, w["q32"], 24, want_parts=True)
    base = runs[("default", "static")]
    bits = lambda x: x.view(np.int32) if x.dtype == np.float32 else x
    for key, got in runs.items():
        for name in ("s", "i", "cand_s", "cand_i", "st0", "st1"):
            assert np.array_equal(bits(got[name]), bits(base[name])), (key, name)
        _lists_are_well_formed(got["part_s"], got["part_r"], K, N_MAIN, str(key))
    for name in ("part_s", "part_r"):       # same tiles per workgroup: the lists themselves
        assert np.array_equal(bits(runs[("0", "static")][name]), bits(base[name])), name
    want = _pooled_best(base["part_s"], base["part_r"], K)
    for key, got in runs.items():           # any assignment of tiles to workgroups: the K best of the pooled lists
        ps, pr = _pooled_best(got["part_s"], got["part_r"], K)
        assert np.array_equal(ps.view(np.int32), want[0].view(np.int32)) and np.array_equal(pr, want[1]), key
    _check_against_64_and_oracle(cuda, w, 256, 24, wide=runs[("0", "tickets")])


def test_cosine_topk_at_24_returns_24_distinct_rows(cuda):
    """the pad never reaches the merge's output: plain cosine_topk at k = 24 over n >= 24 x 64 rows"""
    import torch
    from rag import _native as nat
    w = _world(cuda, N_MAIN)
    q16 = nat.queries_to_f16(w["q32"], nat.SLAB_F16)
    s, i = nat.cosine_topk(q16, w["slab"], N_MAIN, D, 24)
    torch.cuda.synchronize()
    i, s = i.cpu().numpy(), s.cpu().numpy()
    assert ((i >= 0) & (i < N_MAIN)).all() and np.isfinite(s).all()
    assert (np.diff(np.sort(i, axis=1), axis=1) > 0).all()
    for qi in Q_C:
        assert i[qi].tolist() == w["copies"][:24]
