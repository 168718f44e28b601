"""GPU: the deferred insertion of csrc/scan_wide.hip's split-list forms (header: "Deferred insertion") leaves every list bit for
bit what the chain on every tile (CRS_WIDE_DEFER=0) leaves, and that is the oracle's ranking.

Shape: 256 queries (and 200: wave 7 idle, wave 6 a quarter valid) x 384-element fp16 rows, 409 600 + 37 rows -- 256 streams of
64-row tiles see 25 tiles each, one more than a 24-slot list holds, and the 37 extra rows make a ragged last tile; 25 rounds are
below the ticket schedule's threshold, so a stream's tiles and with them the partial lists are the same in every run.

Data (seeded on the host, fp16):
  random      unit rows, queries near rows;
  ascending   the same rows sorted by their score under query 0, rising: for that query every tile is a candidate;
  descending  falling: no candidate after the list is full;
  dup_stream  2 000 copies of one row: all 1 600 rows of stream 17's 25 tiles and the first 400 of stream 18's (a stream has no
              more rows than that) -- equal scores over a whole list and past its end; queries 3 and 130 sit on / beside the row;
  dup_spread  the 2 000 copies every 204 rows, over all streams.
Settings: K' = 24 and 32, CRS_WIDE_MFMA = 16 and 32, CRS_WIDE_STAGGER = 0 and default; 256-element rows at K' = 24 once.  (All three
knobs are read at every plan, so they are flipped inside the process.)

Per setting ``nat.cosine_topk`` runs with the deferral on and with CRS_WIDE_DEFER=0: scores, ids and the partial lists in the
caller's workspace (capi.hip, "scan workspace": threshold words, then [nq, streams, kp] scores, then rows, 256-byte aligned) must
be equal bit for bit.  The default's ids must be those of oracle/scan_ref.py, and the scores within topk_check.TIGHT_TOL (2e-5), the
tolerance tests/test_scan_wide_gpu.py holds fp16 slabs to.  The bit-for-bit comparison and the oracle's ids are two tests per
corpus, so that the first does not hide behind the second.

The oracle's ids are its exact ranking: ``cosine_topk_ref`` (fp64 accumulation) names k + 8 candidates per query, and they are
ranked by ``full_scores_f64`` (score desc, id asc).  The products of fp16 values are multiples of 2^-48 and sums of 384 of them
below 1 fit fp64's 53 bits, so these scores are exact and equal rows tie exactly, lower id first.  ``cosine_topk_ref`` alone does
not give that ranking: whatever it accumulates in, it rounds every score to fp32 BEFORE it selects, so two rows whose exact scores
fall between the same two fp32 numbers tie there and come out lower id first, whichever is the better.  That happened to a first
version of this test on "ascending": query 248's rows 238662 and 100334 score 0.196739604957 and 0.196739599353 exactly (5.6e-9
apart, an fp32 step is 1.5e-8 there), the rounded oracle tied them and put 100334 first, and the kernel, whose fp32 sums are
0x3e49761c and 0x3e49761b, had them in the exact order.  (With fp32 accumulation the oracle's BLAS sums carry rounding of their
own and differ from its fp64 ranking on one other list of the "dup" corpora.)  The eight spare candidates cover a rounded score
that falls a few places behind its exact rank."""
import os

import numpy as np
import pytest

from oracle import scan_ref
from topk_check import TIGHT_TOL

pytestmark = pytest.mark.gpu

N, TILE, NWG = 409_600 + 37, 64, 256
COPIES, Q_ON, Q_NEAR = 2000, 3, 130
KINDS = ("random", "ascending", "descending", "dup_stream", "dup_spread")


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


_BASE = {}
_WORLD = {}


def _base(d):
    """seeded unit rows and 256 queries near rows, fp16, once per row length"""
    if d not in _BASE:
        c = scan_ref.synth_corpus(N, d, seed=1234 + d)
        q = scan_ref.synth_queries(c, 256, seed=4321 + d)
        _BASE[d] = (q.astype(np.float16), c.astype(np.float16))
    return _BASE[d]


def _copy_rows(kind):
    if kind == "dup_spread":
        return np.arange(COPIES) * (N // COPIES)
    tiles17 = np.arange(17, N // TILE, NWG)[:25]
    rows17 = (tiles17[:, None] * TILE + np.arange(TILE)[None, :]).ravel()
    tiles18 = np.arange(18, N // TILE, NWG)
    rows18 = (tiles18[:, None] * TILE + np.arange(TILE)[None, :]).ravel()[:COPIES - rows17.size]
    return np.sort(np.concatenate([rows17, rows18]))


def _exact_topk(q, c, k, spare=8):
    """the oracle's ranking by exact scores (module docstring): (scores fp32, ids) [nq, k]"""
    _, cand = scan_ref.cosine_topk_ref(q, c, k + spare, accumulate=np.float64)
    out_s, out_i = np.empty((q.shape[0], k), np.float32), np.empty((q.shape[0], k), np.int64)
    for r in range(q.shape[0]):
        f64 = scan_ref.full_scores_f64(q[r:r + 1], c[cand[r]])[0]
        o = np.lexsort((cand[r], -f64))[:k]
        out_s[r], out_i[r] = f64[o], cand[r][o]
    return out_s, out_i


def _world(cuda, kind, d):
    """the slab on the device, the queries and the oracle's exact top-32; one corpus at a time"""
    import torch
    if (kind, d) in _WORLD:
        return _WORLD[(kind, d)]
    _WORLD.clear()
    torch.cuda.empty_cache()
    q, c = _base(d)
    q = q.copy()
    if kind in ("ascending", "descending"):
        s0 = c.astype(np.float32) @ q[0].astype(np.float32)
        order = np.argsort(s0, kind="stable")
        c = c[order if kind == "ascending" else order[::-1]]
    elif kind.startswith("dup"):
        c = c.copy()
        at = _copy_rows(kind)
        c[at] = c[at[0]]
        q[Q_ON] = c[at[0]]
        q[Q_NEAR] = (c[at[0]].astype(np.float32) + 0.02 * q[Q_NEAR].astype(np.float32)).astype(np.float16)
    ref_s, ref_i = _exact_topk(q, c, 32)
    w = dict(q=torch.from_numpy(q).to(cuda), slab=torch.from_numpy(np.ascontiguousarray(c)).to(cuda), ref_s=ref_s, ref_i=ref_i, d=d, c=c, qh=q,
             copies=_copy_rows(kind) if kind.startswith("dup") else None)
    _WORLD[(kind, d)] = w
    return w


def _scan(cuda, w, nq, k):
    """one cosine_topk; scores, ids and the partial-list block of the workspace, on the host"""
    import torch
    from rag import _native as nat
    d = w["d"]
    plan = nat.scan_plan_describe(nq, d, k, N)
    assert f"scan_wide_kernel<{d},8,{k}>" in plan and f"streams={NWG} " in plan and f"kp={2 * k}" in plan, plan
    ws = torch.full((nat.scan_workspace_bytes(nq, d, k, N),), 0x5a, dtype=torch.uint8, device=cuda)
    s, i = nat.cosine_topk(w["q"][:nq].contiguous(), w["slab"], N, d, k, workspace=ws)
    torch.cuda.synchronize()
    al = lambda b: (b + 255) // 256 * 256
    lo = al(nq * 4)
    parts = ws[lo:lo + 2 * al(NWG * nq * 2 * k * 4)].cpu().numpy()
    return s.cpu().numpy(), i.cpu().numpy(), parts


_RUNS = {}


def _runs(cuda, kind, d, settings):
    """every setting once, deferral on and CRS_WIDE_DEFER=0: {what: (nq, k, deferred, plain)}; shared by the tests of a corpus"""
    if (kind, d) not in _RUNS:
        _RUNS.clear()
        w = _world(cuda, kind, d)
        out = {}
        for nq, k, env, what in settings:
            with _Env(**env):
                got = _scan(cuda, w, nq, k)
                with _Env(CRS_WIDE_DEFER=0):
                    plain = _scan(cuda, w, nq, k)
            out[f"{kind} d={d} {what}"] = (nq, k, got, plain)
        _RUNS[(kind, d)] = out
    return _RUNS[(kind, d)]


def _settings_384():
    return [(nq, k, dict(CRS_WIDE_MFMA=mfma, **({"CRS_WIDE_STAGGER": 0} if stagger == "0" else {})), f"nq={nq} k'={k} mfma={mfma} stagger={stagger}")
            for nq in (256, 200) for k in (24, 32) for mfma in (16, 32) for stagger in ("default", "0")]


def _settings_256():
    return [(256, 24, dict(CRS_WIDE_MFMA=mfma), f"nq=256 k'=24 mfma={mfma}") for mfma in (16, 32)]


def _bit_for_bit(cuda, kind, d, settings):
    w = _world(cuda, kind, d)
    for what, (nq, k, got, plain) in _runs(cuda, kind, d, settings).items():
        assert np.array_equal(got[2], plain[2]), f"{what}: partial lists"
        assert np.array_equal(got[0].view(np.int32), plain[0].view(np.int32)), f"{what}: scores"
        assert np.array_equal(got[1], plain[1]), f"{what}: ids"
        s, i = got[0], got[1]
        err = float(np.abs(s - w["ref_s"][:nq, :k]).max())
        assert err <= TIGHT_TOL, (what, err)
        assert ((i >= 0) & (i < N)).all() and (np.diff(np.sort(i, axis=1), axis=1) > 0).all(), what
        if w["copies"] is not None:      # equal scores: the lowest rows, in row order
            assert i[Q_ON].tolist() == w["copies"][:k].tolist(), what
            assert len(set(s[Q_ON].view(np.int32).tolist())) == 1, what


def _oracle_ids(cuda, kind, d, settings):
    w = _world(cuda, kind, d)
    bad = []
    for what, (nq, k, got, plain) in _runs(cuda, kind, d, settings).items():
        i, ref_i = got[1], w["ref_i"][:nq, :k]
        diff = np.nonzero((i != ref_i).any(axis=1))[0]
        gap = 0.0
        for r in diff:      # the oracle's own (exact) scores of the rows that changed places
            at = np.nonzero(i[r] != ref_i[r])[0]
            f64 = lambda ids: w["c"][ids].astype(np.float64) @ w["qh"][r].astype(np.float64)
            gap = max(gap, float(np.abs(f64(i[r][at]) - f64(ref_i[r][at])).max()))
        print(f"{what}: lists differing from the oracle {diff.size} of {nq}, largest fp64 gap between swapped rows {gap:.2e}")
        if diff.size:
            bad.append((what, diff[:5].tolist()))
    assert not bad, bad[:4]


@pytest.fixture(scope="module", params=KINDS)
def kind(request):
    """module scope: pytest then runs both tests of a corpus before it builds the next one"""
    return request.param


def test_deferred_lists_are_the_undeferred_lists(cuda, kind):
    _bit_for_bit(cuda, kind, 384, _settings_384())


def test_default_lists_hold_the_oracles_ids(cuda, kind):
    _oracle_ids(cuda, kind, 384, _settings_384())


def test_deferred_lists_on_256_element_rows(cuda):
    _bit_for_bit(cuda, "random", 256, _settings_256())
    _oracle_ids(cuda, "random", 256, _settings_256())
