"""GPU: crs::maxsim_topk (csrc/maxsim_scan.hip), the exact MaxSim sweep of a token index, at op level -- bit for bit against
crs::maxsim over every row, and against the fp64 restatement of tests/_maxsim_ref.py within the bound derived there."""
import functools

import numpy as np
import pytest

import _maxsim_ref as mr

pytestmark = pytest.mark.gpu

# Items are 64 rows and windows 256 tokens, both counted from an item's first row.  Item 0: three rows that fill a window exactly;
# the short lengths and two empty rows, again 256 in all; a row that leaves room (200) and one that then straddles the window's
# end (100); a row longer than a window (300) whose tail shares a window with what follows.  Row 140 repeats row 6 (a tie).
DUP = (6, 140)
LENS = [100, 100, 56, 1, 15, 16, 17, 33, 0, 0, 174, 200, 100, 300, 7, 0, 40] + [(7 * i) % 61 for i in range(133)]
LENS[DUP[1]] = LENS[DUP[0]]
Q_LENS = (17, 0, 1, 16, 64)


@functools.lru_cache(maxsize=None)
def _case(dimp, nq, lens=tuple(LENS), seed=5, ref=True):
    """Queries of tests/_maxsim_ref.make_case (poisoned past q_len) over documents of `lens` tokens in THIS order: noise plus copies of
    query tokens at a strength drawn per document.  With `ref` also the fp64 scores and bounds of every (query, row)."""
    base = mr.make_case(seed, dimp, nq, 1, q_lens=Q_LENS, doc_lens=(1,))
    rng = np.random.default_rng(seed + 1)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat_q = np.where(np.abs(base["q16"].astype(np.float64)) > 100, 0, base["q16"].astype(np.float64)).reshape(-1, dimp)
    tok = mr._unit16(rng.standard_normal((int(offsets[-1]), dimp))).astype(np.float64)
    strength = np.repeat(rng.uniform(0.0, 2.5, len(lens)), lens)
    tok16 = mr._unit16(tok + (strength * rng.uniform(0, 1, len(tok)))[:, None] * flat_q[rng.integers(0, len(flat_q), len(tok))])
    if lens == tuple(LENS):
        tok16[offsets[DUP[1]]:offsets[DUP[1] + 1]] = tok16[offsets[DUP[0]]:offsets[DUP[0] + 1]]
    rows = np.tile(np.arange(len(lens), dtype=np.int64), (nq, 1))
    want, bound = mr.maxsim_ref(base["q16"], base["q_len"], tok16, offsets, rows) if ref else (None, None)
    return {"q16": base["q16"], "q_len": base["q_len"], "tok16": tok16, "offsets": offsets, "want": want, "bound": bound}


def _dev(cuda, case, tok16=None, q16=None):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    return (t(case["q16"] if q16 is None else q16), t(case["q_len"]), t(case["tok16"] if tok16 is None else tok16),
            len(case["tok16"]), t(case["offsets"]), len(case["offsets"]) - 1)


def _host_topk(scores, k, first, count, nonempty):
    """[(row, score)] per query: score descending, row ascending, rows without tokens left out."""
    rows = [r for r in range(first, first + count) if nonempty[r]]
    return [sorted(((r, s[r]) for r in rows), key=lambda x: (-x[1], x[0]))[:k] for s in scores]


def _check_bitwise(cuda, case, k, first=0, count=None, args=None):
    import torch
    from rag import _native as nat
    args = args or _dev(cuda, case)
    n_rows = args[5]
    count = n_rows - first if count is None else count
    nq = len(case["q_len"])
    every = torch.arange(n_rows, device=cuda).repeat(nq, 1)
    full = nat.maxsim(*args, every).cpu().numpy()
    s, r = nat.maxsim_topk(*args, k, row_first=first, row_count=count)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    nonempty = np.diff(case["offsets"]) > 0
    for q, best in enumerate(_host_topk(full, k, first, count, nonempty)):
        if case["q_len"][q] == 0:
            best = []
        assert r[q].tolist() == [x[0] for x in best] + [-1] * (k - len(best)), (q, r[q], best)
        assert s[q, :len(best)].view(np.uint32).tolist() == np.asarray([x[1] for x in best], np.float32).view(np.uint32).tolist(), q
        assert np.all(np.isneginf(s[q, len(best):]))
    return s, r


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("nq", [1, 9])
@pytest.mark.parametrize("dimp", [32, 96, 128])
def test_scan_matches_maxsim_bitwise_and_fp64(cuda, dimp, nq, k):
    case = _case(dimp, nq)
    s, r = _check_bitwise(cuda, case, k)
    skipped = 0
    for q in range(nq):
        if case["q_len"][q] == 0:
            continue
        want, bound = case["want"][q], case["bound"][q]
        live = r[q] >= 0
        assert np.all(np.abs(s[q, live] - want[r[q, live]]) <= bound[r[q, live]])
        rows = np.flatnonzero(np.diff(case["offsets"]) > 0)
        order = rows[np.argsort(-want[rows], kind="stable")]
        a, b = order[k - 1], order[k]
        if want[a] - want[b] > 2.0 * max(bound[a], bound[b]):
            assert set(r[q].tolist()) == set(order[:k].tolist()), q
        else:
            skipped += 1
            assert {a, b} == set(DUP), (q, a, b, want[a] - want[b])      # only the planted tie may sit on the cut
    print(f"maxsim_topk dimp {dimp} nq {nq} k {k}: {skipped} queries cut at the duplicate pair")


def test_k_above_the_rows_with_tokens_and_row_ranges(cuda):
    case = _case(32, 9)
    args = _dev(cuda, case)
    n_rows = args[5]
    _check_bitwise(cuda, case, 64, first=3, count=12, args=args)         # 9 rows with tokens: (-inf, -1) tails
    _check_bitwise(cuda, case, 10, first=70, count=n_rows - 70, args=args)      # starts mid-item
    _check_bitwise(cuda, case, 10, first=13, count=100, args=args)       # starts at the 300-token row, ends mid-item
    _check_bitwise(cuda, case, 5, first=20, count=0, args=args)
    _check_bitwise(cuda, case, 5, first=8, count=2, args=args)           # empty rows only


def test_many_items_per_workgroup(cuda):
    """More items than the plan starts workgroups for a query group (nq 9: 256), so a workgroup walks several and its lists and
    buffers carry across them."""
    lens = tuple((i * 5) % 4 for i in range(64 * 300 + 5))
    case = _case(32, 9, lens=lens, ref=False)
    _check_bitwise(cuda, case, 10)


def test_unread_regions_do_not_matter(cuda):
    import torch
    from rag import _native as nat
    case = _case(128, 9)
    clean = np.where(np.abs(case["q16"].astype(np.float32)) > 100, 0, case["q16"]).astype(np.float16)
    dirty_tok = np.concatenate([case["tok16"], np.full((300, 128), np.nan, np.float16)])
    a = nat.maxsim_topk(*_dev(cuda, case, q16=clean), 10)
    q, l, t, n, o, nr = _dev(cuda, case, tok16=dirty_tok)
    b = nat.maxsim_topk(q, l, t, n, o, nr, 10)                            # poisoned query rows past q_len, NaN past the last token
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))


def test_byte_offsets_past_4_gib(cuda):
    """A token buffer of just over 2^32 bytes of which only the tail is written: rows 1.. straddle and follow the 2^32-byte line."""
    import torch
    from rag import _native as nat
    line, dimp = 1 << 24, 128
    lens = [line - 20, 40, 17, 300, 1, 64]
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    small = _case(dimp, 9, lens=tuple(lens[1:]), seed=9)
    tok = torch.empty((int(offsets[-1]), dimp), dtype=torch.float16, device=cuda)
    tok[lens[0]:] = torch.from_numpy(small["tok16"]).to(cuda)
    t = lambda x: torch.from_numpy(x).to(cuda)
    s, r = nat.maxsim_topk(t(small["q16"]), t(small["q_len"]), tok, tok.shape[0], t(offsets), len(lens), 5, row_first=1)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    for q in range(9):
        if small["q_len"][q] == 0:
            assert np.all(r[q] == -1)
            continue
        want, bound = small["want"][q], small["bound"][q]
        assert sorted(r[q].tolist()) == [1, 2, 3, 4, 5]
        assert np.all(np.abs(s[q] - want[r[q] - 1]) <= bound[r[q] - 1])
        assert np.all(np.diff(s[q]) <= 0)
