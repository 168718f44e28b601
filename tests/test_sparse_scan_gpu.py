"""GPU: the impact scan (csrc/sparse_scan.hip, crs::sparse_topk) against tests/_sparse_ref.py.

Every product and every sum is rounded to fp32 on its own and a row's terms are added in ascending token id, so the kernel is a
pure function of its inputs: scores are compared as int32 words and rows with ==."""
import numpy as np
import pytest

import _sparse_ref as ref

pytestmark = pytest.mark.gpu

VOCAB = 3000
CHUNK_TOKENS = 2048          # kChunk of csrc/csr_scan.h: one row of the corpus is longer


def _corpus(n_rows, seed=7):
    """Sparse rows over 3000 ids: Zipf-like ids with random positive weights, 5 % empty rows, a whole empty tile (rows 64..127 when
    there are that many), one row of 2500 ids (longer than a staged chunk), and ten exact copies of one row (equal scores)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    rows = []
    for r in range(n_rows):
        if (n_rows > 1 and rng.random() < 0.05) or (n_rows >= 192 and 64 <= r < 128):
            rows.append((np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32)))
            continue
        ids = np.unique(rng.choice(VOCAB, size=int(rng.integers(2, 90)), p=p)).astype(np.int32)
        rows.append((ids, (rng.random(ids.size) * 2.5 + 0.01).astype(np.float32)))
    if n_rows >= 40:
        ids = np.sort(rng.choice(VOCAB, size=2500, replace=False)).astype(np.int32)
        rows[n_rows // 5] = (ids, (rng.random(2500) + 0.01).astype(np.float32))
        dup = (np.array([5, 17, 2990, 2995], dtype=np.int32), np.array([0.5, 1.25, 2.0, 0.75], dtype=np.float32))
        for r in rng.choice(np.arange(n_rows // 2, n_rows), size=10, replace=False).tolist():
            rows[r] = dup
    return rows


def _queries(n, seed=3):
    """n queries of 1..40 ids; query 1 has no terms, query 2 one id no row holds (2999 is never drawn into a row: see _case), query 3
    (n >= 4) exactly the duplicate rows' ids."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, VOCAB + 1)
    p /= p.sum()
    out = []
    for _ in range(n):
        ids = np.unique(rng.choice(VOCAB - 1, size=int(rng.integers(1, 41)), p=p[:-1] / p[:-1].sum())).astype(np.int32)
        out.append((ids, (rng.random(ids.size) * 2 + 0.01).astype(np.float32)))
    if n > 1:
        out[1] = (np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32))
    if n > 2:
        out[2] = (np.array([2999], dtype=np.int32), np.array([1.0], dtype=np.float32))
    if n > 3:
        out[3] = (np.array([5, 17, 2990, 2995], dtype=np.int32), np.array([1.0, 1.0, 1.0, 1.0], dtype=np.float32))
    return out


_CACHE = {}


def _case(n_rows):
    if n_rows not in _CACHE:
        rows = _corpus(n_rows)
        rows = [(i[i != 2999], w[i != 2999]) for i, w in rows]          # id 2999 is in no row
        off, tok, w = ref.csr_of(rows)
        q_off, q_tok, q_w = ref.csr_of(_queries(64))
        scored = [ref.sparse_scores_ref(off, tok, w, n_rows, q_tok[q_off[q]:q_off[q + 1]], q_w[q_off[q]:q_off[q + 1]]) for q in range(64)]
        _CACHE[n_rows] = dict(csr=(off, tok, w), q=(q_off, q_tok, q_w), scored=scored, want={})
    return _CACHE[n_rows]


def _want(case, k):
    if k not in case["want"]:
        lists = [ref.topk_of(s, h, k) for s, h in case["scored"]]
        case["want"][k] = np.stack([s for s, _ in lists]), np.stack([r for _, r in lists])
    return case["want"][k]


def _run(cuda, csr, n_rows, q, k):
    import torch
    from rag import _native as nat
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)          # noqa: E731
    s, r = nat.sparse_topk(dev(csr[0]), dev(csr[1]), dev(csr[2]), n_rows, dev(q[0]), dev(q[1]), dev(q[2]), k)
    torch.cuda.synchronize()
    return s.cpu().numpy(), r.cpu().numpy()


def _assert_bits(got, want, what):
    (got_s, got_r), (want_s, want_r) = got, want
    assert got_s.dtype == np.float32 and got_r.dtype == np.int64 and got_s.shape == want_s.shape and got_r.shape == want_r.shape, what
    bad = np.argwhere(got_r != want_r)
    assert bad.size == 0, f"{what}: rows differ first at {bad[0].tolist()}: {got_r[tuple(bad[0])]} != {want_r[tuple(bad[0])]}"
    bad = np.argwhere(got_s.view(np.int32) != want_s.view(np.int32))
    assert bad.size == 0, f"{what}: scores differ in their bits first at {bad[0].tolist()}: {got_s[tuple(bad[0])]!r} != {want_s[tuple(bad[0])]!r}"


def _prefix(q, nq):
    q_off, q_tok, q_w = q
    return q_off[: nq + 1], q_tok[: q_off[nq]], q_w[: q_off[nq]]


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 257])
def test_op_matches_the_fp32_reference_bit_for_bit(cuda, n_rows):
    """n_rows x nq in {1, 64} x k in {1, 10, 64}: fewer rows than a tile, ragged last tiles, 257 rows = a second workgroup; empty
    rows, a whole empty tile (257), a row spanning two staged chunks, ten exact duplicates, a query with no terms and one whose only
    term no row holds."""
    case = _case(n_rows)
    off, tok, w = case["csr"]
    if n_rows == 257:
        assert (np.diff(off) > CHUNK_TOKENS).sum() == 1 and (np.diff(off)[64:128] == 0).all()
    for nq, k in ((1, 1), (1, 10), (1, 64), (64, 1), (64, 10), (64, 64)):
        want_s, want_r = _want(case, k)
        _assert_bits(_run(cuda, case["csr"], n_rows, _prefix(case["q"], nq), k), (want_s[:nq], want_r[:nq]), f"n_rows={n_rows} nq={nq} k={k}")
    want_s, want_r = _want(case, 64)
    assert (want_r[1] == -1).all() and (want_r[2] == -1).all() and np.isneginf(want_s[2]).all()
    if n_rows == 257:
        top = want_r[3][:10]
        assert len(set(want_s[3][:10].tolist())) == 1 and (np.diff(top) > 0).all()       # the duplicates tie: lower row first
        s, h = ref.sparse_scores_scalar(off, tok, w, n_rows, *[a[case["q"][0][3]:case["q"][0][4]] for a in case["q"][1:]])
        assert (s.view(np.int32) == case["scored"][3][0].view(np.int32)).all() and (h == case["scored"][3][1]).all()


def test_the_pair_cap(cuda):
    """Exactly 4096 (query, token) pairs in one launch, and 4097 refused with CRS_EINVAL before anything runs."""
    from rag import _native as nat
    case = _case(257)
    rng = np.random.default_rng(12)
    queries = [(np.sort(rng.choice(VOCAB - 1, size=64, replace=False)).astype(np.int32), (rng.random(64) + 0.1).astype(np.float32)) for _ in range(64)]
    q = ref.csr_of(queries)
    assert q[1].size == nat.BM25_MAX_PAIRS == 4096
    want = ref.sparse_topk_ref(*case["csr"], 257, *q, 10)
    _assert_bits(_run(cuda, case["csr"], 257, q, 10), want, "4096 pairs")
    ids, w = queries[63]
    queries[63] = (np.r_[ids, VOCAB - 1].astype(np.int32), np.r_[w, 1.0].astype(np.float32))
    with pytest.raises(nat.NativeError, match="CRS_BM25_MAX_PAIRS"):
        _run(cuda, case["csr"], 257, ref.csr_of(queries), 10)


def test_offsets_out_of_range_are_clamped(cuda):
    """A malformed CSR gives the scores of the clamped one, never an access outside the buffers: lo into [0, total], hi into
    [lo, total].  The token and weight arrays sit in the middle of larger allocations whose surroundings hold an id every query
    asks for with a huge weight, so a read outside would show in the scores; the outputs are framed by canaries."""
    import torch
    from rag import _native as nat
    rng = np.random.default_rng(5)
    n_rows, total = 70, 600
    tok = np.sort(rng.choice(VOCAB, size=(n_rows, 9), replace=True), axis=1).astype(np.int32).reshape(-1)[:total]
    w = (rng.random(total) + 0.1).astype(np.float32)
    off = (np.arange(n_rows + 1) * 8).astype(np.int64)
    off[3], off[10], off[11], off[40], off[70] = -50, 10 ** 12, -(10 ** 12), 2 ** 31 + 7, 2 ** 40
    bait = 77
    q = ref.csr_of([(np.array([bait], dtype=np.int32), np.array([1.0], dtype=np.float32)),
                    (np.unique(tok[::5]).astype(np.int32), np.ones(np.unique(tok[::5]).size, dtype=np.float32))])
    pad = 4096
    tok_buf = torch.full((total + 2 * pad,), bait, dtype=torch.int32, device=cuda)
    w_buf = torch.full((total + 2 * pad,), 1e30, dtype=torch.float32, device=cuda)
    tok_buf[pad: pad + total] = torch.from_numpy(np.where(tok == bait, bait + 1, tok).astype(np.int32)).to(cuda)
    w_buf[pad: pad + total] = torch.from_numpy(w).to(cuda)
    tok_in = np.where(tok == bait, bait + 1, tok).astype(np.int32)
    k = 10
    out_s = torch.full((2 * k + 32,), 123.0, dtype=torch.float32, device=cuda)
    out_r = torch.full((2 * k + 32,), 123, dtype=torch.int64, device=cuda)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)          # noqa: E731
    nat.sparse_topk(dev(off), tok_buf[pad: pad + total], w_buf[pad: pad + total], n_rows, dev(q[0]), dev(q[1]), dev(q[2]), k,
                    out_scores=out_s[16: 16 + 2 * k].view(2, k), out_rows=out_r[16: 16 + 2 * k].view(2, k))
    torch.cuda.synchronize()
    assert (out_s[:16] == 123).all() and (out_s[16 + 2 * k:] == 123).all() and (out_r[:16] == 123).all() and (out_r[16 + 2 * k:] == 123).all()
    got = out_s[16: 16 + 2 * k].view(2, k).cpu().numpy(), out_r[16: 16 + 2 * k].view(2, k).cpu().numpy()
    want = ref.sparse_topk_ref(off, tok_in, w, n_rows, *q, k, scalar=True)
    _assert_bits(got, want, "clamped offsets")
    assert (got[1][0] == -1).all()                     # the bait id is only outside the arrays: no hit
    assert np.isfinite(got[0][1][got[1][1] >= 0]).all() and (got[0][1][got[1][1] >= 0] < 1e3).all()
