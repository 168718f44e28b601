"""GPU: the late-interaction kernels at op level -- crs::maxsim (csrc/maxsim.hip) and crs::token_project (csrc/token_project.hip) --
against the fp64 restatements of tests/_maxsim_ref.py over the same fp16 / fp32 inputs, within the bounds DERIVED there (the
module docstring holds the derivation; nothing here is fitted to what the kernels return).  Each parity test prints the largest
observed error-to-bound ratio."""
import numpy as np
import pytest

import _maxsim_ref as mr

pytestmark = pytest.mark.gpu


def _dev(cuda, x, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).to(cuda)


def _maxsim(cuda, case, rows=None, q16=None, q_len=None):
    import torch
    from rag import _native as nat
    rows = case["rows"] if rows is None else rows
    q16 = case["q16"] if q16 is None else q16
    q_len = case["q_len"] if q_len is None else q_len
    tok = case["tok16"]
    tok_d = _dev(cuda, tok if tok.shape[0] else np.zeros((1, tok.shape[1]), np.float16), np.float16)
    out = nat.maxsim(_dev(cuda, q16, np.float16), _dev(cuda, q_len, np.int32), tok_d, tok.shape[0], _dev(cuda, case["offsets"], np.int64),
                     case["n_rows"], _dev(cuda, rows, np.int64))
    torch.cuda.synchronize()
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(np.shape(rows))
    return out.cpu().numpy()


def _ratio(got, want, bound):
    """Largest |error| / bound over the cells with a positive bound; cells that are exact by rule must be equal."""
    rule = bound == 0
    assert np.array_equal(got[rule].astype(np.float64), want[rule]), (got[rule], want[rule])
    if rule.all():
        return 0.0
    return float((np.abs(got[~rule].astype(np.float64) - want[~rule]) / bound[~rule]).max())


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("m_max", [1, 3, 4, 5, 64])
@pytest.mark.parametrize("dimp", [32, 96, 128])
def test_maxsim_matches_fp64(cuda, dimp, m_max, nq):
    """q_len over {0, 1, 15, 16, 17, 32, 33, 64} and document lengths over {0, 1, 15, 16, 17, 31, 33, 180, 513}: every pairing
    of them is scored (the rows of each query walk all nine documents; with m_max < 9 in several launches)."""
    worst = 0.0
    q_sets = [[ql] for ql in mr.Q_LENS] if nq == 1 else [list(mr.Q_LENS[:5]), list(mr.Q_LENS[3:])]
    for n, lens in enumerate(q_sets):
        case = mr.make_case(1000 * dimp + 10 * m_max + n, dimp, nq, m_max, q_lens=lens)
        n_docs = case["n_rows"]
        for first in range(0, n_docs, m_max):                          # every document for every query
            rows = np.stack([(np.arange(first, first + m_max) + a) % n_docs for a in range(nq)]).astype(np.int64)
            got = _maxsim(cuda, case, rows=rows)
            want, bound = mr.maxsim_ref(case["q16"], case["q_len"], case["tok16"], case["offsets"], rows)
            assert np.isfinite(got).all()
            worst = max(worst, _ratio(got, want, bound))
    print(f"maxsim dimp {dimp} m_max {m_max} nq {nq}: largest |error| / bound {worst:.3e}")
    assert worst <= 1.0, worst


def _trap_case(dimp=96):
    """Three documents of 20, 16 and 33 tokens and two queries of 9 and 17 tokens, lq_max 24."""
    case = mr.make_case(77, dimp, 2, 3, lq_max=24, q_lens=[9, 17], doc_lens=(20, 16, 33), poison_padding=False)
    lens = np.diff(case["offsets"])
    case["rows"] = np.asarray([[0, 1, 2], [2, 0, 1]], dtype=np.int64)
    return case, lens


def test_the_next_documents_first_token_is_not_seen(cuda):
    """The token right behind each document is a copy of a query token (dot product 1, above every token inside): a loop that
    runs one token too far, or masks by the group and not by the document, scores higher."""
    case, _ = _trap_case()
    off = case["offsets"]
    tok = case["tok16"].copy()
    for r in range(2):                                                 # first token of documents 1 and 2
        tok[off[r + 1]] = case["q16"][0, 3]
    case["tok16"] = tok
    want, bound = mr.maxsim_ref(case["q16"], case["q_len"], tok, off, case["rows"])
    inside = (case["q16"][0, 3].astype(np.float64) @ tok[off[0]:off[1]].astype(np.float64).T).max()
    assert inside < 0.9                                                # the planted copy would have won row 3 of query 0
    got = _maxsim(cuda, case)
    assert _ratio(got, want, bound) <= 1.0


def test_query_rows_at_and_past_q_len_are_not_seen(cuda):
    """Rows q_len.. of the query block carry 200s (and NaNs): the scores carry the bits of a block whose padding is zero."""
    case, _ = _trap_case()
    clean, dirty = case["q16"].copy(), case["q16"].copy()
    for a in range(2):
        clean[a, case["q_len"][a]:] = 0
        dirty[a, case["q_len"][a]:] = np.float16(200.0)
        dirty[a, case["q_len"][a] + 1::2] = np.float16(np.nan)
    a_, b_ = _maxsim(cuda, case, q16=clean), _maxsim(cuda, case, q16=dirty)
    assert np.isfinite(b_).all() and a_.tobytes() == b_.tobytes()
    want, bound = mr.maxsim_ref(clean, case["q_len"], case["tok16"], case["offsets"], case["rows"])
    assert _ratio(b_, want, bound) <= 1.0


def test_all_similarities_negative(cuda):
    """Every document token is minus a mix of the query's tokens plus a common direction: every dot product is negative, so a mask
    that writes 0 where it should write -inf lifts every row maximum of a ragged group to 0."""
    rng = np.random.default_rng(5)
    dimp, lq = 64, 17
    base = np.abs(rng.standard_normal(dimp)) + 0.5
    q = mr._unit16(base[None, None, :] + 0.3 * rng.uniform(0, 1, (1, lq, dimp)))
    lens = np.asarray([17, 33, 1], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    tok = mr._unit16(-(base[None, :] + 0.3 * rng.uniform(0, 1, (int(off[-1]), dimp))))
    case = {"q16": q, "q_len": np.asarray([lq], np.int32), "tok16": tok, "offsets": off, "n_rows": 3,
            "rows": np.asarray([[0, 1, 2]], dtype=np.int64)}
    want, bound = mr.maxsim_ref(q, case["q_len"], tok, off, case["rows"])
    assert (want < -0.5 * lq).all()
    got = _maxsim(cuda, case)
    assert (got < 0).all() and _ratio(got, want, bound) <= 1.0


@pytest.mark.parametrize("doc_len", [15, 16, 17, 33])
def test_maximum_at_the_documents_last_token(cuda, doc_len):
    case = mr.make_case(doc_len, 128, 1, 1, lq_max=16, q_lens=[16], doc_lens=(doc_len, 7), poison_padding=False)
    off = case["offsets"]
    r = int(np.flatnonzero(np.diff(off) == doc_len)[0])
    tok = case["tok16"].copy()
    tok[off[r + 1] - 1] = case["q16"][0, 5]                            # the last token IS query token 5: that row's maximum is 1
    case["tok16"], case["rows"] = tok, np.asarray([[r]], dtype=np.int64)
    want, bound = mr.maxsim_ref(case["q16"], case["q_len"], tok, off, case["rows"])
    best = case["q16"][0].astype(np.float64) @ tok[off[r]:off[r + 1]].astype(np.float64).T
    assert best[5].argmax() == doc_len - 1
    without = want[0, 0] - best[5].max() + best[5, :-1].max()
    assert want[0, 0] - without > 100 * bound[0, 0]                    # missing the last token is far outside the bound
    got = _maxsim(cuda, case)
    assert _ratio(got, want, bound) <= 1.0


def test_edge_rows(cuda):
    """Rows -1 and n_rows score -inf (and are never dereferenced: the offsets array ends at n_rows + 1); an empty document scores 0;
    so does an empty query -- but a bad row of an empty query is still -inf."""
    case = mr.make_case(9, 32, 2, 4, lq_max=8, q_lens=[8, 0], doc_lens=(0, 5, 19), poison_padding=True)
    empty = int(np.flatnonzero(np.diff(case["offsets"]) == 0)[0])
    full = (empty + 1) % 3
    case["rows"] = np.asarray([[-1, case["n_rows"], empty, full], [full, -1, empty, case["n_rows"] + 5]], dtype=np.int64)
    got = _maxsim(cuda, case)
    want, bound = mr.maxsim_ref(case["q16"], case["q_len"], case["tok16"], case["offsets"], case["rows"])
    assert got[0, 0] == -np.inf and got[0, 1] == -np.inf and got[0, 2] == 0 and np.isfinite(got[0, 3]) and got[0, 3] != 0
    assert got[1, 0] == 0 and got[1, 1] == -np.inf and got[1, 2] == 0 and got[1, 3] == -np.inf
    assert _ratio(got, want, bound) <= 1.0
    # offsets outside [0, n_tokens] are clamped
    wild = dict(case, offsets=np.asarray([-7, 0, 10 ** 12, 10 ** 12 + 3], dtype=np.int64), rows=np.asarray([[0, 1, 2, 1]] * 2, dtype=np.int64))
    got = _maxsim(cuda, wild)
    want, bound = mr.maxsim_ref(case["q16"], case["q_len"], case["tok16"], wild["offsets"], wild["rows"])
    assert got[0, 0] == 0 and got[0, 2] == 0 and _ratio(got, want, bound) <= 1.0


def test_a_pair_does_not_depend_on_its_launch(cuda):
    """The same (query, row) pair alone (nq 1, m_max 1, lq_max = its q_len), then at another position of a
    5 x 64 launch with lq_max 64, and of a 3 x 7 launch with lq_max = q_len + 5 (at most 64): equal bits."""
    big = mr.make_case(23, 128, 5, 64, lq_max=64, q_lens=[33, 17, 64, 1, 20])
    got = _maxsim(cuda, big)
    for a, c in ((0, 0), (1, 37), (2, 63), (4, 5)):
        lq = int(big["q_len"][a])
        alone = dict(big, q16=big["q16"][a:a + 1, :lq], q_len=big["q_len"][a:a + 1], rows=big["rows"][a:a + 1, c:c + 1])
        one = _maxsim(cuda, alone)
        assert one.tobytes() == got[a:a + 1, c:c + 1].tobytes(), (a, c, one, got[a, c])
        moved_rows = np.full((3, 7), -1, dtype=np.int64)
        moved_rows[2, 6] = big["rows"][a, c]
        q3 = np.zeros((3, min(64, lq + 5), 128), dtype=np.float16)
        q3[2, :lq] = big["q16"][a, :lq]
        moved = _maxsim(cuda, dict(big, q16=q3, q_len=np.asarray([0, 3, lq], np.int32), rows=moved_rows))
        assert moved[2:3, 6:7].tobytes() == one.tobytes()


def test_order_equals_the_fp64_order_where_the_gap_allows(cuda):
    case = mr.ordering_case()
    want, bound = mr.maxsim_ref(case["q16"], case["q_len"], case["tok16"], case["offsets"], case["rows"])
    assert mr.separated_fraction(want, bound) >= 0.9
    got = _maxsim(cuda, case).astype(np.float64)
    checked = 0
    for a in range(want.shape[0]):
        for x in range(want.shape[1]):
            for y in range(want.shape[1]):
                if want[a, x] - want[a, y] > 2.0 * max(bound[a, x], bound[a, y]):
                    assert got[a, x] > got[a, y], (a, x, y)
                    checked += 1
    assert checked >= 0.9 * 5 * 64 * 63 / 2


# ---- the projection ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dim", [32, 90, 96, 128])
@pytest.mark.parametrize("H", [64, 384, 768])
def test_token_project_matches_fp64(cuda, H, dim, with_bias):
    """n_tok 150 (three workgroups, the last one ragged, and no multiple of 16): a third of the tokens dropped (their hidden rows
    NaN), the kept ones packed in a shuffled order, one token with a zero hidden row.  dim 96 fills every row of the sixth column
    tile; dim 90 leaves W rows and bias entries 90..95 of that tile unread and has padding columns [90, 96) to check."""
    import torch
    from rag import _native as nat
    rng = np.random.default_rng(H + dim + with_bias)
    n_tok, dimp = 150, mr.dimp_of(dim)
    hidden = (rng.standard_normal((n_tok, H)) * np.exp(rng.uniform(-2, 2, (n_tok, 1)))).astype(np.float32)
    w16 = (rng.standard_normal((dim, H)) / np.sqrt(H)).astype(np.float16)
    bias = (0.1 * rng.standard_normal(dim)).astype(np.float32) if with_bias else None
    keep = rng.random(n_tok) > 0.33
    keep[[0, 63, 64, 149]] = True
    zero_tok = 64
    hidden[zero_tok] = 0.0
    dst = np.full(n_tok, -1, dtype=np.int64)
    dst[keep] = rng.permutation(int(keep.sum()))                        # packing order follows dst, not the token order
    hidden_dev = hidden.copy()
    hidden_dev[~keep] = np.nan
    slots = int(keep.sum())
    out = torch.full((slots + 2, dimp), 7.0, dtype=torch.float16, device=cuda)
    nat.token_project(_dev(cuda, hidden_dev, np.float32), _dev(cuda, w16, np.float16), None if bias is None else _dev(cuda, bias, np.float32),
                      _dev(cuda, dst, np.int64), out)
    torch.cuda.synchronize()
    got = out.cpu().numpy().astype(np.float64)
    want, bound, written = mr.project_ref(hidden, w16, bias, dst, dim)
    assert written.all() and want.shape == (slots, dimp)
    assert np.isfinite(got).all()                                       # no NaN leaked from the dropped rows
    assert (got[slots:] == 7.0).all()                                   # nothing written past the slots in use
    assert (got[:slots, dim:] == 0).all()                               # zero padding
    if not with_bias:
        assert (got[dst[zero_tok]] == 0).all()                          # v = 0 gives a zero row
    ratio = float((np.abs(got[:slots] - want) / bound).max())
    norms = np.sqrt((got[:slots] ** 2).sum(1))
    live = np.ones(slots, dtype=bool)
    if not with_bias:
        live[dst[zero_tok]] = False
    assert np.abs(norms[live] - 1).max() < 2e-3
    print(f"token_project H {H} dim {dim} bias {with_bias}: largest |error| / bound {ratio:.3e}")
    assert ratio <= 1.0, ratio
    # a token's output does not depend on what else is in the launch: token 63 alone
    one = torch.zeros((1, dimp), dtype=torch.float16, device=cuda)
    nat.token_project(_dev(cuda, hidden[63:64], np.float32), _dev(cuda, w16, np.float16), None if bias is None else _dev(cuda, bias, np.float32),
                      _dev(cuda, np.zeros(1), np.int64), one)
    assert one.cpu().numpy().tobytes() == out[dst[63]:dst[63] + 1].cpu().numpy().tobytes()


def test_limits_are_refused_before_any_launch(cuda):
    import torch
    from rag import _native as nat
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=cuda)
    with pytest.raises(nat.NativeError):                                # lq_max 65
        nat.maxsim(z((1, 65, 32), torch.float16), z(1, torch.int32), z((4, 32), torch.float16), 4, z(2, torch.int64), 1, z((1, 1), torch.int64))
    with pytest.raises(nat.NativeError):                                # dimp 48
        nat.maxsim(z((1, 8, 48), torch.float16), z(1, torch.int32), z((4, 48), torch.float16), 4, z(2, torch.int64), 1, z((1, 1), torch.int64))
    with pytest.raises(nat.NativeError):                                # hidden 48
        nat.token_project(z((4, 48), torch.float32), z((32, 48), torch.float16), None, z(4, torch.int64), z((4, 32), torch.float16))
    with pytest.raises(nat.NativeError):                                # dim 129
        nat.token_project(z((4, 64), torch.float32), z((129, 64), torch.float16), None, z(4, torch.int64), z((4, 160), torch.float16))


# ---- address arithmetic past 32 bits ---------------------------------------------------------------------------------------------
def test_token_offsets_past_2_31_and_2_32_bytes(cuda):
    """2^24 + 1061 tokens of dimp 128 (4.3 GB), filled on the device: background tokens live on coordinates [64, 128) and the queries
    on [0, 64), so every background dot product is exactly 0; the planted documents straddle the token offsets at 2^31 bytes and at
    2^32 bytes (= 2^31 elements).  The low-address control document sits at token 3000, so an offset wrapped at 2^31 or 2^32 bytes (or elements)
    lands on tokens 0..40, which are background, and scores 0 instead of the planted document's 8 to 12."""
    import torch
    from rag import _native as nat
    total = torch.cuda.get_device_properties(cuda).total_memory
    if total < 64e9:
        pytest.skip(f"device memory {total / 1e9:.0f} GB: not an MI355X")
    T, dimp = mr.HIGH_TOKENS, mr.HIGH_DIMP
    tok = torch.zeros((T, dimp), dtype=torch.float16, device=cuda)
    g = torch.Generator(device=cuda)
    g.manual_seed(mr.HIGH_SEED)
    chunk = 1 << 21
    for lo in range(0, T, chunk):
        hi = min(T, lo + chunk)
        tok[lo:hi, mr.HIGH_HEAD:] = (torch.randn((hi - lo, dimp - mr.HIGH_HEAD), generator=g, device=cuda) * 0.125).half()
    off = mr.high_offsets()
    planted = mr.high_planted()
    host = {}
    for r, x in planted.items():
        tok[int(off[r]):int(off[r + 1])] = _dev(cuda, x, np.float16)
        host[r] = x
    q16 = mr.high_queries()
    nq, lq = q16.shape[:2]
    rows = np.asarray([[1, 3, 5, 7, 0], [7, 5, 3, 1, 2], [5, 0, 7, 3, 1]], dtype=np.int64)
    out = nat.maxsim(_dev(cuda, q16, np.float16), _dev(cuda, np.full(nq, lq), np.int32), tok, T, _dev(cuda, off, np.int64), len(off) - 1,
                     _dev(cuda, rows, np.int64))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    del tok
    torch.cuda.empty_cache()
    # the fp64 expectation needs the planted tokens alone: a small CSR of the four documents
    small_off = np.zeros(len(off), dtype=np.int64)
    parts = []
    for r in range(len(off) - 1):
        n = host[r].shape[0] if r in host else 0
        small_off[r + 1] = small_off[r] + n
        if n:
            parts.append(host[r])
    want, bound = mr.maxsim_ref(q16, np.full(nq, lq), np.concatenate(parts), small_off, rows)
    back = np.isin(rows, (0, 2, 4, 6))
    assert (got[back] == 0).all()                                       # background rows: every product is exactly 0
    assert (want[~back] > 5).all()
    err = np.abs(got[~back].astype(np.float64) - want[~back])
    print(f"maxsim past 2^31 / 2^32 bytes: scores {np.round(want[0, :4], 3)}, largest |error| / bound {(err / bound[~back]).max():.3e}")
    assert (err <= bound[~back]).all(), (got, want)
