"""GPU: the fp8 token index at op level -- crs::token_project_f8 against the fp64 projection, crs::maxsim_f8 against
fp64 MaxSim over the decoded e4m3 operands (tests/_f8_ref.py), and crs::maxsim_topk_f8 bit for bit against crs::maxsim_f8."""
import functools

import numpy as np
import pytest

import _f8_ref as f8
import _maxsim_ref as mr

pytestmark = pytest.mark.gpu

Q_LENS = (1, 16, 17, 64)
DOC_LENS = (0, 1, 15, 16, 17, 33)
# the sweep: windows are 256 tokens and items 64 rows, both counted from an item's first row; 255 / 256 / 257 sit on a window's
# edge, 600 is longer than two windows; row 150 repeats row 5 (a tie)
SCAN_LENS = [255, 1, 256, 0, 257, 600, 0, 33] + [(11 * i) % 47 for i in range(192)]
DUP = (5, 150)
SCAN_LENS[DUP[1]] = SCAN_LENS[DUP[0]]
GROUP_Q = 8      # queries of a workgroup of the fp8 sweep (kMsF8GroupQ)


@functools.lru_cache(maxsize=None)
def _case(dimp, nq, lens):
    """uint8 queries (poisoned with 448 past q_len) and documents of `lens` tokens: e4m3 codes of 2^S times unit vectors that mix
    noise with copies of query tokens (scores spread out); the last 3 coordinates are padding (code 0) when dimp > 32."""
    rng = np.random.default_rng(dimp + 1000 * nq)
    dim = dimp - 3 if dimp > 32 else dimp
    unit = lambda x: x / np.maximum(np.sqrt((x * x).sum(-1, keepdims=True)), 1e-30)
    q = np.zeros((nq, 64, dimp))
    q[..., :dim] = rng.standard_normal((nq, 64, dim))
    q = unit(q)
    q_len = np.asarray([Q_LENS[i % 4] for i in range(nq)], dtype=np.int32)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n = int(offsets[-1])
    tok = np.zeros((n, dimp))
    tok[:, :dim] = rng.standard_normal((n, dim))
    strength = np.repeat(rng.uniform(0.0, 2.5, len(lens)), lens)
    tok = unit(unit(tok) + (strength * rng.uniform(0, 1, n))[:, None] * q.reshape(-1, dimp)[rng.integers(0, nq * 64, n)])
    q8, tok8 = f8.encode(q * 2.0 ** f8.S), f8.encode(tok * 2.0 ** f8.S)
    for a in range(nq):
        q8[a, q_len[a]:] = 0x7e
    if lens == tuple(SCAN_LENS):
        tok8[offsets[DUP[1]]:offsets[DUP[1] + 1]] = tok8[offsets[DUP[0]]:offsets[DUP[0] + 1]]
    return {"q8": q8, "q_len": q_len, "tok8": tok8, "offsets": offsets}


def _dev(cuda, case, offsets=None):
    import torch
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(cuda)
    off = case["offsets"] if offsets is None else offsets
    return t(case["q8"]), t(case["q_len"]), t(case["tok8"]), len(case["tok8"]), t(off), len(off) - 1


@pytest.mark.parametrize("dim", [24, 32, 64, 96, 128])
def test_projection_against_fp64(cuda, dim):
    import torch
    from rag import _native as nat
    rng = np.random.default_rng(dim)
    H, n_tok, dimp = 64, 150, mr.dimp_of(dim)
    hidden = rng.standard_normal((n_tok, H)).astype(np.float32)
    w16 = (rng.standard_normal((dim, H)) / np.sqrt(H)).astype(np.float16)
    bias = (0.1 * rng.standard_normal(dim)).astype(np.float32)
    dst = rng.permutation(n_tok).astype(np.int64)
    dst[::7] = -1
    hidden[::7] = np.nan                                      # never read
    y, bound, written = mr.project_ref(hidden, w16, bias, dst, dim)
    t = lambda x: torch.from_numpy(x).to(cuda)
    out = torch.full((n_tok, dimp), 0x55, dtype=torch.uint8, device=cuda)
    nat.token_project_f8(t(hidden), t(w16), t(bias), t(dst), out)
    out = out.cpu().numpy()
    written = np.concatenate([written, np.zeros(n_tok - len(written), dtype=bool)])
    assert np.all(out[~written] == 0x55), "a slot no token names was written"
    want = y[written[:len(y)]] * 2.0 ** f8.S
    # fp32 projection error (tests/_maxsim_ref.py, without its fp16 rounding term, plus the fp32 roundings of the two scalings),
    # then half an e4m3 step at the largest magnitude the exact value can have reached
    delta = (bound[written[:len(y)]] - 2.0 ** -11 + 4 * mr.U) * 2.0 ** f8.S
    got = f8.decode(out[written])
    err = np.abs(got - want)
    limit = delta + f8.half_step(np.abs(want) + delta)
    print(f"token_project_f8 dim {dim}: largest |error| / bound {np.max(err / limit):.3f}")
    assert np.all(err <= limit)
    assert np.all(out[written][:, dim:] == 0), "padding must be code 0"


@pytest.mark.parametrize("dimp", [32, 64, 96, 128])
def test_maxsim_f8_against_fp64(cuda, dimp):
    """The tolerance is that of an fp32 accumulation of exact products.  (A kernel on the fp8 matrix instructions misses it by up
    to 6.7 times; the decode to fp16 stays under 0.03 of it.)"""
    import torch
    from rag import _native as nat
    case = _case(dimp, 4, DOC_LENS)
    rows = np.tile(np.arange(len(DOC_LENS), dtype=np.int64), (4, 1))
    want, tol = f8.maxsim(case["q8"], case["q_len"], case["tok8"], case["offsets"], rows)
    got = nat.maxsim(*_dev(cuda, case), torch.from_numpy(rows).to(cuda)).cpu().numpy().astype(np.float64)
    live = tol > 0
    print(f"maxsim_f8 dimp {dimp}: largest |error| / tolerance {np.max(np.abs(got - want)[live] / tol[live]):.3f}")
    assert np.all(got[~live] == 0)
    assert np.all(np.abs(got - want) <= tol)


def _check_topk(cuda, case, k, first=0, count=None, offsets=None):
    import torch
    from rag import _native as nat
    args = _dev(cuda, case, offsets)
    n_rows, nq = args[5], len(case["q_len"])
    count = n_rows - first if count is None else count
    full = nat.maxsim(*args, torch.arange(n_rows, device=cuda).repeat(nq, 1)).cpu().numpy()
    s, r = nat.maxsim_topk(*args, k, row_first=first, row_count=count)
    s, r = s.cpu().numpy(), r.cpu().numpy()
    nonempty = np.diff(case["offsets"] if offsets is None else offsets) > 0
    rows = [x for x in range(first, first + count) if nonempty[x]]
    for q in range(nq):
        best = sorted(rows, key=lambda x: (-full[q, x], x))[:k] if case["q_len"][q] else []
        assert r[q].tolist() == best + [-1] * (k - len(best)), (q, r[q], best)
        assert s[q, :len(best)].view(np.uint32).tolist() == full[q, best].view(np.uint32).tolist(), q
        assert np.all(np.isneginf(s[q, len(best):]))
    return r


@pytest.mark.parametrize("k", [1, 10, 32])
@pytest.mark.parametrize("nq", [1, GROUP_Q, GROUP_Q + 1])
@pytest.mark.parametrize("dimp", [32, 64, 96, 128])
def test_topk_f8_is_maxsim_f8_bit_for_bit(cuda, dimp, nq, k):
    r = _check_topk(cuda, _case(dimp, nq, tuple(SCAN_LENS)), k)
    if k > 1:                                                 # the duplicated document: same score, the lower row first
        for q in range(nq):
            at = r[q].tolist()
            if DUP[0] in at or DUP[1] in at:
                assert DUP[1] not in at[:-1] or at.index(DUP[1]) == at.index(DUP[0]) + 1


def test_topk_f8_row_range_and_descending_offset(cuda):
    case = _case(128, GROUP_Q + 1, tuple(SCAN_LENS))
    _check_topk(cuda, case, 10, first=3, count=130)
    offsets = case["offsets"].copy()
    offsets[-1] = offsets[-2] - 5                             # the last row ends before it starts: empty, never returned
    _check_topk(cuda, case, 32, offsets=offsets)


@pytest.mark.parametrize("bad, word", [(dict(lq_max=65), "lq_max"), (dict(dimp=48), "dimp"), (dict(k=65), "k must"), (dict(nq=65536), "nq"),
                                       (dict(row_first=1), "row range"), (dict(ws_bytes=16), "workspace too small")])
def test_refusals(cuda, bad, word):
    """CRS_EINVAL with a message naming the argument, through the C ABI (the torch ops check the same limits ahead of it)."""
    import torch
    from rag import _native as nat
    lib, buf = nat.load(), torch.zeros(4096, dtype=torch.uint8, device=cuda)
    p = buf.data_ptr()
    a = dict(nq=2, lq_max=4, dimp=32, k=4, row_first=0, ws_bytes=nat.maxsim_topk_workspace_bytes(2, 4, 2, f8=True))
    assert a["ws_bytes"] <= 4096 - 1024
    a.update(bad)
    rc = lib.crs_maxsim_topk_f8(p, p, a["nq"], a["lq_max"], p, p, 2, 8, a["row_first"], 2, a["dimp"], a["k"], p + 1024, a["ws_bytes"], p, p, None)
    assert rc != 0 and word in lib.crs_last_error().decode()
    if word in ("lq_max", "dimp", "nq"):
        assert lib.crs_maxsim_f8(p, p, a["nq"], a["lq_max"], p, p, 2, 8, p, 1, a["dimp"], p, None) != 0
        assert word in lib.crs_last_error().decode()
    if word == "dimp":
        assert lib.crs_token_project_f8(p, p, None, p, p, 4, 64, 129, None) != 0 and "dim" in lib.crs_last_error().decode()
