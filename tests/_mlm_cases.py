"""The case table of the SPLADE head's shape tests (csrc/mlm_pool.hip): plain numpy, no device, no tests here.  Shared by
tests/test_mlm_cases_cpu.py, which proves the table's coverage claims on the fp64 references, and tests/test_mlm_pool_shapes_gpu.py,
which runs the cases.

  head               the seeded weights of a head (w_t ~ 1 / sqrt(H)), as tests/test_mlm_pool_gpu.py has always drawn them.
  xform_case(H)      one case per mlm_transform_kernel<NJ>: 3 texts of 23 positions, lens (23, 1, 9) -- 69 tokens in one row tile and
                     four transform workgroups: rows 0..31 hold a whole text, the next one's only token and padding; 32..63 padding
                     on both sides of a text's nine tokens; 64..95 padding, then rows past the last token; 96..127 are wholly past
                     it (the last two take the path without a matrix product, which stores zeros).  V = 130 in rows of 133: two
                     column tiles, the second with two live columns.  H / 64 steps of the projection's K loop.
  teeth_case(H)      the input of test_the_transform_tolerance_tells_erf_gelu_from_tanh_gelu (5 x 48 tokens at scale 1.5) at H.
  long_case(seq)     H = 64, four texts longer than a wave's 64 rows or the 128-row tile, lens (seq, 1, inner, seq), V = 128 k + 10.
  group_case(b, s)   H = 64, V = 300: 16, 17 and 33 row tiles, that is one, two and three groups of kMlmGroupM row tiles.
  clamp_case()       lens above seq and below 0.
  blocks / uncovered / pooled_without   the coverage condition of the long cases and the faults the bounds must catch.
"""
import numpy as np

import _sparse_ref as ref

HIDDEN = (64, 128, 256, 384, 512, 768, 1024)      # make_mlm_plan's list (csrc/mlm_plan.cpp); NJ = H / 64
TILE_M, TILE_N, TILE_K = 128, ref.TILE_N, 64       # csrc/mlm_plan.h
WAVE_ROWS, BLOCK_ROWS, XFORM_ROWS, GROUP_M = 64, 16, 32, 16
NAN32 = 0x7FC5A5A5                                 # the NaN pattern of padding positions (tests/_row_ref.py)
FILL = -7.5                                        # what test_mlm_pool_gpu._run leaves in the cells the kernels must not write


def head(V, Hd, seed):
    rng = np.random.default_rng(seed)
    w_t = (rng.standard_normal((Hd, Hd)) / np.sqrt(Hd)).astype(np.float16)
    w_d = (rng.standard_normal((V, Hd)) * 0.05).astype(np.float16)
    return dict(w_t=w_t, b_t=(rng.standard_normal(Hd) * 0.1).astype(np.float32), gamma=(1.0 + 0.1 * rng.standard_normal(Hd)).astype(np.float32),
                beta=(0.1 * rng.standard_normal(Hd)).astype(np.float32), eps=1e-12, w_d=w_d,
                bias=(rng.standard_normal(V) * 0.2 - 0.1).astype(np.float32))


def clamped(lens, seq):
    return np.clip(np.asarray(lens, dtype=np.int64), 0, seq)


def nan_padding(hidden, lens):
    """a copy of hidden [batch, seq, H] with the NaN pattern at every position at or past its text's (clamped) length"""
    out = np.array(hidden, dtype=np.float32)
    for b, n in enumerate(clamped(lens, out.shape[1])):
        out[b, n:].view(np.int32)[...] = NAN32
    return out


def _case(hd, hidden, lens, pad=3):
    lens = np.asarray(lens, dtype=np.int32)
    return dict(head=hd, hidden=nan_padding(hidden, lens), lens=lens, vp=hd["w_d"].shape[0] + pad)


# ---- every transform instantiation ------------------------------------------------------------------------------------------------------
XFORM_BATCH, XFORM_SEQ, XFORM_LENS, XFORM_V = 3, 23, (23, 1, 9), 130


def xform_case(H):
    rng = np.random.default_rng(7000 + H)
    return _case(head(XFORM_V, H, seed=H), rng.standard_normal((XFORM_BATCH, XFORM_SEQ, H)), XFORM_LENS)


def teeth_case(H):
    rng = np.random.default_rng(21)
    return _case(head(16, H, seed=11), rng.standard_normal((5, 48, H)) * 1.5, np.full(5, 48), pad=0)


def real_rows(case):
    """(h16 fp64 [n, H], flat token rows [n]) of a case's real tokens, in row order: what the transform kernel multiplies"""
    batch, seq, H = case["hidden"].shape
    live = (np.arange(seq)[None, :] < clamped(case["lens"], seq)[:, None]).reshape(-1)
    rows = np.flatnonzero(live)
    return ref.f16(case["hidden"].reshape(-1, H)[rows]), rows


def transform_bound(case):
    """(ref, bound16, second-order fraction, rows) of a case's real tokens: _sparse_ref.transform_ref_and_bound"""
    hd = case["head"]
    h16, rows = real_rows(case)
    return ref.transform_ref_and_bound(h16, hd["w_t"], hd["b_t"], hd["gamma"], hd["beta"], hd["eps"]) + (rows,)


def tanh_transform(case):
    """the transform of a case's real tokens in fp64 with the tanh form of GELU: what the bound must tell from the erf form"""
    hd = case["head"]
    h16, _ = real_rows(case)
    x = h16 @ hd["w_t"].astype(np.float64).T + hd["b_t"]
    g = 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    return (g - g.mean(-1, keepdims=True)) / np.sqrt(g.var(-1, keepdims=True) + hd["eps"]) * hd["gamma"] + hd["beta"]


# ---- texts longer than a wave span and a tile -------------------------------------------------------------------------------------------
LONG_INNER = {65: 64, 100: 63, 128: 127, 129: 128, 200: 129, 300: 65}      # seq -> the length of text 2
LONG_K = {65: 1, 100: 1, 128: 1, 129: 1, 200: 1, 300: 1}                    # V = 128 k + 10: the smallest k that covers every block
LONG_SEQS = tuple(LONG_INNER)
POSITION_SEQ = 200


def long_lens(seq):
    return (seq, 1, LONG_INNER[seq], seq)


def long_case(seq, k=None):
    V = TILE_N * (LONG_K[seq] if k is None else k) + 10
    rng = np.random.default_rng(3000 + seq)
    return _case(head(V, 64, seed=seq), rng.standard_normal((4, seq, 64)), long_lens(seq))


def position_case():
    """(a batch of four texts of 200 positions, the probe text [200, 64] that takes each of its rows in turn)"""
    case = long_case(POSITION_SEQ)
    probe = np.random.default_rng(99).standard_normal((POSITION_SEQ, 64)).astype(np.float32)
    return case, probe


# ---- more than one group of row tiles ---------------------------------------------------------------------------------------------------
GROUP_V = 300
GROUP_CASES = ((16, 128), (17, 128), (35, 61), (33, 128), (41, 100))         # (batch, seq)


def group_case(batch, seq):
    """lens mixed, never 0 (every row tile holds a real token, so that a tile the remap drops is missed); the first and the last
    text are full: the last rows of the ragged last tile are live."""
    rng = np.random.default_rng(100 * batch + seq)
    lens = rng.integers(1, seq + 1, size=batch)
    lens[0], lens[1], lens[-1] = seq, 1, seq
    return _case(head(GROUP_V, 64, seed=1000 * batch + seq), rng.standard_normal((batch, seq, 64)), lens)


def geometry(batch, seq, V):
    """(grid_m, grid_n, pool_grid, xform_grid) as make_mlm_plan gives them, restated"""
    grid_m, grid_n = -(-batch * seq // TILE_M), -(-V // TILE_N)
    return grid_m, grid_n, grid_m * grid_n, grid_m * TILE_M // XFORM_ROWS


# ---- the lens clamp ---------------------------------------------------------------------------------------------------------------------
CLAMP_SEQ, CLAMP_LENS, CLAMP_MEANS = 48, (53, -3, 0, 48, 7), (48, 0, 0, 48, 7)


def clamp_case():
    """(hidden with NaN at the padding positions of the clamped lens, head): run with CLAMP_LENS and with CLAMP_MEANS"""
    rng = np.random.default_rng(55)
    hidden = nan_padding(rng.standard_normal((len(CLAMP_LENS), CLAMP_SEQ, 64)), CLAMP_LENS)
    return hidden, head(TILE_N + 1, 64, seed=5)


# ---- the coverage condition and the faults ----------------------------------------------------------------------------------------------
def transform_of(case):
    """t fp64 [batch, seq, H] from transform_ref on the fp16-rounded hidden states; zeros at the padding positions"""
    hd = case["head"]
    batch, seq, H = case["hidden"].shape
    t = np.zeros((batch, seq, H))
    for b, n in enumerate(clamped(case["lens"], seq)):
        t[b, :n] = ref.transform_ref(ref.f16(case["hidden"][b, :n]), hd["w_t"], hd["b_t"], hd["gamma"], hd["beta"], hd["eps"])
    return t


def pooled_without(t, case, drop=None, rows=BLOCK_ROWS):
    """(weights fp64 [batch, V], bound [batch, V]): pool_ref and pool_bound of t [batch, seq, H]; with drop = k, the token rows
    [rows k, rows (k + 1)) of the flattened batch are left out of every maximum, as an epilogue that skips a 16-row block or a
    remap that drops a 128-row tile would leave them out.  The bound is that of the unfaulted result."""
    hd = case["head"]
    batch, seq, H = t.shape
    lens = clamped(case["lens"], seq)
    want, absdot = ref.pool_ref(t, lens, hd["w_d"], hd["bias"])
    bound = ref.pool_bound(absdot, want, H)
    if drop is None:
        return want, bound
    out = want.copy()
    w64, bias = hd["w_d"].astype(np.float64), hd["bias"].astype(np.float64)
    for b in range(batch):
        tok = b * seq + np.arange(lens[b])
        hit = tok // rows == drop
        if hit.any():
            kept = t[b, : lens[b]][~hit]
            out[b] = np.log1p(np.maximum((kept @ w64.T + bias).max(0), 0.0)) if len(kept) else 0.0
    return out, bound


def blocks(lens, seq, rows=BLOCK_ROWS):
    """the indices k of the `rows`-row blocks of the flattened batch that hold a real token"""
    out = set()
    for b, n in enumerate(clamped(lens, seq)):
        out.update(((b * seq + np.arange(n)) // rows).tolist())
    return sorted(out)


def uncovered(t, case, margin):
    """The (text, 16-row block) pairs with real tokens for which NO column has all of: its maximum over the text inside the block;
    that maximum positive; the runner-up outside the block lower by more than margin x the column's pool_bound -- taken on the
    weights, behind max(0, .) and log1p, which is no weaker than on the logits (log1p is 1-Lipschitz there).  Empty: an epilogue that
    skips or mis-bounds any block of any text moves a compared cell by more than margin x its bound."""
    hd = case["head"]
    batch, seq, H = t.shape
    lens = clamped(case["lens"], seq)
    want, absdot = ref.pool_ref(t, lens, hd["w_d"], hd["bias"])
    bound = ref.pool_bound(absdot, want, H)
    w64, bias = hd["w_d"].astype(np.float64), hd["bias"].astype(np.float64)
    missing = []
    for b in range(batch):
        n = int(lens[b])
        logits = t[b, :n] @ w64.T + bias
        blk = (b * seq + np.arange(n)) // BLOCK_ROWS
        for k in np.unique(blk):
            inside = blk == k
            top = logits[inside].max(0)
            rest = np.log1p(np.maximum(logits[~inside].max(0), 0.0)) if (~inside).any() else np.zeros_like(top)
            ok = (top > 0) & (np.log1p(np.maximum(top, 0.0)) - rest > margin * bound[b])
            if not ok.any():
                missing.append((b, int(k)))
    return missing
