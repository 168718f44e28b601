"""fp64 reference, data builders and shared assertions of the near-duplicate join tests (csrc/join.hip).

The truth is the fp32 shadow: the pair set of a threshold t is {i < j : <c_i, c_j> >= t} over the shadow rows, dotted in fp64.  The
two-stage join (fp16 slab scores at t - eps, fp32 check at t) is restated in numpy (two_stage) so that the assertions the GPU tests
apply to the kernels can be shown to reject broken variants on the CPU (tests/test_dedup_cpu.py).
"""
from __future__ import annotations

import numpy as np

from oracle import scan_ref

TILE = 256                     # CRS_PAIRS_TILE
COSINES = (0.999, 0.99, 0.97, 0.95, 0.90, 0.80)
THRESHOLDS = (0.5, 0.93, 0.985)
U24 = 2.0 ** -24


# ------------------------------------------------------------------------------------------------------------ the bound
def epsilon64(E: float, pdim: int, *, drop_E2: bool = False, drop_arith: bool = False) -> float:
    """eps = (2 E + E^2)(1 + 1e-4) + (1.5 pdim + 8) 2^-23, restated (the keyword arguments build the broken variants)."""
    E = float(E)
    rows = 2.0 * E + (0.0 if drop_E2 else E * E)
    return rows * (1.0 + 1e-4) + (0.0 if drop_arith else (1.5 * pdim + 8.0) * 2.0 ** -23)


def check_epsilon(eps: float, E: float, pdim: int) -> None:
    want = epsilon64(E, pdim)
    assert abs(eps - want) <= 1e-12 * want, f"epsilon {eps!r} is not the formula's {want!r} (E = {E!r}, pdim = {pdim})"


def padded(dim: int) -> int:
    return -(-dim // 128) * 128


# ------------------------------------------------------------------------------------------------------------ data
def _unit(x):
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def _at_cosine(x, cos, rng):
    """Unit rows at the given cosines to the unit rows x (fp64); dimension 1 has no orthogonal direction: the copy is x itself."""
    g = rng.standard_normal(x.shape)
    g -= (g * x).sum(axis=1, keepdims=True) * x
    nrm = np.sqrt((g * g).sum(axis=1, keepdims=True))
    u = np.divide(g, nrm, out=np.zeros_like(g), where=nrm > 1e-9)
    c = np.asarray(cos, dtype=np.float64)[:, None]
    return _unit(c * x + np.sqrt(np.maximum(1.0 - c * c, 0.0)) * u)


def planted_rows(n: int, dim: int, seed: int = 0, extras: bool = False) -> np.ndarray:
    """fp32 [n (+ 2), dim]: the first max(1, 2n // 3) rows are random directions, row base + r is a copy of row r at the target
    cosine COSINES[r % 6] (n = 300: rows 200-299 copy rows 0-99).  extras: + one exact copy (of row base // 2) and one negated copy
    (of row base // 2 + 1, or of row 0)."""
    rng = np.random.default_rng(1000 * dim + n + seed)
    base = max(1, 2 * n // 3)
    x = _unit(rng.standard_normal((base, dim)))
    m = n - base
    rows = [x]
    if m:
        rows.append(_at_cosine(x[:m], [COSINES[r % len(COSINES)] for r in range(m)], rng))
    if extras:
        rows.append(x[base // 2][None])
        rows.append(-x[(base // 2 + 1) % base][None])
    return np.ascontiguousarray(np.concatenate(rows).astype(np.float32))


def band_rows(t: float, half_width: float, dim: int = 64, n_pairs: int = 1024, seed: int = 7):
    """(fp32 [2 n_pairs, dim], planted pairs int64 [n_pairs, 2]): row n_pairs + r is at a cosine uniform in [t - half_width,
    t + half_width] to row r; every other pair is two random directions."""
    rng = np.random.default_rng(seed)
    x = _unit(rng.standard_normal((n_pairs, dim)))
    cos = t + half_width * (2.0 * rng.random(n_pairs) - 1.0)
    y = _at_cosine(x, cos, rng)
    planted = np.stack([np.arange(n_pairs), n_pairs + np.arange(n_pairs)], axis=1).astype(np.int64)
    return np.ascontiguousarray(np.concatenate([x, y]).astype(np.float32)), planted


def build_standin(x: np.ndarray):
    """The slab build restated: (shadow fp32 [n, dim] unit rows, slab fp16 [n, pdim] zero padded, E = the largest
    |stored row - shadow row|_2)."""
    shadow = scan_ref.l2_normalize_rows(x)
    n, dim = shadow.shape
    slab = np.zeros((n, padded(dim)), dtype=np.float16)
    slab[:, :dim] = scan_ref.quantize_rows_f16(shadow)
    return shadow, slab, row_error_max(slab, shadow)


def row_error_max(slab, shadow) -> float:
    d = slab[:, : shadow.shape[1]].astype(np.float64) - shadow.astype(np.float64)
    return float(np.sqrt((d * d).sum(axis=1)).max()) if len(d) else 0.0


# ------------------------------------------------------------------------------------------------------------ fp64 truth
def gram64(rows) -> np.ndarray:
    r = np.asarray(rows, dtype=np.float64)
    return r @ r.T


def _range_mask(n: int, a_range, b_range) -> np.ndarray:
    i = np.arange(n)
    in_a = (i >= a_range[0]) & (i < a_range[0] + a_range[1])
    in_b = (i >= b_range[0]) & (i < b_range[0] + b_range[1])
    return in_a[:, None] & in_b[None, :] & (i[:, None] < i[None, :])


def pairs_where(mask) -> set:
    a, b = np.nonzero(mask)
    return set(zip(a.tolist(), b.tolist()))


def pair_set64(G, t: float, a_range=None, b_range=None) -> set:
    """{(i, j) : i in A, j in B, i < j, G[i, j] >= t}: the brute-force answer."""
    n = G.shape[0]
    return pairs_where(_range_mask(n, a_range or (0, n), b_range or (0, n)) & (G >= t))


def keep_first64(n: int, pairs) -> np.ndarray:
    """The keep-first rule, row by row: j is dropped iff some kept i < j pairs with it; its entry is the smallest such i."""
    partners = {}
    for a, b in pairs:
        partners.setdefault(b, []).append(a)
    dup = np.full(n, -1, dtype=np.int64)
    for j in range(n):
        kept = [i for i in sorted(partners.get(j, ())) if dup[i] < 0]
        if kept:
            dup[j] = kept[0]
    return dup


# ------------------------------------------------------------------------------------------------------------ the stand-in
def stage1_standin(slab, a_range, b_range, thr: float, cap: int, mutate: str | None = None):
    """crs_pairs_above_f16 in numpy: (pairs int64 [min(count, cap), 2], scores fp32, count).  mutate: 'i_ge_j' lists i >= j too,
    'drop_ragged' ignores the rows of the last, partial tile of either range."""
    S = gram64(slab).astype(np.float32)            # fp16 products are exact; the sum is rounded once here, 1.5 pdim times there
    n = S.shape[0]
    if mutate == "drop_ragged":
        a_range = (a_range[0], a_range[1] // TILE * TILE)
        b_range = (b_range[0], b_range[1] // TILE * TILE)
    mask = _range_mask(n, a_range, b_range)
    if mutate == "i_ge_j":
        i = np.arange(n)
        mask = ((i >= a_range[0]) & (i < sum(a_range)))[:, None] & ((i >= b_range[0]) & (i < sum(b_range)))[None, :]
    a, b = np.nonzero(mask & (S >= np.float32(thr)))
    pairs = np.stack([a, b], axis=1).astype(np.int64)
    return pairs[:cap], S[a, b][:cap], int(len(a))


def sim32_standin(shadow, pairs) -> np.ndarray:
    """crs_pairs_verify_f32's dot: lane l of 16 chains fmaf over coordinates l, l + 16, ...; xor butterfly 8, 4, 2, 1."""
    x = shadow[pairs[:, 0]].astype(np.float32)
    y = shadow[pairs[:, 1]].astype(np.float32)
    m, d = x.shape
    steps = -(-d // 16)
    xp = np.zeros((m, steps * 16), np.float32); xp[:, :d] = x
    yp = np.zeros((m, steps * 16), np.float32); yp[:, :d] = y
    acc = np.zeros((m, 16), np.float32)
    for s in range(steps):                          # (a padded coordinate adds fmaf(0, 0, acc) = acc: the kernel skips it)
        acc = (xp[:, 16 * s: 16 * s + 16].astype(np.float64) * yp[:, 16 * s: 16 * s + 16].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    for o in (8, 4, 2, 1):
        acc = (acc + acc[:, np.arange(16) ^ o]).astype(np.float32)
    return acc[:, 0]


def two_stage(x, t: float, a_range=None, b_range=None, mutate: str | None = None):
    """near_duplicates restated: build, stage 1 at t - eps, stage 2 at t -> dict like the store's (+ E, pdim).
    mutate: 'slab_at_t' thresholds the slab score at t and skips the check; 'i_ge_j', 'drop_ragged' (stage 1); 'no_E2' /
    'no_arith' leave that term out of eps."""
    shadow, slab, E = build_standin(x)
    n, pdim = slab.shape
    a_range, b_range = a_range or (0, n), b_range or (0, n)
    eps = epsilon64(E, pdim, drop_E2=mutate == "no_E2", drop_arith=mutate == "no_arith")
    if mutate == "slab_at_t":
        pairs, scores, count = stage1_standin(slab, a_range, b_range, t, n * n)
        sims, keep = scores, np.ones(len(pairs), bool)
    else:
        pairs, scores, count = stage1_standin(slab, a_range, b_range, t - eps, n * n, mutate)
        sims = sim32_standin(shadow, pairs) if len(pairs) else np.zeros(0, np.float32)
        keep = sims >= t
    a, b, s = pairs[keep, 0], pairs[keep, 1], sims[keep]
    order = np.lexsort((b, a))
    return {"rows_a": a[order], "rows_b": b[order], "similarities": s[order], "candidates": count, "epsilon": eps,
            "E": E, "pdim": pdim, "shadow": shadow, "slab": slab}


# ------------------------------------------------------------------------------------------------------------ assertions
def check_no_pair_near(G, thresholds, eps: float, a_range=None, b_range=None) -> None:
    """The precondition of an exact-set test: no pair of the ranges lies within eps of a threshold (fp64)."""
    n = G.shape[0]
    vals = G[_range_mask(n, a_range or (0, n), b_range or (0, n))]
    for t in thresholds:
        close = int((np.abs(vals - t) <= eps).sum())
        assert close == 0, f"{close} pairs lie within {eps:.3g} of threshold {t}: the data does not separate"


def check_sorted_pairs(rows_a, rows_b) -> None:
    a, b = np.asarray(rows_a), np.asarray(rows_b)
    assert a.dtype == np.int64 and b.dtype == np.int64 and a.shape == b.shape and a.ndim == 1
    assert np.all(a < b), "a pair with i >= j"
    key = list(zip(a.tolist(), b.tolist()))
    assert key == sorted(key), "pairs are not sorted by (a, b)"
    assert len(set(key)) == len(key), "a pair is listed twice"


def check_exact_set(res, shadow, t: float, a_range=None, b_range=None, G=None) -> None:
    """The answer is exactly the fp64 pair set of the shadow rows, sorted, each similarity within 2 d 2^-24 of the fp64 dot."""
    G = gram64(shadow) if G is None else G
    check_sorted_pairs(res["rows_a"], res["rows_b"])
    got = set(zip(res["rows_a"].tolist(), res["rows_b"].tolist()))
    want = pair_set64(G, t, a_range, b_range)
    assert got == want, f"threshold {t}: {len(want - got)} pairs missing (e.g. {sorted(want - got)[:3]}), {len(got - want)} too many (e.g. {sorted(got - want)[:3]})"
    sims = np.asarray(res["similarities"])
    assert sims.dtype == np.float32 and sims.shape == res["rows_a"].shape
    if len(sims):
        dev = np.abs(sims.astype(np.float64) - G[res["rows_a"], res["rows_b"]]).max()
        assert dev <= 2.0 * shadow.shape[1] * U24, f"a similarity is {dev:.3g} from the fp64 dot"


def check_stage1(pairs, scores, count: int, cap: int, slab, shadow, t: float, eps: float, thr1: float, a_range=None, b_range=None) -> None:
    """Stage 1 at thr1 <= t - eps with room for everything (cap >= count): a superset of the fp64 set at t, every candidate's
    slab score within eps of the fp64 dot of the shadow rows, each pair once, and exactly the pairs whose slab score is >= thr1 up
    to the accumulation term."""
    n, pdim = slab.shape
    assert count <= cap and len(pairs) == count
    key = list(map(tuple, np.asarray(pairs).tolist()))
    assert len(set(key)) == count, "a candidate is listed twice"
    got = set(key)
    mask = _range_mask(n, a_range or (0, n), b_range or (0, n))
    assert all(mask[a, b] for a, b in got), "a candidate outside the ranges, or with i >= j"
    G = gram64(shadow)
    missing = pair_set64(G, t, a_range, b_range) - got
    assert not missing, f"stage 1 misses {len(missing)} pairs of the fp64 set, e.g. {sorted(missing)[:3]}"
    S = gram64(slab)
    arith = (1.5 * pdim + 8.0) * 2.0 ** -23
    assert pairs_where(mask & (S >= thr1 + arith)) <= got <= pairs_where(mask & (S >= thr1 - arith)), "candidates are not the pairs above thr1"
    if count:
        p = np.asarray(pairs)
        assert np.abs(np.asarray(scores, dtype=np.float64) - S[p[:, 0], p[:, 1]]).max() <= arith, "a score is not the slab score"
        assert np.abs(np.asarray(scores, dtype=np.float64) - G[p[:, 0], p[:, 1]]).max() <= eps, "a slab score is further than eps from fp64"


def check_band(res, shadow, t: float, planted, max_excluded: float = 0.05) -> int:
    """Band data: pairs within delta = 2 d 2^-24 of t are left out (at most 5 % of the planted pairs); every other pair i < j must
    be classified as fp64 classifies it.  Returns the number left out."""
    G = gram64(shadow)
    n, d = shadow.shape
    delta = 2.0 * d * U24
    out = pairs_where(_range_mask(n, (0, n), (0, n)) & (np.abs(G - t) <= delta))
    assert len(out) <= max_excluded * len(planted), f"{len(out)} pairs within delta of t: more than {max_excluded:.0%} of the planted ones"
    check_sorted_pairs(res["rows_a"], res["rows_b"])
    got = set(zip(res["rows_a"].tolist(), res["rows_b"].tolist())) - out
    want = pair_set64(G, t) - out
    assert got == want, f"{len(want - got)} pairs missing, {len(got - want)} wrongly listed outside the delta band"
    return len(out)
