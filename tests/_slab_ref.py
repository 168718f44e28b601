"""fp64 restatement of the slab build (csrc/slab_row.h) and of the certificate's eps_q (csrc/tail_steps.h), the assertions the
GPU tests and the CPU self-tests share, and a numpy fp32 stand-in of slab_store_row that the CPU tests break on purpose.

Plain numpy; the only project import is oracle.scan_ref.  Sizes that the library decides (the padded row length, the analytic
row-error bound) are passed in by the caller.

Bounds used by the checks, u = 2^-24 (fp32 unit roundoff):

  shadow element against normalise64(x):  (dim/64 + 8) u |ref| + 2^-149
      the kernel sums x^2 with one FMA per element, <= dim/64 per lane, then 6 butterfly additions, all terms non-negative:
      relative error <= (dim/64 + 6) u; the square root halves it, (dim/128 + 3) u; the square root and the division round once
      each: (dim/128 + 5) u.  2^-149 is half the smallest fp32 subnormal spacing's worth of absolute slack for results there.
      A row scaled by a constant in fp32 (x' = fl(s x), each element off by <= u relative) normalises to within 2 u of its twin,
      (dim/128 + 7) u in all, so a scaled row is held to the SAME bound against its UNSCALED twin's reference.

  E against true = max_j |stored_j - shadow_j|_2 (fp64):  true - 2^-25 <= E <= 1.0002 true + 2^-25
      2^-25: the one rounding of int8 * scale (<= 1 in magnitude for a unit row); 1.0002 covers the kernel's 1.0001 factor and its
      fp32 accumulation ((pdim/64 + 6) u / 2 < 2e-6).
"""
from __future__ import annotations

import numpy as np

from oracle import scan_ref

SLAB_F16, SLAB_I8 = 0, 1
U = 2.0 ** -24
DIMS = (1, 3, 63, 64, 65, 100, 128, 384, 768, 1000, 1024)
ROW_COUNTS = (1, 5, 1027)          # one wave per row, four rows per block: 5 and 1027 leave a partly filled last block
SENTINEL_BYTE = 0x5A


def expected_pdim(dim: int, slab_type: int) -> int:
    g = 256 if slab_type == SLAB_I8 else 128
    return -(-dim // g) * g


# ----------------------------------------------------------------------------------------------------------- the fp64 reference
def normalise64(x) -> np.ndarray:
    """x / max(|x|_2, 1e-12) per row, everything in float64."""
    x = np.asarray(x).astype(np.float64)
    nrm = np.sqrt((x * x).sum(axis=-1, keepdims=True))
    return x / np.maximum(nrm, 1e-12)


def stored64(slab, scales, dim: int, slab_type: int) -> np.ndarray:
    """The rows as the scan sees them, float64 [n, dim]: float64(fp16), or int8 * float64(scale)."""
    s = np.asarray(slab)[:, :dim].astype(np.float64)
    if slab_type == SLAB_I8:
        s = s * np.asarray(scales).astype(np.float64)[:, None]
    return s


def row_error64(slab, scales, shadow, dim: int, slab_type: int) -> np.ndarray:
    """Per row |stored - shadow|_2 in float64 over columns [0, dim)."""
    d = stored64(slab, scales, dim, slab_type) - np.asarray(shadow)[:, :dim].astype(np.float64)
    return np.sqrt((d * d).sum(axis=1))


def eps_formula64(q32, q16, dim: int, pdim: int, is_i8: bool, E: float, *, drop_wave=None, fixed_point: bool = True) -> np.ndarray:
    """eps_q = dq (1 + E) + |q|_2 E + (1.5 pdim + 8) 2^-23 per query, in float64, without the kernel's 1.0001 factors.
    dq = |q16 - q32|_2 over pdim (q32 = 0 past dim), + sqrt(pdim) max|q16| / 65024 on int8 slabs.
    drop_wave / fixed_point=False are the MUTATIONS the CPU self-test uses: the kernel's 256 threads stride the padded row, so
    wave w owns the elements e with (e % 256) // 64 == w; drop_wave leaves that wave's partial sums and maximum out."""
    q32 = np.asarray(q32).astype(np.float64)
    h = np.asarray(q16).astype(np.float64)
    nq = q32.shape[0]
    assert h.shape == (nq, pdim) and q32.shape[1] == dim
    x = np.zeros((nq, pdim))
    x[:, :dim] = q32
    keep = np.ones(pdim)
    if drop_wave is not None:
        keep[(np.arange(pdim) % 256) // 64 == drop_wave] = 0.0
    dq = np.sqrt((((h - x) ** 2) * keep).sum(axis=1))
    qn = np.sqrt(((x * x) * keep).sum(axis=1))
    if is_i8 and fixed_point:
        dq = dq + np.sqrt(float(pdim)) * (np.abs(h) * keep).max(axis=1) / 65024.0
    return dq * (1.0 + float(E)) + qn * float(E) + (1.5 * pdim + 8.0) * 2.0 ** -23


def slab_deviation64(q32, q16, slab, scales, shadow, slab_type: int) -> np.ndarray:
    """Per query max over ALL rows of |slab_score - s32|, both dots in float64.  q16 [nq, pdim], slab [n, pdim], shadow [n, dim]."""
    shadow = np.asarray(shadow).astype(np.float64)
    dim = shadow.shape[1]
    s32 = np.asarray(q32).astype(np.float64) @ shadow.T
    if slab_type == SLAB_I8:
        qd = scan_ref.dequantized_queries(np.asarray(q16))
        ss = (qd @ np.asarray(slab).astype(np.float64).T) * np.asarray(scales).astype(np.float64)[None, :]
    else:
        ss = np.asarray(q16).astype(np.float64) @ np.asarray(slab).astype(np.float64).T
    return np.abs(ss - s32).max(axis=1)


# ------------------------------------------------------------------------------------------------------------------ input rows
def make_rows(n: int, dim: int, seed: int):
    """n input rows [n, dim] fp32 of every kind the kernel must survive, their kind names, and twin[i] = the index of the unscaled
    row a scaled row repeats (-1 otherwise).  The first five rows are gaussian, zero, wide, tiny and one-hot, so n = 5 still
    holds the edge kinds; from row 9 on come triplets (gaussian, the same x 1e-6, the same x 1e+6)."""
    rng = np.random.default_rng(seed)
    c = np.arange(dim)
    g0 = rng.standard_normal(dim).astype(np.float32)
    wide = (2.0 ** -(c % 27)).astype(np.float32)
    onehot = np.zeros(dim, np.float32)
    onehot[dim - 1] = 2.5
    rows = [g0, np.zeros(dim, np.float32), wide, np.full(dim, 1e-15, np.float32), onehot, np.full(dim, 0.37, np.float32),
            (wide * rng.choice([-1.0, 1.0], dim)).astype(np.float32), g0 * np.float32(1e-6), g0 * np.float32(1e6)]
    kinds = ["gauss", "zero", "wide", "tiny", "onehot", "const", "wide", "gauss*1e-6", "gauss*1e+6"]
    twin = [-1, -1, -1, -1, -1, -1, -1, 0, 0]
    while len(rows) < n:
        g = rng.standard_normal(dim).astype(np.float32)
        base = len(rows)
        rows += [g, g * np.float32(1e-6), g * np.float32(1e6)]
        kinds += ["gauss", "gauss*1e-6", "gauss*1e+6"]
        twin += [-1, base, base]
    x = np.ascontiguousarray(np.stack(rows[:n]).astype(np.float32))
    twin = np.asarray(twin[:n])
    return x, kinds[:n], twin


# ------------------------------------------------------------------------------------------------------------------ assertions
def check_shadow(shadow, x, kinds, twin, dim: int) -> None:
    """B.1: the written shadow rows [n, dim] against normalise64 of the input (of the unscaled twin for a scaled row)."""
    shadow = np.asarray(shadow)
    assert shadow.dtype == np.float32 and shadow.shape == (x.shape[0], dim)
    assert np.isfinite(shadow).all(), "non-finite value in the shadow"
    src = np.where(twin[:, None] >= 0, x[np.maximum(twin, 0)], x)
    ref = normalise64(src)
    err = np.abs(shadow.astype(np.float64) - ref)
    tol = (dim / 64.0 + 8.0) * U * np.abs(ref) + 2.0 ** -149
    bad = err > tol
    if bad.any():
        r, col = np.argwhere(bad)[0]
        raise AssertionError(f"shadow[{r}, {col}] ({kinds[r]}) = {shadow[r, col]!r}, fp64 {ref[r, col]!r}: off by {err[r, col]:.3e} > {tol[r, col]:.3e}")
    for r, k in enumerate(kinds):
        if k == "zero":
            assert (shadow[r].view(np.uint32) << 1 == 0).all(), "the zero row must stay zero"
        if k == "tiny":   # norm below 1e-12: the row is x / 1e-12, not a unit vector
            assert np.allclose(shadow[r].astype(np.float64), x[r].astype(np.float64) / 1e-12, rtol=4 * U, atol=0)


def check_stored(slab, scales, shadow, dim: int, slab_type: int) -> None:
    """B.2: the stored rows are the DEVICE shadow quantised, bit for bit."""
    slab, shadow = np.asarray(slab), np.asarray(shadow)
    if slab_type == SLAB_I8:
        assert slab.dtype == np.int8
        q, sc = scan_ref.quantize_rows_i8(shadow)
        assert np.array_equal(np.asarray(scales).view(np.uint32), sc.view(np.uint32)), "int8 scales differ from max|shadow| / 127"
        assert np.array_equal(slab[:, :dim], q), "int8 rows differ from rint(shadow / scale)"
    else:
        assert slab.dtype == np.float16
        want = scan_ref.quantize_rows_f16(shadow)
        assert np.array_equal(slab[:, :dim].view(np.int16), want.view(np.int16)), "fp16 rows differ from round-to-nearest-even of the shadow"


def check_padding(slab, dim: int, pdim: int, slab_type: int) -> None:
    """B.3: columns [dim, pdim) of every written row are +0 bits; pdim is the library's padded row length."""
    slab = np.asarray(slab)
    assert pdim == expected_pdim(dim, slab_type) and slab.shape[1] == pdim
    pad = slab[:, dim:]
    bits = pad.view(np.int16) if slab_type == SLAB_F16 else pad
    assert not bits.any(), "padding columns are not +0"


def check_untouched(before, after, written_rows) -> None:
    """B.4: every row outside written_rows has the bits it had before the call (the sentinel)."""
    for name, (b, a) in {"slab": (before[0], after[0]), "scales": (before[1], after[1]), "shadow": (before[2], after[2])}.items():
        if b is None or a is None:
            continue
        b, a = np.asarray(b), np.asarray(a)
        keep = np.ones(b.shape[0], bool)
        keep[np.asarray(written_rows)] = False
        bb = b[keep].reshape(int(keep.sum()), -1).view(np.uint8)
        aa = a[keep].reshape(int(keep.sum()), -1).view(np.uint8)
        assert np.array_equal(bb, aa), f"{name}: a row outside the written ones changed"


def check_row_error(E: float, slab, scales, shadow, dim: int, slab_type: int, analytic_bound: float) -> float:
    """B.5: E (raised from zero by the rows given) against the fp64 maximum, and against the analytic bound.  Returns true."""
    true = float(row_error64(slab, scales, shadow, dim, slab_type).max())
    E = float(E)
    assert true - 2.0 ** -25 <= E <= 1.0002 * true + 2.0 ** -25, f"E = {E!r}, fp64 max row error {true!r}"
    assert E <= analytic_bound, f"E = {E!r} above the analytic bound {analytic_bound!r}"
    return true


def check_build(x, kinds, twin, slab, scales, shadow, E, dim: int, pdim: int, slab_type: int, analytic_bound: float) -> float:
    """B.1-3 and 5 on the written rows (in input order)."""
    check_shadow(shadow, x, kinds, twin, dim)
    check_stored(slab, scales, shadow, dim, slab_type)
    check_padding(slab, dim, pdim, slab_type)
    return check_row_error(E, slab, scales, shadow, dim, slab_type, analytic_bound)


def sentinel_arrays(cap: int, dim: int, pdim: int, slab_type: int):
    """Host copies of the sentinel-filled arrays: slab bytes 0x5a, scales and shadow NaN."""
    if slab_type == SLAB_I8:
        slab = np.full((cap, pdim), SENTINEL_BYTE, np.int8)
    else:
        slab = np.full((cap, pdim), SENTINEL_BYTE * 257, np.int16).view(np.float16)
    return slab, np.full(cap, np.nan, np.float32), np.full((cap, dim), np.nan, np.float32)


# ------------------------------------------------------------------------------------------- fp32 stand-in of slab_store_row
def _fma32(a, b, c):
    """fl32(a * b + c): the product of two fp32 is exact in fp64 (the sum is then rounded twice, which the checks tolerate)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _lanes(v, width: int):
    """[n, width] -> [n, steps, 64], zero padded: lane l owns the elements l, l + 64, ..."""
    steps = -(-width // 64)
    out = np.zeros((v.shape[0], steps * 64), np.float32)
    out[:, :width] = v
    return out.reshape(v.shape[0], steps, 64)


def _wsum32(p):
    """The wave64 xor butterfly in fp32 ([n, 64] -> [n])."""
    p = p.astype(np.float32)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        p = (p + p[:, lane ^ o]).astype(np.float32)
    return p[:, 0]


def _sumsq32(v, width: int):
    t = _lanes(v, width)
    acc = np.zeros((v.shape[0], 64), np.float32)
    for s in range(t.shape[1]):
        acc = _fma32(t[:, s], t[:, s], acc)
    return _wsum32(acc)


MUTATIONS = ("scale_unnormalised", "norm_over_pdim", "no_padding", "E_without_last_wave", "E_mean", "f16_truncate")


def store_rows_standin(src, dim: int, pdim: int, slab_type: int, slab, scales, shadow, rows, E: float, mutate: str | None = None) -> float:
    """numpy fp32 stand-in of slab_store_row in the kernel's operation order: lane-strided FMA partial sums, a 6-level pairwise
    reduction, fp32 square root and division.  src [n, >= dim] fp32 (a row may be longer than dim: the kernel must not read
    past dim); writes rows `rows` of slab / scales / shadow in place and returns the raised E.  `mutate` names one deliberate
    fault (MUTATIONS)."""
    assert mutate is None or mutate in MUTATIONS
    src = np.asarray(src, np.float32)
    rows = np.asarray(rows)
    n = src.shape[0]
    nw = pdim if mutate == "norm_over_pdim" else dim
    ss = _sumsq32(src[:, :nw], nw)
    den = np.maximum(np.sqrt(ss).astype(np.float32), np.float32(1e-12))
    x = (src[:, :dim] / den[:, None]).astype(np.float32)
    xp = np.zeros((n, pdim), np.float32)
    xp[:, :dim] = x
    if slab_type == SLAB_I8:
        amax = np.abs(src[:, :dim] if mutate == "scale_unnormalised" else x).max(axis=1).astype(np.float32)
        sc = (amax / np.float32(127.0)).astype(np.float32)
        safe = np.where(sc > 0, sc, np.float32(1.0)).astype(np.float32)
        qv = np.clip(np.rint((xp / safe[:, None]).astype(np.float32)), -127, 127).astype(np.float32)
        stored = qv.astype(np.int8)
        d = _fma32(-qv, np.broadcast_to(sc[:, None], qv.shape), xp)
        scales[rows] = sc
    else:
        h = xp.astype(np.float16)
        if mutate == "f16_truncate":
            over = np.abs(h.astype(np.float32)) > np.abs(xp)
            h = np.where(over, np.nextafter(h, np.float16(0)), h).astype(np.float16)
        stored = h
        d = (xp - h.astype(np.float32)).astype(np.float32)
    t = _lanes(d, pdim)
    acc = np.zeros((n, 64), np.float32)
    for s in range(t.shape[1]):
        acc = _fma32(t[:, s], t[:, s], acc)
    err = (np.sqrt(_wsum32(acc)).astype(np.float32) * np.float32(1.0001)).astype(np.float32)
    if mutate == "no_padding":
        slab[rows, :dim] = stored[:, :dim]
    else:
        slab[rows] = stored
    shadow[rows] = x
    if mutate == "E_without_last_wave":
        err = err[:-1]
    if mutate == "E_mean":
        return max(float(E), float(err.mean(dtype=np.float32))) if err.size else float(E)
    return max(float(E), float(err.max())) if err.size else float(E)


# ------------------------------------------------------------------------------------------------- the certificate's test cases
CERT_ROWS, CERT_NQ, CERT_K_IN, CERT_K_OUT = 2000, 32, 16, 10
CERT_DIMS = (100, 384, 768, 1024)
CERT_BETAS = (0.01, 0.1, 0.3, 1.0)


def cert_corpus(dim: int) -> np.ndarray:
    return scan_ref.synth_corpus(CERT_ROWS, dim, seed=700 + dim)


def cert_queries(dim: int, stored, shadow) -> np.ndarray:
    """CERT_NQ fp32 queries: half random unit vectors, half adversarial normalise(c_j + beta (c^_j - c_j) / |c^_j - c_j|) -- leaning
    into row j's quantisation error, where Cauchy-Schwarz is tightest.  stored: the rows as float64, shadow: the fp32 rows."""
    rng = np.random.default_rng(900 + dim)
    half = CERT_NQ // 2
    q = np.empty((CERT_NQ, dim))
    q[:half] = rng.standard_normal((half, dim))
    js = rng.choice(CERT_ROWS, CERT_NQ - half, replace=False)
    for i, j in enumerate(js):
        c = np.asarray(shadow[j]).astype(np.float64)
        e = np.asarray(stored[j]).astype(np.float64) - c
        nrm = np.sqrt((e * e).sum())
        assert nrm > 0
        q[half + i] = c + CERT_BETAS[i % len(CERT_BETAS)] * e / nrm
    return np.ascontiguousarray(normalise64(q).astype(np.float32))


def eps_window(formula):
    """C: the window eps_meas must fall into.  1.0004 covers the kernel's three safety factors (1.0001^2 on dq, 1.0002 on |q| E);
    3 * 2^-24 is the fp32 resolution of t and of the two additions of the comparison at magnitudes <= 1."""
    formula = np.asarray(formula, np.float64)
    return formula - 3 * U, 1.0004 * formula + 3 * U
