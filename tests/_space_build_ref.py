"""The row build of the spaces 'ip' / 'l2' (csrc/slab_row.h, csrc/row_build.hip, csrc/space.hip) restated for the tests: a numpy fp32 stand-in of
slab_store_row (ip / l2) in the kernel's operation order that the CPU tests break on purpose, the assertions the GPU tests and the
CPU self-tests share, the bounds of the query conversion and of the distances, and the input rows.

A space is named 'ip' / 'l2' here (as in tests/_space_ref.py); sdim = dim, or dim + 1 for l2.  u = 2^-24, the fp32 unit roundoff.

Bounds, each derived from the arithmetic and none taken from a device result:

  t against S = sum v_i^2 (fp64, over the device's own shadow):  0 <= t, |t - S| <= (ceil(dim/64) + 7) u S
      a lane's chain is ceil(dim/64) fmas (the product is exact inside an fma: one rounding each), the xor butterfly six additions;
      all terms are non-negative, so k roundings give a relative error <= (1 + u)^k - 1 < (k + 1) u for k <= 22.

  t against the stand-in's t:  one fp32 ulp
      the stand-in's fma rounds twice (fp64, then fp32); where that differs from the device's single rounding it differs by one
      ulp of a partial sum, and the partial sums only grow.

  E against true = max_rows |stored - shadow|_2 over all sdim coordinates (fp64):  true - 2^-25 <= E <= 1.0002 true + 2^-25
      the window of _slab_ref.check_row_error: the rows have norm <= 1 as cosine rows do, so the same derivation
      holds (2^-25: the rounding of int8 * scale; 1.0002: the kernel's 1.0001 and its fp32 accumulation).

  a converted query against fp64:  ((ceil(sdim/64) + 7) / 2 + 2) u |ref| + 2^-149            (queries_tol)
  a distance against fp64:         (d + 2) u mass  [+ u |1 - s| under ip]                    (distance_tol_full)
  rows_norm_max against fp64:      ((ceil(dim/64) + 7) / 2 + 1) u, relative                  (norm_max_rel_tol)
"""
from __future__ import annotations

import numpy as np

import _slab_ref as sl
import _space_ref as sr
from _slab_ref import _fma32, _lanes, _sumsq32, _wsum32, check_padding, check_untouched, sentinel_arrays   # noqa: F401 (re-exported)
from oracle import scan_ref

SLAB_F16, SLAB_I8 = sl.SLAB_F16, sl.SLAB_I8
U = 2.0 ** -24
DIMS_IP = (1, 63, 64, 65, 100, 128, 384, 768, 1024)
# l2 puts t at a lane-0 boundary (64, 128, 384, 768), at the last lane of the last slot (1023) and across the fp16 pad (127 -> 128)
DIMS_L2 = (1, 63, 64, 127, 128, 383, 384, 768, 1023)
DIMS = {"ip": DIMS_IP, "l2": DIMS_L2}
ROW_COUNTS = (1, 5, 131)           # one wave per row, four rows per block: 5 and 131 leave a part-filled last block


def sdim_of(dim: int, space: str) -> int:
    return dim + (1 if space == "l2" else 0)


def row_mul(space: str, R: float) -> np.float32:
    """The multiplier of a caller's vector under scale R (a power of two): 1/R (ip), 1/(2R) (l2).  Exact."""
    return np.float32((0.5 if space == "l2" else 1.0) / R)


def steps(width: int) -> int:
    return -(-width // 64)


# ------------------------------------------------------------------------------------------------------------------ input rows
def make_space_rows(n: int, dim: int, R: float, seed: int):
    """n fp32 rows [n, dim] with norms below R, and their kinds.  The first six rows are one of each kind, so n = 5 still holds
    every kind but 'neg'; the rest are random.
      random     a gaussian direction, norms spread (log-uniform) over [R/8, R)
      top        norm exactly R (1 - 2^-20): m = 4^j <= min(dim, 256) coordinates of magnitude R (1 - 2^-20) / 2^j, signs alternating
      axis_last  0.9 R on coordinate dim - 1 only
      zero
      wide       element magnitudes spread over 2^14, so that the fp16 image reaches the subnormals
      neg        all negative"""
    rng = np.random.default_rng(seed)

    def random_row(norm):
        g = rng.standard_normal(dim)
        return (g * (norm / np.sqrt((g * g).sum()))).astype(np.float32)

    j = 0
    while 4 ** (j + 1) <= min(dim, 256):
        j += 1
    m = 4 ** j
    top = np.zeros(dim, np.float32)
    at = (np.arange(m) * (dim // m))
    top[at] = np.float32(R * (1.0 - 2.0 ** -20) / 2 ** j) * np.where(np.arange(m) % 2 == 0, 1.0, -1.0).astype(np.float32)
    axis = np.zeros(dim, np.float32)
    axis[dim - 1] = np.float32(0.9 * R)
    c = np.arange(dim)
    wide = (2.0 ** -(c % 15)) * rng.choice([-1.0, 1.0], dim)
    wide = (wide * (0.7 * R / np.sqrt((wide * wide).sum()))).astype(np.float32)
    neg = -np.abs(random_row(0.6 * R))
    rows = [random_row(0.97 * R), top, axis, np.zeros(dim, np.float32), wide, neg]
    kinds = ["random", "top", "axis_last", "zero", "wide", "neg"]
    while len(rows) < n:
        rows.append(random_row(R * 2.0 ** rng.uniform(-3.0, -0.002)))
        kinds.append("random")
    x = np.ascontiguousarray(np.stack(rows[:n]).astype(np.float32))
    assert np.sqrt((x.astype(np.float64) ** 2).sum(axis=1)).max() < R
    return x, kinds[:n]


# --------------------------------------------------------------------------------------- fp32 stand-in of slab_store_row (ip / l2)
MUTATIONS = ("t_without_a_lane", "t_not_in_amax", "shadow_stride_dim", "no_padding", "E_over_dim_only", "E_without_last_wave",
             "f16_truncate", "rescale_t_linear")


def store_rows_space_standin(src, dim: int, space: str, mul, pdim: int, slab_type: int, slab, scales, shadow, rows, E: float,
                             mutate: str | None = None) -> float:
    """numpy fp32 stand-in of slab_store_row (ip / l2) in the kernel's operation order.  src [n, >= dim] fp32 (the caller's vectors,
    or the shadow rows themselves for a rescale), mul an exact power of two; writes rows `rows` of slab [cap, pdim] / scales
    [cap] / shadow [cap, sdim] in place and returns the raised E.
      v = src * mul; t = the lane-strided fma chain of v^2, then the butterfly, placed at column dim under l2; amax over all sdim
      coordinates; sc = amax / 127, rint and clip for int8; fp16 by round-to-nearest-even; err over the pdim columns, times 1.0001f.
    `mutate` names one deliberate fault (MUTATIONS)."""
    assert mutate is None or mutate in MUTATIONS
    assert space in sr.SPACES
    src = np.asarray(src, np.float32)
    rows = np.asarray(rows)
    n = src.shape[0]
    sdim = sdim_of(dim, space)
    mul = np.float32(mul)
    v = (src[:, :dim] * mul).astype(np.float32)
    xp = np.zeros((n, pdim), np.float32)
    xp[:, :dim] = v
    if space == "l2":
        part = _lanes(v, dim)
        acc = np.zeros((n, 64), np.float32)
        for s in range(part.shape[1]):
            acc = _fma32(part[:, s], part[:, s], acc)
        if mutate == "t_without_a_lane":
            acc[:, (dim - 1) % 64] = 0.0           # the lane of the last element: it owns a coordinate at every dim
        t = _wsum32(acc)
        if mutate == "rescale_t_linear":           # the old t times the factor, not the sum of the rescaled squares
            t = (src[:, dim] * mul).astype(np.float32)
        xp[:, dim] = t
    if slab_type == SLAB_I8:
        over = xp[:, :dim] if mutate == "t_not_in_amax" else xp[:, :sdim]
        amax = np.abs(over).max(axis=1).astype(np.float32)
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
    if mutate == "E_over_dim_only":
        d = d.copy()
        d[:, dim:] = 0.0
    part = _lanes(d, pdim)
    acc = np.zeros((n, 64), np.float32)
    for s in range(part.shape[1]):
        acc = _fma32(part[:, s], part[:, s], acc)
    err = (np.sqrt(_wsum32(acc)).astype(np.float32) * np.float32(1.0001)).astype(np.float32)
    if mutate == "no_padding":
        slab[rows, :sdim] = stored[:, :sdim]
    else:
        slab[rows] = stored
    if mutate == "shadow_stride_dim" and space == "l2":
        flat = shadow.reshape(-1)                  # a view: shadow is contiguous
        for i, r in enumerate(rows):
            flat[int(r) * dim: int(r) * dim + sdim] = xp[i, :sdim]
    else:
        shadow[rows] = xp[:, :sdim]
    if mutate == "E_without_last_wave":
        err = err[:-1]
    return max(float(E), float(err.max())) if err.size else float(E)


def standin_norm_max(x) -> float:
    """rows_norm_max in the kernel's order: sqrt of the lane-strided fma chain and the butterfly, the largest over the rows."""
    x = np.asarray(x, np.float32)
    return float(np.sqrt(_sumsq32(x, x.shape[1])).astype(np.float32).max())


def lane0_power_of_two_row(dim: int = 384) -> np.ndarray:
    """The row whose fp32 norm rounds DOWN onto a power of two: x[0] = 2 and 2^-12 on every other coordinate of lane 0 (64, 128,
    ...).  Lane 0's chain starts at 4.0 and absorbs each 2^-24 (below half an ulp of 4.0, which is 2^-22), so the kernel's norm is
    exactly 2.0 while the true norm is 2 sqrt(1 + (dim/64 - 1) 2^-26) > 2."""
    x = np.zeros(dim, np.float32)
    x[0] = 2.0
    x[64::64] = 2.0 ** -12
    return x


# ------------------------------------------------------------------------------------------------------------------ assertions
def row_error64(slab, scales, shadow, sdim: int, slab_type: int) -> np.ndarray:
    """Per row |stored - shadow|_2 in float64 over all sdim coordinates (t included under l2)."""
    return sl.row_error64(slab, scales, shadow, sdim, slab_type)


def check_row_error_space(E: float, slab, scales, shadow, sdim: int, slab_type: int) -> float:
    """E (raised from below by the rows given) against the fp64 maximum over sdim coordinates, and against the analytic bound of
    a row of sdim coordinates and norm <= 1.  Returns the fp64 maximum."""
    from rag import _native as nat
    return sl.check_row_error(E, slab, scales, shadow, sdim, slab_type, nat.exact_row_error_bound(sdim, slab_type))


def check_build_space(x, mul, space: str, slab, scales, shadow, E: float, dim: int, pdim: int, slab_type: int) -> float:
    """The written rows (in input order) against their input x [n, dim] under the multiplier mul.  Returns the fp64 row error."""
    from rag import _native as nat
    x = np.asarray(x, np.float32)
    slab, shadow = np.asarray(slab), np.asarray(shadow)
    n, sdim = x.shape[0], sdim_of(dim, space)
    assert shadow.dtype == np.float32 and shadow.shape == (n, sdim), f"shadow shape {shadow.shape}, expected {(n, sdim)}"
    assert np.isfinite(shadow).all(), "non-finite value in the shadow"
    # a power-of-two multiply is exact: the shadow holds fl32(x * mul) bit for bit
    want = (x * np.float32(mul)).astype(np.float32)
    assert np.array_equal(shadow[:, :dim].view(np.uint32), want.view(np.uint32)), "shadow[:, :dim] is not x * mul bit for bit"
    if space == "l2":
        t = shadow[:, dim]
        S = (shadow[:, :dim].astype(np.float64) ** 2).sum(axis=1)
        assert (t >= 0).all(), "t is negative"
        off = np.abs(t.astype(np.float64) - S)
        bad = off > (steps(dim) + 7) * U * S
        assert not bad.any(), f"t of row {np.flatnonzero(bad)[0]} is off by {off[bad][0]:.3e} (sum {S[bad][0]:.3e})"
        mine = _sumsq32(shadow[:, :dim], dim)
        ulp = np.spacing(np.maximum(np.abs(mine), np.abs(t)).astype(np.float32)).astype(np.float64)
        assert (np.abs(t.astype(np.float64) - mine.astype(np.float64)) <= ulp).all(), "t is more than one ulp from the fixed order's sum"
    # the stored row is the DEVICE shadow quantised, bit for bit, t included
    sl.check_stored(slab, scales, shadow, sdim, slab_type)
    check_padding(slab, sdim, pdim, slab_type)
    assert pdim == nat.padded_dim(sdim, slab_type)
    return check_row_error_space(E, slab, scales, shadow, sdim, slab_type)


def check_rescaled(before_shadow, after_shadow, space: str, shift: int) -> None:
    """The rescale assertion: the shadow after a rescale by 2^shift is rescale_rows of the shadow before it, bit for bit -- every
    coordinate times 2^-shift and t times 2^-2 shift exactly."""
    want = sr.rescale_rows(np.asarray(before_shadow, np.float32), space, shift)
    assert np.array_equal(np.asarray(after_shadow).view(np.uint32), want.view(np.uint32)), "the rescaled shadow is not the old one times 2^-shift (t: 2^-2 shift)"


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


# ---------------------------------------------------------------------------------------------------------------------- bounds
def queries_tol(ref64, sdim: int) -> np.ndarray:
    """Bound on |converted query - fp64| per coordinate.  The sum of squares is ceil(dim/64) fmas and six butterfly additions of
    non-negative terms, and under l2 the addition of 1: relative error <= (ceil(sdim/64) + 7) u.  The square root halves it and
    rounds once, the division rounds once more (q * (1/R) is exact): ((ceil(sdim/64) + 7) / 2 + 2) u |ref|.  2^-149: a result in
    the subnormals."""
    return ((steps(sdim) + 7) / 2.0 + 2.0) * U * np.abs(np.asarray(ref64, np.float64)) + 2.0 ** -149


def norm_max_rel_tol(dim: int) -> float:
    """rows_norm_max: the sum of squares as above ((ceil(dim/64) + 7) u covers its ceil(dim/64) + 6 roundings), halved by the
    square root, which rounds once."""
    return ((steps(dim) + 7) / 2.0 + 1.0) * U


def distance_tol_full(q32_row, x32, space: str) -> np.ndarray:
    """_space_ref.distance_tol plus, under ip, the rounding of the final 1 - s: u |1 - s|.
    distance_tol is (d + 2) u mass, mass = sum |q_i x_i| (ip) or sum (q_i - x_i)^2 (l2).  The kernel's sum is ceil(d/64) fmas
    and at most six inexact butterfly additions; under l2 each difference rounds once before it is squared (2 u of its square),
    and x = shadow * back is exact: at most ceil(d/64) + 8 <= d + 2 roundings of the mass for d >= 7, and for d < 7 only
    ceil(log2 d) butterfly additions have two non-zero operands (1 + ceil(log2 d) + 2 <= d + 2).  Without the 1 - s term the
    bound is 0 for a zero row (distance exactly 1) and too small for a short one."""
    tol = sr.distance_tol(q32_row, x32, space)
    if space == "ip":
        tol = tol + U * np.abs(sr.metric64_rows(q32_row, x32, "ip"))
    return tol
