"""CPU: the assertions of the ip / l2 row-build tests (tests/_space_build_ref.py) can fail.

A numpy fp32 stand-in of slab_store_row (ip / l2) passes the assertions the GPU tests apply to the kernels, eight deliberately broken
stand-ins each fail one, a stand-in rescale equals a stand-in append under the grown scale bit for bit, and the row whose fp32 norm
rounds down onto a power of two is pinned without a GPU.
"""
import numpy as np
import pytest

import _space_build_ref as ref
import _space_ref as sr
from rag import _native as nat

F16, I8 = ref.SLAB_F16, ref.SLAB_I8
TYPES = [F16, I8]
IDS = {F16: "f16", I8: "i8"}.get
CASES = [(space, dim) for space in sr.SPACES for dim in ref.DIMS[space]]
REJECTED_BY = {}


def rejects(name):
    """Registers the test that shows a mutation's rejection (test_every_mutation_has_a_rejection_test)."""
    def mark(fn):
        REJECTED_BY.setdefault(name, []).append(fn.__name__)
        return fn
    return mark


def _arrays(cap, dim, space, st):
    sdim = ref.sdim_of(dim, space)
    pdim = nat.padded_dim(sdim, st)
    return ref.sentinel_arrays(cap, sdim, pdim, st), sdim, pdim


def _build(n, dim, space, st, R=2.0, mutate=None, x=None, seed=5):
    """Append n rows at row0 = 4 of sentinel arrays of n + 9 rows with the stand-in, as the GPU test does with the kernel."""
    (slab, scales, shadow), sdim, pdim = _arrays(n + 9, dim, space, st)
    if x is None:
        x, _ = ref.make_space_rows(n, dim, R, seed)
    before = (slab.copy(), scales.copy(), shadow.copy())
    rows = np.arange(4, 4 + n)
    mul = ref.row_mul(space, R)
    E = ref.store_rows_space_standin(x, dim, space, mul, pdim, st, slab, scales, shadow, rows, 0.0, mutate)
    return dict(x=x, mul=mul, space=space, slab=slab, scales=scales, shadow=shadow, E=E, before=before, rows=rows, dim=dim, sdim=sdim,
                pdim=pdim, st=st)


def _check_all(b):
    r = b["rows"]
    ref.check_build_space(b["x"], b["mul"], b["space"], b["slab"][r], b["scales"][r], b["shadow"][r], b["E"], b["dim"], b["pdim"], b["st"])
    ref.check_untouched(b["before"], (b["slab"], b["scales"] if b["st"] == I8 else None, b["shadow"]), r)


def _must_fail(b):
    with pytest.raises(AssertionError):
        _check_all(b)


# ------------------------------------------------------------------------------------------------------ the stand-in passes
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", CASES)
def test_standin_passes_the_kernels_assertions(space, dim, st):
    for n, R in ((5, 2.0), (43, 2.0 ** -10), (43, 2.0 ** 12)):
        _check_all(_build(n, dim, space, st, R))


def test_input_rows_hold_every_kind_inside_the_scale():
    for dim in (1, 63, 384, 1024):
        for R in (2.0 ** -10, 2.0, 2.0 ** 12):
            x, kinds = ref.make_space_rows(131, dim, R, seed=dim)
            assert kinds[:6] == ["random", "top", "axis_last", "zero", "wide", "neg"] and set(kinds[6:]) == {"random"}
            norms = np.sqrt((x.astype(np.float64) ** 2).sum(axis=1))
            assert norms.max() < R and norms[1] == R * (1 - 2.0 ** -20) and norms[3] == 0
            rnd = norms[[i for i, k in enumerate(kinds) if k == "random"]]
            assert rnd.min() >= R / 8 * (1 - 1e-6) and rnd.max() / rnd.min() > 4
            assert x[2, dim - 1] == np.float32(0.9 * R) and np.count_nonzero(x[2]) == 1
            assert (x[5] <= 0).all()
            if dim >= 63:        # the fp16 image of the scaled row reaches the subnormals (below 2^-14)
                w = np.abs(x[4].astype(np.float64)) / R
                assert w.max() / w.min() == 2.0 ** 14 and w.min() < 2.0 ** -14


# ---------------------------------------------------------------------------------------------------- broken stand-ins fail
@rejects("t_without_a_lane")
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 64, 127, 384, 1023])
def test_t_without_a_lane_fails(dim, st):
    _must_fail(_build(12, dim, "l2", st, mutate="t_without_a_lane"))


@rejects("t_not_in_amax")
@pytest.mark.parametrize("dim", [64, 128, 384, 1023])
def test_int8_scale_without_t_fails(dim):
    # t = |v|^2 exceeds every |v_i| once the mass is spread over enough coordinates: the first row has norm 0.97 R
    b = _build(12, dim, "l2", I8, mutate="t_not_in_amax")
    assert b["shadow"][4, dim] > np.abs(b["shadow"][4, :dim]).max()
    _must_fail(b)


@rejects("shadow_stride_dim")
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 64, 127, 1023])
def test_l2_shadow_with_stride_dim_fails(dim, st):
    _must_fail(_build(12, dim, "l2", st, mutate="shadow_stride_dim"))


@rejects("no_padding")
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", [("ip", 1), ("ip", 100), ("ip", 65), ("l2", 63), ("l2", 128), ("l2", 1023)])
def test_unwritten_padding_fails(space, dim, st):
    b = _build(12, dim, space, st, mutate="no_padding")
    if b["pdim"] == b["sdim"]:           # l2 1023 -> 1024 columns: no padding to leave out
        _check_all(b)
    else:
        _must_fail(b)


@rejects("E_over_dim_only")
@pytest.mark.parametrize("st,dim", [(F16, 1), (F16, 64), (F16, 127), (F16, 384), (F16, 1023), (I8, 1), (I8, 3)])
def test_E_without_the_error_of_t_fails(dim, st):
    """One row on one axis: v = 0.45 is an fp16 number at dim 1 .. 1023 only up to its own rounding, t = fl(v^2) carries an
    error of its own.  On int8 rows t's error vanishes where t is the row's largest coordinate (it quantises to 127 exactly), so
    the int8 cases are the low dimensions, where |v| > t."""
    x = np.zeros((1, dim), np.float32)
    x[0, dim - 1] = 1.8
    b = _build(1, dim, "l2", st, mutate="E_over_dim_only", x=x)
    r = b["rows"]
    with pytest.raises(AssertionError):
        ref.check_row_error_space(b["E"], b["slab"][r], b["scales"][r], b["shadow"][r], b["sdim"], st)
    _check_all(_build(1, dim, "l2", st, x=x))
    # and a whole batch: the maximum over rows is under-reported too
    _must_fail(_build(43, dim, "l2", st, mutate="E_over_dim_only"))


@rejects("E_without_last_wave")
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", [("ip", 63), ("ip", 100), ("ip", 1024), ("l2", 1), ("l2", 127), ("l2", 1023)])
def test_E_without_the_last_wave_fails(space, dim, st):
    # n = 5: the last row is alone in the second block.  Order the batch so that this row carries the maximum.
    # (not ip at dim 1: an int8 row of one coordinate is 127 * scale, without error)
    good = _build(5, dim, space, st)
    r = good["rows"]
    worst = int(np.argmax(ref.row_error64(good["slab"][r], good["scales"][r], good["shadow"][r], good["sdim"], st)))
    order = [i for i in range(5) if i != worst] + [worst]
    x = np.ascontiguousarray(good["x"][order])
    b = _build(5, dim, space, st, mutate="E_without_last_wave", x=x)
    with pytest.raises(AssertionError):
        ref.check_row_error_space(b["E"], b["slab"][r], b["scales"][r], b["shadow"][r], b["sdim"], st)
    _check_all(_build(5, dim, space, st, x=x))


@rejects("f16_truncate")
@pytest.mark.parametrize("space,dim", [("ip", 1), ("ip", 100), ("ip", 1024), ("l2", 1), ("l2", 127), ("l2", 1023)])
def test_fp16_cast_by_truncation_fails(space, dim):
    _must_fail(_build(12, dim, space, F16, mutate="f16_truncate"))


# ------------------------------------------------------------------------------------------------------- append vs rescale
def _append_then_rescale(dim, space, st, R, shift, mutate=None, n=43):
    """A: append under R, then rescale by 2^shift (the source is the shadow row itself).  B: append under R 2^shift."""
    a = _build(n, dim, space, st, R)
    old = a["shadow"][a["rows"]].copy()
    E = ref.store_rows_space_standin(old, dim, space, np.float32(2.0 ** -shift), a["pdim"], st, a["slab"], a["scales"], a["shadow"],
                                     a["rows"], a["E"], mutate)
    b = _build(n, dim, space, st, R * 2.0 ** shift, x=a["x"])
    return a, b, old, E


@pytest.mark.parametrize("shift", [1, 3, 20])
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("space,dim", [("ip", 1), ("ip", 100), ("ip", 1024), ("l2", 1), ("l2", 64), ("l2", 127), ("l2", 384), ("l2", 1023)])
def test_rescale_equals_an_append_under_the_grown_scale(space, dim, st, shift):
    a, b, old, E = _append_then_rescale(dim, space, st, 2.0, shift)
    for key in ("slab", "shadow") + (("scales",) if st == I8 else ()):
        assert ref.same_bits(a[key], b[key]), key
    ref.check_rescaled(old, a["shadow"][a["rows"]], space, shift)
    assert E >= a["E"]                                # a running maximum: the old value stays
    _check_all(b)


@rejects("rescale_t_linear")
@pytest.mark.parametrize("shift", [1, 3, 20])
@pytest.mark.parametrize("st", TYPES, ids=IDS)
@pytest.mark.parametrize("dim", [1, 64, 127, 1023])
def test_rescale_with_t_scaled_linearly_fails(dim, st, shift):
    a, b, old, _ = _append_then_rescale(dim, "l2", st, 2.0, shift, mutate="rescale_t_linear")
    with pytest.raises(AssertionError):
        ref.check_rescaled(old, a["shadow"][a["rows"]], "l2", shift)
    assert not ref.same_bits(a["shadow"], b["shadow"])


def test_every_mutation_has_a_rejection_test():
    assert set(REJECTED_BY) == set(ref.MUTATIONS) and len(ref.MUTATIONS) >= 8


# -------------------------------------------------------------------------------------------------------------- the bounds
def test_distance_tol_full_covers_a_zero_row():
    q = np.full(8, 0.25, np.float32)
    x = np.zeros((2, 8), np.float32)
    x[1] = 2.0 ** -20
    assert sr.distance_tol(q, x, "ip")[0] == 0.0                       # the existing bound: nothing for the rounding of 1 - s
    full = ref.distance_tol_full(q, x, "ip")
    assert full[0] == ref.U and full[1] > ref.U * (1 - 2.0 ** -18)
    assert np.array_equal(ref.distance_tol_full(q, x, "l2"), sr.distance_tol(q, x, "l2"))


def test_tolerances_are_the_derived_figures():
    assert ref.queries_tol(np.array([1.0, 0.0]), 384).tolist() == [(13 / 2 + 2) * ref.U + 2.0 ** -149, 2.0 ** -149]
    assert ref.queries_tol(np.array([-1.0]), 1024)[0] == (23 / 2 + 2) * ref.U + 2.0 ** -149
    assert ref.norm_max_rel_tol(1) == 5 * ref.U and ref.norm_max_rel_tol(1024) == 12.5 * ref.U


# ------------------------------------------------------------------------------------------------------ the covering example
def test_the_fp32_norm_can_round_down_onto_a_power_of_two():
    """R is chosen from rows_norm_max, an fp32 norm.  For this row the kernel's order gives exactly 2.0, so R = norm_scale_for(2.0)
    = 2 would leave |x / R| > 1; the store therefore chooses R from an inflated norm (VectorStore._grow_scale)."""
    x = ref.lane0_power_of_two_row(384)
    assert x[0] == 2.0 and np.flatnonzero(x).tolist() == [0, 64, 128, 192, 256, 320]
    got = ref.standin_norm_max(x[None, :])
    true = float(np.sqrt((x.astype(np.float64) ** 2).sum()))
    assert got == 2.0 and true > 2.0 and abs(true / 2.0 - 1.0 - 2.5 * 2.0 ** -26) < 1e-12
    assert nat.norm_scale_for(got) == 2.0                               # the hazard: the uninflated norm maps to R = 2
    assert got >= true * (1 - ref.norm_max_rel_tol(384))                # and the fp32 norm is inside its derived bound
    assert nat.norm_scale_for(nat.covering_norm(got, 384)) == 4.0
    # the inflation covers the bound of rows_norm_max at every dimension, and leaves the scales of ordinary norms alone
    for dim in (1, 64, 384, 1024):
        assert nat.covering_norm(1.0, dim) >= 1.0 / (1 - ref.norm_max_rel_tol(dim))
    assert [nat.norm_scale_for(nat.covering_norm(v, 1024)) for v in (0.0, 0.3, 1.5, 1.95, 5.0)] == [1.0, 0.5, 2.0, 2.0, 8.0]
    assert nat.norm_scale_for(nat.covering_norm(2.0, 384)) == 4.0       # a norm of exactly 2^e now gets R = 2^(e + 1)
