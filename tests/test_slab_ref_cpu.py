"""CPU: the fp64 reference and the shared assertions of the slab-build and eps_q tests (tests/_slab_ref.py) can fail.

The reference is tied to the oracle, a numpy fp32 stand-in of slab_store_row passes the assertions the GPU tests apply to the
kernel, six deliberately broken stand-ins each fail one, and the eps_q window of test_cert_eps_gpu.py rejects a formula with a
wave's partial dropped or without the int8 fixed-point term, on that test's own inputs.
"""
import numpy as np
import pytest

import _slab_ref as ref
from oracle import scan_ref
from rag import _native as nat

F16, I8 = ref.SLAB_F16, ref.SLAB_I8
TYPES = [F16, I8]


def _standin_build(n, dim, st, mutate=None, x=None, seed=5):
    """Append n rows at row0 = 4 of sentinel arrays of n + 9 rows with the stand-in, as the GPU test does with the kernel."""
    pdim = nat.padded_dim(dim, st)
    kinds = twin = None
    if x is None:
        x, kinds, twin = ref.make_rows(n, dim, seed)
    slab, scales, shadow = ref.sentinel_arrays(n + 9, dim, pdim, st)
    before = (slab.copy(), scales.copy(), shadow.copy())
    src = x
    if mutate == "norm_over_pdim":   # the rows sit in a wider buffer whose tail holds the sentinel: reading past dim must show
        src = np.full((n, pdim), 23130.0, np.float32)
        src[:, :dim] = x
    rows = np.arange(4, 4 + n)
    E = ref.store_rows_standin(src, dim, pdim, st, slab, scales, shadow, rows, 0.0, mutate)
    return dict(x=x, kinds=kinds, twin=twin, slab=slab, scales=scales, shadow=shadow, E=E, before=before, rows=rows, dim=dim, pdim=pdim, st=st)


def _check_all(b):
    r = b["rows"]
    ref.check_build(b["x"], b["kinds"], b["twin"], b["slab"][r], b["scales"][r], b["shadow"][r], b["E"], b["dim"], b["pdim"], b["st"],
                    nat.exact_row_error_bound(b["dim"], b["st"]))
    ref.check_untouched(b["before"], (b["slab"], b["scales"] if b["st"] == I8 else None, b["shadow"]), r)


# ------------------------------------------------------------------------------------------- the reference against the oracle
@pytest.mark.parametrize("dim", [1, 65, 384, 1000])
def test_normalise64_is_the_oracles_normalisation(dim):
    x, _, _ = ref.make_rows(40, dim, 1)
    got = ref.normalise64(x)
    want = scan_ref.l2_normalize_rows(x)      # fp64 norm, fp32 division
    assert np.abs(got - want).max() <= 2.0 ** -24 * np.abs(got).max() + 2.0 ** -149
    assert not np.isnan(got).any()
    assert np.array_equal(got[1], np.zeros(dim))                    # the zero row
    assert np.allclose(got[3], x[3].astype(np.float64) / 1e-12, rtol=1e-15)     # norm below 1e-12


@pytest.mark.parametrize("dim", [3, 100, 384, 1024])
def test_row_error64_stays_below_the_analytic_bounds(dim):
    c = scan_ref.synth_corpus(200, dim, seed=dim)
    e16 = ref.row_error64(scan_ref.quantize_rows_f16(c), None, c, dim, F16)
    q, sc = scan_ref.quantize_rows_i8(c)
    e8 = ref.row_error64(q, sc, c, dim, I8)
    assert 0 < e16.max() <= 2.0 ** -11 + np.sqrt(dim) * 2.0 ** -25
    assert 0 < e8.max() <= np.sqrt(dim) / 254
    assert e16.max() < e8.max()
    # and by hand: one row, one element off by a known amount
    one = np.zeros((1, dim), np.float32)
    one[0, 0] = 1.0
    slab = one.astype(np.float16)
    slab[0, 0] = np.float16(1.0 - 2.0 ** -11)
    assert ref.row_error64(slab, None, one, dim, F16)[0] == 2.0 ** -11


def test_library_sizes_match_the_reference():
    for st in TYPES:
        for dim in ref.DIMS:
            assert nat.padded_dim(dim, st) == ref.expected_pdim(dim, st)
    assert nat.padded_dim(384, I8) == 512


# ------------------------------------------------------------------------------------------------------ the stand-in passes
@pytest.mark.parametrize("st", TYPES, ids=["f16", "i8"])
@pytest.mark.parametrize("dim", ref.DIMS)
def test_standin_passes_the_kernels_assertions(dim, st):
    for n in (5, 43):
        _check_all(_standin_build(n, dim, st))


# ---------------------------------------------------------------------------------------------------- broken stand-ins fail
def _must_fail(b):
    with pytest.raises(AssertionError):
        _check_all(b)


@pytest.mark.parametrize("st", TYPES, ids=["f16", "i8"])
@pytest.mark.parametrize("dim", [65, 100, 1000])
def test_norm_over_pdim_fails(dim, st):
    _must_fail(_standin_build(12, dim, st, "norm_over_pdim"))


@pytest.mark.parametrize("st", TYPES, ids=["f16", "i8"])
@pytest.mark.parametrize("dim", [1, 65, 1000])
def test_unwritten_padding_fails(dim, st):
    _must_fail(_standin_build(12, dim, st, "no_padding"))


@pytest.mark.parametrize("dim", [3, 100, 1024])
def test_scale_from_the_unnormalised_row_fails(dim):
    _must_fail(_standin_build(12, dim, I8, "scale_unnormalised"))


@pytest.mark.parametrize("dim", [3, 100, 1024])
def test_fp16_cast_by_truncation_fails(dim):
    _must_fail(_standin_build(12, dim, F16, "f16_truncate"))


@pytest.mark.parametrize("st", TYPES, ids=["f16", "i8"])
@pytest.mark.parametrize("dim", [3, 100, 1024])
def test_E_as_the_mean_fails(dim, st):
    _must_fail(_standin_build(12, dim, st, "E_mean"))


@pytest.mark.parametrize("st", TYPES, ids=["f16", "i8"])
@pytest.mark.parametrize("dim", [3, 100, 1024])
def test_E_without_the_last_wave_fails(dim, st):
    # n = 5: the last row is alone in the second block.  Order the batch so that this row carries the maximum.
    good = _standin_build(5, dim, st)
    r = good["rows"]
    worst = int(np.argmax(ref.row_error64(good["slab"][r], good["scales"][r], good["shadow"][r], dim, st)))
    order = [i for i in range(5) if i != worst] + [worst]
    x = np.ascontiguousarray(good["x"][order])
    b = _standin_build(5, dim, st, "E_without_last_wave", x=x)
    r = b["rows"]
    with pytest.raises(AssertionError):
        ref.check_row_error(b["E"], b["slab"][r], b["scales"][r], b["shadow"][r], dim, st, nat.exact_row_error_bound(dim, st))
    ok = _standin_build(5, dim, st, None, x=x)
    ref.check_row_error(ok["E"], ok["slab"][r], ok["scales"][r], ok["shadow"][r], dim, st, nat.exact_row_error_bound(dim, st))


# ------------------------------------------------------------------------------------- the eps_q window rejects a wrong formula
def _cert_inputs(dim, st):
    """test_cert_eps_gpu.py's inputs with the stand-in in the kernel's place."""
    pdim = nat.padded_dim(dim, st)
    c = ref.cert_corpus(dim)
    n = c.shape[0]
    slab, scales, shadow = ref.sentinel_arrays(n, dim, pdim, st)
    E = ref.store_rows_standin(c, dim, pdim, st, slab, scales, shadow, np.arange(n), 0.0)
    q32 = ref.cert_queries(dim, ref.stored64(slab, scales, dim, st), shadow)
    q16 = np.zeros((q32.shape[0], pdim), np.float16)
    ref.store_rows_standin(q32, dim, pdim, F16, q16, None, np.empty_like(q32), np.arange(q32.shape[0]), 0.0)
    return q32, q16, slab, scales, shadow, E, pdim


@pytest.mark.parametrize("st", TYPES, ids=["f16", "i8"])
@pytest.mark.parametrize("dim", ref.CERT_DIMS)
def test_eps_window_rejects_a_dropped_partial_and_a_missing_fixed_point_term(dim, st):
    q32, q16, slab, scales, shadow, E, pdim = _cert_inputs(dim, st)
    good = ref.eps_formula64(q32, q16, dim, pdim, st == I8, E)
    lo, hi = ref.eps_window(good)
    # what a kernel with the fault would measure as: its formula times the kernel's safety factors (1 .. 1.0003), +- the
    # measurement's resolution -- all of it must lie below the window
    def rejected(bad):
        return (1.0003 * bad + 3 * ref.U < lo).all()
    waves = [w for w in range(4) if w * 64 < min(pdim, 256)]      # a wave owns elements only if the padded row reaches it
    assert len(waves) == (4 if pdim >= 256 else 2)
    for w in waves:
        bad = ref.eps_formula64(q32, q16, dim, pdim, st == I8, E, drop_wave=w)
        if w * 64 < dim:
            assert rejected(bad), f"dropping wave {w}'s partial stays inside the window"
        else:                                                           # only zero padding there: nothing to drop
            assert np.array_equal(bad, good)
    if st == I8:
        assert rejected(ref.eps_formula64(q32, q16, dim, pdim, True, E, fixed_point=False))
        if nat.padded_dim(dim, F16) != pdim:
            assert rejected(_wrong_pdim(q32, q16, dim, E))
    # the bound is sound on these inputs: eps covers the largest deviation over all rows, and the adversarial half uses more of
    # it than the random half
    dev = ref.slab_deviation64(q32, q16, slab, scales, shadow, st)
    assert (dev <= good).all()
    half = ref.CERT_NQ // 2
    assert (dev[half:] / good[half:]).max() > (dev[:half] / good[:half]).max()


def _wrong_pdim(q32, q16, dim, E):
    """int8 with the fp16 slab's padded length (384 instead of 512 at dim 384): smaller sqrt(pdim) and arithmetic terms."""
    p16 = nat.padded_dim(dim, F16)
    return ref.eps_formula64(q32, q16[:, :p16], dim, p16, True, E)
