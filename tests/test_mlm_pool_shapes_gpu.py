"""GPU: the SPLADE head (csrc/mlm_pool.hip) at the shapes the workload uses and tests/test_mlm_pool_gpu.py does not reach: every
mlm_transform_kernel<NJ> with a projection K loop of H / 64 steps behind it, texts longer than a wave's 64 rows and the 128-row
tile, more than one group of kMlmGroupM row tiles, and lens outside [0, seq].  The cases are tests/_mlm_cases.py's;
tests/test_mlm_cases_cpu.py proves without a device what they cover and that the bounds used here fail a wrong kernel.

The transform is held to _sparse_ref.transform_ref_and_bound (derived per H, half an fp16 ulp included) where H varies, and to
test_mlm_pool_gpu._check's own tolerance at H = 64; the projection and the pool always to _sparse_ref.pool_bound on the device's own
fp16 t, through the same _check / _check_pool.  Padding positions hold NaN patterns in every case."""
import numpy as np
import pytest

import _mlm_cases as mc
import _row_ref as rr
from test_mlm_pool_gpu import _check, _check_pool, _dev, _run

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _dev_head(cuda, head):
    return {k: _dev(cuda, v) for k, v in head.items() if k != "eps"}


def _run_case(cuda, case, **kw):
    return _run(cuda, case["head"], case["hidden"], case["lens"], vp=case["vp"], **kw)


def _plan(case):
    from rag import _native as nat
    batch, seq, H = case["hidden"].shape
    p = nat.mlm_pool_plan(batch, seq, H, case["head"]["w_d"].shape[0])
    return p["grid_m"], p["grid_n"], p["pool_grid"], p["xform_grid"]


def _transform_ratio(t16, case, tag):
    """the device's t at the real tokens against transform_ref_and_bound; exact zeros everywhere else"""
    want, bound, second, rows = mc.transform_bound(case)
    assert second < rr.SECOND_ORDER_LIMIT
    ratio = np.abs(t16[rows].astype(np.float64) - want) / bound
    at = np.unravel_index(ratio.argmax(), ratio.shape)
    off = int((t16[rows].view(np.int16) != want.astype(np.float16).view(np.int16)).sum())
    print(f"mlm-transform-ratio {tag}: worst |device - fp64| / bound = {ratio.max():.4f} at token row {rows[at[0]]} column {at[1]}; "
          f"{off} of {want.size} elements are not the fp16 nearest to the fp64 value")
    assert (ratio <= 1.0).all(), f"{tag}: worst error / bound {ratio.max():.3f}"
    rest = np.ones(t16.shape[0], dtype=bool)
    rest[rows] = False
    assert (t16[rest].view(np.int16) == 0).all(), "a padding row or a row past the last token is not exact zeros"
    return want, bound


@pytest.mark.parametrize("H", mc.HIDDEN)
def test_every_transform_instantiation_and_k_loop_length(cuda, H):
    case = mc.xform_case(H)
    assert _plan(case) == (1, 2, 2, 4)
    out, t16, guard = _run_case(cuda, case)
    assert t16.shape == (mc.TILE_M, H)
    _transform_ratio(t16, case, f"H {H} NJ {H // 64} xform")
    assert (t16[mc.XFORM_BATCH * mc.XFORM_SEQ:].view(np.int16) == 0).all()                       # rows 69..127
    _check_pool(out, t16, guard, case["head"], case["lens"], mc.XFORM_BATCH, mc.XFORM_SEQ, case["vp"])
    assert np.count_nonzero(out[:, : mc.XFORM_V]) > 20
    again, t16_again, _ = _run_case(cuda, case)
    assert (_bits(again) == _bits(out)).all() and (t16_again.view(np.int16) == t16.view(np.int16)).all()


@pytest.mark.parametrize("H", mc.HIDDEN)
def test_the_transform_bound_tells_erf_gelu_from_tanh_gelu_on_the_device(cuda, H):
    """The device is within the bound of the erf form everywhere and outside it for the tanh form at 50 elements or more."""
    case = mc.teeth_case(H)
    _, t16, _ = _run_case(cuda, case)
    want, bound = _transform_ratio(t16, case, f"H {H} NJ {H // 64} teeth")
    outside = int((np.abs(t16[: want.shape[0]].astype(np.float64) - mc.tanh_transform(case)) > bound).sum())
    print(f"H {H}: tanh-GELU reference outside the bound at {outside} of {want.size} elements")
    assert outside >= 50


@pytest.mark.parametrize("seq", mc.LONG_SEQS)
def test_texts_longer_than_a_wave_span_and_a_tile(cuda, seq):
    case = mc.long_case(seq)
    out, t16, guard = _run_case(cuda, case)
    _check(out, t16, guard, case["head"], case["hidden"], case["lens"], case["vp"])
    # the precondition, on the device's own t: every 16-row block of every text decides a compared cell by 4 x its bound
    t_dev = t16[: 4 * seq].astype(np.float64).reshape(4, seq, 64)
    assert mc.uncovered(t_dev, case, margin=4.0) == []
    again, _, _ = _run_case(cuda, case)
    assert (_bits(again) == _bits(out)).all()


def test_a_long_text_gives_the_same_bits_at_every_position(cuda):
    """200 tokens alone start at row 0; as text 1, 2, 3 of four they start at rows 200, 400, 600: in another wave, another tile."""
    case, probe = mc.position_case()
    d = _dev_head(cuda, case["head"])
    alone, _, _ = _run(cuda, case["head"], probe[None], np.array([mc.POSITION_SEQ]), dev_head=d)
    assert np.count_nonzero(alone) > 10
    base, _, _ = _run(cuda, case["head"], case["hidden"], case["lens"], dev_head=d)
    for pos in range(4):
        hidden, lens = case["hidden"].copy(), case["lens"].copy()
        hidden[pos], lens[pos] = probe, mc.POSITION_SEQ
        got, _, _ = _run(cuda, case["head"], hidden, lens, dev_head=d)
        assert (_bits(got[pos]) == _bits(alone[0])).all(), f"position {pos}"
        others = [b for b in range(4) if b != pos]
        assert (_bits(got[others]) == _bits(base[others])).all(), f"the other texts moved when text {pos} changed"


@pytest.mark.parametrize("batch,seq", mc.GROUP_CASES)
def test_more_than_one_group_of_row_tiles(cuda, batch, seq):
    case = mc.group_case(batch, seq)
    assert _plan(case) == mc.geometry(batch, seq, mc.GROUP_V)
    d = _dev_head(cuda, case["head"])
    out, t16, guard = _run_case(cuda, case, dev_head=d)
    _check(out, t16, guard, case["head"], case["hidden"], case["lens"], case["vp"])
    assert all(np.count_nonzero(out[b, : mc.GROUP_V]) > 0 for b in range(batch))
    again, _, _ = _run_case(cuda, case, dev_head=d)
    assert (_bits(again) == _bits(out)).all()
    # the last text lives in the last row tile, in the ragged last group where there is one: alone it gives the same bits
    alone, _, _ = _run(cuda, case["head"], case["hidden"][-1:], case["lens"][-1:], vp=case["vp"], dev_head=d)
    assert (_bits(alone[0]) == _bits(out[-1])).all()


def test_lens_outside_the_sequence_are_clamped(cuda):
    hidden, head = mc.clamp_case()
    d = _dev_head(cuda, head)
    got, t16, guard = _run(cuda, head, hidden, np.asarray(mc.CLAMP_LENS), dev_head=d)
    want, t16_want, _ = _run(cuda, head, hidden, np.asarray(mc.CLAMP_MEANS), dev_head=d)
    assert np.isfinite(got).all() and np.isfinite(t16.astype(np.float32)).all()
    assert (_bits(got) == _bits(want)).all() and (t16.view(np.int16) == t16_want.view(np.int16)).all()
    assert (_bits(got[1:3]) == 0).all()
    assert np.count_nonzero(got[0]) > 10 and np.count_nonzero(got[4]) > 10
    assert (guard == mc.FILL).all()
    _check(want, t16_want, guard, head, hidden, np.asarray(mc.CLAMP_MEANS), head["w_d"].shape[0])
