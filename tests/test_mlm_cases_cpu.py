"""CPU: the case table of tests/_mlm_cases.py covers what tests/test_mlm_pool_shapes_gpu.py claims to run, and the bounds of that
module can fail a wrong kernel.  Everything here is asserted on the fp64 references alone; no device, no native code but the
launch plan (plain C++).

  coverage     every hidden size of make_mlm_plan; the text lengths 63, 64, 65, 127, 128, 129 behind a full text; text starts at no
               multiple of 16, 64 or 128; 16, 17 and 33 row tiles, a ragged last tile among them; the plan's grids as restated.
  admissible   transform_ref_and_bound's second-order fraction below SECOND_ORDER_LIMIT for every case it is used on.
  teeth        per H: the tanh form of GELU lies more than 2 x bound from the erf form at 50 elements or more, so a device output
               within the bound of one form is outside the bound of the other.
  blocks       every 16-row block of every long text owns a column's maximum by more than 8 x the bound (twice the margin the GPU
               test asserts on the device's own t: the difference absorbs the fp16 rounding of t); V is the smallest that does it.
  faults       a 16-row block dropped from the maximum (long cases) or a 128-row tile dropped (group cases) moves a compared
               cell past its bound, for every block and every tile of every case."""
import numpy as np
import pytest

import _mlm_cases as mc
import _row_ref as rr
import _sparse_ref as ref


def test_the_table_covers_every_hidden_size_of_the_plan():
    from rag import _native as nat
    assert [h for h in range(32, 1025 + 64, 32) if _accepts(nat, h)] == list(mc.HIDDEN)
    for H in mc.HIDDEN:
        p = nat.mlm_pool_plan(mc.XFORM_BATCH, mc.XFORM_SEQ, H, mc.XFORM_V)
        assert (p["xform_grid"], p["grid_m"], p["grid_n"], p["tile_k"]) == (4, 1, 2, mc.TILE_K) and H // mc.TILE_K == H // 64
    # the four transform workgroups of 32 rows: the text each row belongs to (-1 past the last token) and whether it is a real token
    tokens = mc.XFORM_BATCH * mc.XFORM_SEQ
    row = np.arange(4 * mc.XFORM_ROWS)
    text = np.where(row < tokens, row // mc.XFORM_SEQ, -1)
    live = (text >= 0) & (row % mc.XFORM_SEQ < np.asarray(mc.XFORM_LENS)[np.maximum(text, 0)])
    text, live = text.reshape(4, -1), live.reshape(4, -1)
    assert tokens == 69 and int(live.sum()) == sum(mc.XFORM_LENS)
    assert set(text[0][live[0]]) == {0, 1} and not live[0].all()            # a whole text, the next one's only token, padding
    assert set(text[1]) == {1, 2} and live[1].any() and not live[1, 0] and not live[1, -1]     # padding, a text's real tokens, padding
    assert set(text[2]) == {2, -1} and not live[2].any()                    # padding up to the last token, then rows past it
    assert set(text[3]) == {-1}                                             # wholly past the last token
    assert mc.XFORM_V - mc.TILE_N == 2


def _accepts(nat, hidden):
    try:
        nat.mlm_pool_plan(1, 1, hidden, 10)
        return True
    except nat.NativeError:
        return False


def test_long_texts_reach_the_required_lengths_and_boundaries():
    assert set(mc.LONG_SEQS) == {65, 100, 128, 129, 200, 300}
    assert set(mc.LONG_INNER.values()) == {63, 64, 65, 127, 128, 129}
    for seq, inner in mc.LONG_INNER.items():
        assert inner <= seq and mc.long_lens(seq) == (seq, 1, inner, seq)
        assert seq > mc.WAVE_ROWS                                           # the last text starts in an earlier wave than it ends
    for seq in (100, 300):
        for b in range(1, 4):
            assert all((b * seq) % m for m in (16, 64, 128)), (seq, b)
    assert mc.POSITION_SEQ in mc.LONG_SEQS
    starts = {(pos * mc.POSITION_SEQ) % mc.TILE_M for pos in range(4)}      # the probe's first row within its tile
    assert len(starts) == 4 and {s // mc.WAVE_ROWS for s in starts} == {0, 1}


def test_group_cases_reach_one_two_and_three_groups():
    from rag import _native as nat
    grid_ms, ragged = set(), 0
    for batch, seq in mc.GROUP_CASES:
        p = nat.mlm_pool_plan(batch, seq, 64, mc.GROUP_V)
        assert (p["grid_m"], p["grid_n"], p["pool_grid"], p["xform_grid"]) == mc.geometry(batch, seq, mc.GROUP_V)
        assert p["grid_n"] == 3 and mc.GROUP_V - 2 * mc.TILE_N == 44
        grid_ms.add(p["grid_m"])
        ragged += (batch * seq) % mc.TILE_M != 0
        case = mc.group_case(batch, seq)
        assert case["lens"].min() >= 1 and case["lens"][-1] == seq and case["lens"][1] == 1
        assert mc.blocks(case["lens"], seq, mc.TILE_M) == list(range(p["grid_m"]))       # every row tile holds a real token
    assert grid_ms == {16, 17, 33} and ragged >= 1
    assert {gm % mc.GROUP_M for gm in grid_ms} == {0, 1}                    # full groups only, and a last group of one tile


def test_the_clamp_case_is_what_it_means():
    assert tuple(mc.clamped(mc.CLAMP_LENS, mc.CLAMP_SEQ)) == mc.CLAMP_MEANS
    assert max(mc.CLAMP_LENS) > mc.CLAMP_SEQ and min(mc.CLAMP_LENS) < 0 and 0 in mc.CLAMP_LENS
    hidden, _ = mc.clamp_case()
    for b, n in enumerate(mc.CLAMP_MEANS):
        assert np.isfinite(hidden[b, :n]).all() and (hidden[b, n:].view(np.int32) == mc.NAN32).all()


@pytest.mark.parametrize("H", mc.HIDDEN)
def test_the_transform_bound_is_admissible_and_tells_erf_gelu_from_tanh_gelu(H):
    for name, case in (("xform", mc.xform_case(H)), ("teeth", mc.teeth_case(H))):
        want, bound, second, rows = mc.transform_bound(case)
        assert second < rr.SECOND_ORDER_LIMIT, (name, second)
        assert np.isfinite(bound).all() and (bound > 2.0 ** -25).all()          # (half an fp16 ulp is never less)
        hd = case["head"]
        h16, _ = mc.real_rows(case)
        assert len(rows) == int(mc.clamped(case["lens"], case["hidden"].shape[1]).sum())
        assert np.allclose(want, ref.transform_ref(h16, hd["w_t"], hd["b_t"], hd["gamma"], hd["beta"], hd["eps"]), rtol=1e-12, atol=1e-13)
    tanh_form = mc.tanh_transform(case)
    apart = int((np.abs(tanh_form - want) > 2.0 * bound).sum())
    print(f"H {H}: second-order fraction {second:.2e}; tanh form more than 2 x bound from the erf form at {apart} of {want.size} elements")
    assert apart >= 50


@pytest.mark.parametrize("seq", mc.LONG_SEQS)
def test_every_block_of_every_long_text_owns_a_column(seq):
    case = mc.long_case(seq)
    t = mc.transform_of(case)
    assert mc.uncovered(t, case, margin=8.0) == []
    for k in range(1, mc.LONG_K[seq]):                                      # V = 128 k + 10 with the smallest such k
        smaller = mc.long_case(seq, k)
        assert mc.uncovered(mc.transform_of(smaller), smaller, margin=8.0) != [], k
    assert case["head"]["w_d"].shape[0] == mc.TILE_N * mc.LONG_K[seq] + 10


@pytest.mark.parametrize("seq", mc.LONG_SEQS)
def test_a_dropped_block_moves_a_cell_past_its_bound(seq):
    case = mc.long_case(seq)
    t = mc.transform_of(case)
    want, bound = mc.pooled_without(t, case)
    ks = mc.blocks(case["lens"], seq)
    assert len(ks) >= 2 * (seq // mc.BLOCK_ROWS)                             # (two full texts; neighbours may share a block)
    for k in ks:
        got, _ = mc.pooled_without(t, case, drop=k)
        assert (np.abs(got - want) > bound).any(), k


@pytest.mark.parametrize("batch,seq", mc.GROUP_CASES)
def test_a_dropped_row_tile_moves_a_cell_past_its_bound(batch, seq):
    case = mc.group_case(batch, seq)
    t = mc.transform_of(case)
    want, bound = mc.pooled_without(t, case)
    assert all(np.count_nonzero(want[b]) > 0 for b in range(batch))
    for tile in range(mc.geometry(batch, seq, mc.GROUP_V)[0]):
        got, _ = mc.pooled_without(t, case, drop=tile, rows=mc.TILE_M)
        assert (np.abs(got - want) > bound).any(), tile
