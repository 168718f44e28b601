"""GPU: the MLM head with the max-pool epilogue (csrc/mlm_pool.hip, crs::mlm_sparse_pool) against tests/_sparse_ref.py.

The vocabulary projection is checked against fp64 on the SAME fp16-rounded operands: the decoder as given, and the transform's
output t as the device itself left it in the workspace (fp16).  The bound is derived, not fitted (_sparse_ref.pool_bound):
2 gamma_K sum_k |a_k w_k| + one fp32 ulp of the result.  The transform in front is checked on its own against fp64 on the
fp16-rounded hidden states and W_t: |t_dev - t_ref| <= half an fp16 ulp of the value (the one rounding of the result) + 3e-4.
The absolute term is the worst case of the fp32 chain at the operand scales of _head, not a fit: the K = 64 projection and its
bias are off by at most gamma_65 sum|w h| <= 3.9e-6 x 10; GELU has slope <= 1.13 and its erf fit adds 1.4e-6: 4.6e-5 per
element; LayerNorm subtracts a mean with the same error and scales by gamma / std <= 1.4 x 2: 2 x 4.6e-5 x 2.8 = 2.6e-4."""
import numpy as np
import pytest

import _sparse_ref as ref

pytestmark = pytest.mark.gpu

TILE_N = ref.TILE_N
H = 64


def _head(V, Hd, seed):
    rng = np.random.default_rng(seed)
    w_t = (rng.standard_normal((Hd, Hd)) / np.sqrt(Hd)).astype(np.float16)
    w_d = (rng.standard_normal((V, Hd)) * 0.05).astype(np.float16)
    return dict(w_t=w_t, b_t=(rng.standard_normal(Hd) * 0.1).astype(np.float32), gamma=(1.0 + 0.1 * rng.standard_normal(Hd)).astype(np.float32),
                beta=(0.1 * rng.standard_normal(Hd)).astype(np.float32), eps=1e-12, w_d=w_d,
                bias=(rng.standard_normal(V) * 0.2 - 0.1).astype(np.float32))


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _run(cuda, head, hidden, lens, vp=None, fill=None, dev_head=None):
    """(out [batch, Vp] numpy, t16 [tokens_padded, H] numpy fp16, the guard cells behind out)."""
    import torch
    from rag import _native as nat
    batch, seq, Hd = hidden.shape
    V = head["w_d"].shape[0]
    vp = V if vp is None else vp
    d = dev_head or {k: _dev(cuda, v) for k, v in head.items() if k != "eps"}
    plan = nat.mlm_pool_plan(batch, seq, Hd, V)
    ws = torch.zeros(plan["workspace_bytes"], dtype=torch.uint8, device=cuda)
    guard = 64
    flat = torch.full((batch * vp + guard,), -7.5 if fill is None else fill, dtype=torch.float32, device=cuda)
    out = flat[: batch * vp].view(batch, vp)
    nat.mlm_sparse_pool(_dev(cuda, hidden), _dev(cuda, lens.astype(np.int32)), d["w_t"], d["b_t"], d["gamma"], d["beta"], head["eps"],
                        d["w_d"], d["bias"], 512, ws, out)
    torch.cuda.synchronize()
    t16 = ws[: plan["t16_bytes"]].view(torch.float16).view(plan["tokens_padded"], Hd).cpu().numpy()
    return out.cpu().numpy(), t16, flat[batch * vp:].cpu().numpy()


def _lens(batch, seq, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, seq + 1, size=batch)
    lens[0] = seq
    if batch > 1:
        lens[1] = 1
    return lens.astype(np.int32)


def _check(out, t16, guard, head, hidden, lens, vp):
    batch, seq, Hd = hidden.shape
    V = head["w_d"].shape[0]
    # the transform: fp64 on the fp16-rounded hidden states and W_t
    t_dev = t16[: batch * seq].astype(np.float64).reshape(batch, seq, Hd)
    for b in range(batch):
        n = int(lens[b])
        want = ref.transform_ref(ref.f16(hidden[b, :n]), head["w_t"], head["b_t"], head["gamma"], head["beta"], head["eps"])
        tol = np.spacing(np.abs(want).astype(np.float16)).astype(np.float64) / 2 + 3e-4
        err = np.abs(t_dev[b, :n] - want)
        assert (err <= tol).all(), f"transform, text {b}: worst error / tolerance {np.max(err / tol):.3f}"
        assert (t_dev[b, n:] == 0).all(), f"text {b}: padding rows of t are not zero"
    assert (t16[batch * seq:] == 0).all()
    # the projection + pool: fp64 on the device's own t and the fp16 decoder
    want, absdot = ref.pool_ref(t_dev, lens, head["w_d"], head["bias"])
    bound = ref.pool_bound(absdot, want, Hd)
    got = out[:, :V].astype(np.float64)
    assert np.isfinite(out[:, :V]).all() and (out[:, :V] >= 0).all()
    ratio = np.abs(got - want) / bound
    print(f"batch {batch} seq {seq} V {V}: worst |device - fp64| / bound = {ratio.max():.3f}; nonzero {np.count_nonzero(got)} of {got.size}")
    assert (ratio <= 1.0).all(), f"worst error / bound {ratio.max():.3f} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    assert (out[:, V:] == -7.5).all(), "columns [V, Vp) were written"
    assert (guard == -7.5).all(), "memory past [batch, Vp] was written"
    return want


@pytest.mark.parametrize("V", [1, 10, 16, 250, TILE_N - 1, TILE_N, TILE_N + 1, 2 * TILE_N + 10])
def test_pool_matches_fp64_on_the_same_fp16_operands(cuda, V):
    """Every V x seq in {1, 17, 48} x batch in {1, 5}: 5 x 48 = 240 rows are two row tiles (see the next test for three), sequences
    straddle 16-row blocks, 64-row wave spans and the 128-row tile; lens mixed, 1 and seq among them; Vp = V + 3 with canaries."""
    head = _head(V, H, seed=V)
    for seq in (1, 17, 48):
        for batch in (1, 5):
            rng = np.random.default_rng(1000 * seq + batch)
            hidden = rng.standard_normal((batch, seq, H)).astype(np.float32)
            lens = _lens(batch, seq, seq + batch)
            out, t16, guard = _run(cuda, head, hidden, lens, vp=V + 3)
            _check(out, t16, guard, head, hidden, lens, V + 3)


def test_three_row_tiles_and_every_position_gives_the_same_bits(cuda):
    """9 texts of 48 tokens = 432 rows: four row tiles.  One text's row is bit-equal alone and at every position of the batch."""
    import torch
    V, seq, batch = 2 * TILE_N + 10, 48, 9
    head = _head(V, H, seed=3)
    rng = np.random.default_rng(8)
    hidden = rng.standard_normal((batch, seq, H)).astype(np.float32)
    lens = _lens(batch, seq, 4)
    out, t16, guard = _run(cuda, head, hidden, lens)
    _check(out, t16, guard, head, hidden, lens, V)
    probe, probe_len = hidden[3].copy(), 29
    alone, _, _ = _run(cuda, head, probe[None], np.array([probe_len]))
    assert np.count_nonzero(alone) > 10
    for pos in range(batch):
        h2, l2 = hidden.copy(), lens.copy()
        h2[pos], l2[pos] = probe, probe_len
        got, _, _ = _run(cuda, head, h2, l2)
        assert (got[pos].view(np.int32) == alone[0].view(np.int32)).all(), f"position {pos}"
        others = [b for b in range(batch) if b != pos]
        assert (got[others].view(np.int32) == out[others].view(np.int32)).all(), f"the other texts moved when text {pos} changed"


def test_the_transform_tolerance_tells_erf_gelu_from_tanh_gelu(cuda):
    """The tolerance of _check is derived as a worst case, so it must still be sharp enough to mean something: the same fp64
    transform with the tanh form of GELU (which differs from the erf form by up to 5e-4 before the LayerNorm) lies outside it
    against the device's output, at many elements, while the erf form lies inside it everywhere."""
    head = _head(16, H, seed=11)
    rng = np.random.default_rng(21)
    hidden = (rng.standard_normal((5, 48, H)) * 1.5).astype(np.float32)
    lens = np.full(5, 48, dtype=np.int32)
    _, t16, _ = _run(cuda, head, hidden, lens)
    t_dev = t16[: 5 * 48].astype(np.float64)
    h = ref.f16(hidden.reshape(-1, H))
    erf_form = ref.transform_ref(h, head["w_t"], head["b_t"], head["gamma"], head["beta"], head["eps"])
    x = h @ head["w_t"].astype(np.float64).T + head["b_t"]
    g = 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))
    tanh_form = (g - g.mean(-1, keepdims=True)) / np.sqrt(g.var(-1, keepdims=True) + head["eps"]) * head["gamma"] + head["beta"]
    tol = np.spacing(np.abs(erf_form).astype(np.float16)).astype(np.float64) / 2 + 3e-4
    assert (np.abs(t_dev - erf_form) <= tol).all()
    outside = (np.abs(t_dev - tanh_form) > tol).sum()
    print(f"tanh-GELU reference: {outside} of {t_dev.size} elements outside the tolerance")
    assert outside >= 50


def test_padding_rows_never_reach_the_result(cuda):
    """NaN and 1e30 in the hidden states of padding positions: finite output, bit-equal to the run with zeros there."""
    V, seq, batch = TILE_N + 1, 17, 5
    head = _head(V, H, seed=5)
    rng = np.random.default_rng(2)
    hidden = rng.standard_normal((batch, seq, H)).astype(np.float32)
    lens = np.array([17, 1, 5, 16, 9], dtype=np.int32)
    runs = []
    for pad in (0.0, np.nan, 1e30):
        h = hidden.copy()
        for b in range(batch):
            h[b, lens[b]:] = pad
        out, t16, _ = _run(cuda, head, h, lens)
        assert np.isfinite(out).all() and np.isfinite(t16.astype(np.float32)).all(), pad
        runs.append(out)
    assert (runs[1].view(np.int32) == runs[0].view(np.int32)).all() and (runs[2].view(np.int32) == runs[0].view(np.int32)).all()


def test_all_negative_columns_are_exactly_zero_and_zero_length_rows_too(cuda):
    V, seq, batch = 250, 17, 3
    head = _head(V, H, seed=6)
    head["bias"][::3] = -1000.0                        # far below any dot product: those columns' logits are all negative
    rng = np.random.default_rng(3)
    hidden = rng.standard_normal((batch, seq, H)).astype(np.float32)
    lens = np.array([17, 0, 4], dtype=np.int32)        # lens 0 is clamped, not an error: an all-zero row
    out, _, _ = _run(cuda, head, hidden, lens, fill=3.25)
    assert (out[:, ::3].view(np.int32) == 0).all()
    assert (out[1].view(np.int32) == 0).all()
    assert np.count_nonzero(out[0]) > 20


def test_the_real_tail_at_768_by_30522(cuda):
    """H = 768, V = 30522 = 16 * 1907 + 10 (238 column tiles and one of 58 columns), batch 2, seq 32."""
    V, Hd, seq, batch = 30522, 768, 32, 2
    head = _head(V, Hd, seed=9)
    rng = np.random.default_rng(4)
    hidden = rng.standard_normal((batch, seq, Hd)).astype(np.float32)
    lens = np.array([32, 11], dtype=np.int32)
    out, t16, guard = _run(cuda, head, hidden, lens, vp=V + 6)
    _check(out, t16, guard, head, hidden, lens, V + 6)


def test_bad_arguments_are_refused(cuda):
    import torch
    from rag import _native as nat
    head = _head(10, H, seed=1)
    d = {k: _dev(cuda, v) for k, v in head.items() if k != "eps"}
    hidden = torch.zeros((2, 8, H), device=cuda)
    lens = torch.ones(2, dtype=torch.int32, device=cuda)
    args = lambda **kw: dict(dict(hidden=hidden, lens=lens, max_pos=512), **kw)          # noqa: E731

    def call(hidden, lens, max_pos, out=None):
        return nat.mlm_sparse_pool(hidden, lens, d["w_t"], d["b_t"], d["gamma"], d["beta"], 1e-12, d["w_d"], d["bias"], max_pos, None, out)

    assert call(**args()).shape == (2, 10)
    with pytest.raises(nat.NativeError, match="max_pos"):
        call(**args(max_pos=7))
    with pytest.raises(nat.NativeError, match="Vp"):
        call(**args(out=torch.zeros((2, 9), device=cuda)))
    with pytest.raises(nat.NativeError, match="lens"):
        call(**args(lens=lens[:1]))
    with pytest.raises(nat.NativeError, match="hidden"):
        nat.mlm_sparse_pool(torch.zeros((2, 8, 96), device=cuda), lens, torch.zeros((96, 96), dtype=torch.float16, device=cuda),
                            torch.zeros(96, device=cuda), torch.zeros(96, device=cuda), torch.zeros(96, device=cuda), 1e-12,
                            torch.zeros((10, 96), dtype=torch.float16, device=cuda), d["bias"], 512)
