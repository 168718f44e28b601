"""CPU checks of the encoder oracle's fp64 / kernel-numerics forms (oracle/encoder_ref.py) and of the case tables the
GPU tests use (tests/_encoder_cases.py): every case must be well conditioned BEFORE a GPU assertion leans on it."""
import numpy as np
import pytest
import torch

import _encoder_cases as ec
from oracle import encoder_ref as er

CONFIGS = [("tiny", er.TINY, 4, 24), ("minilm", er.MINILM_L6, 3, 32), ("bge", er.BGE_BASE, 2, 16)]


@pytest.mark.parametrize("name,cfg,batch,seq", CONFIGS)
def test_fp32_oracle_is_within_1e5_of_fp64(name, cfg, batch, seq):
    w = er.make_weights(cfg, seed=12)
    ids, mask = er.synth_tokens(cfg, batch, seq, seed=13)
    valid = mask.astype(bool)
    h32 = er.encode_ref(ids, mask, w, cfg, return_hidden=True)
    h64 = er.encode_ref(ids, mask, w, cfg, return_hidden=True, dtype=torch.float64)
    assert h32.dtype == np.float32 and h64.dtype == np.float64
    assert np.abs(h32 - h64)[valid].max() < 1e-5
    for pooling in ("mean", "cls"):
        p32 = er.encode_ref(ids, mask, w, cfg, pooling=pooling)
        p64 = er.encode_ref(ids, mask, w, cfg, pooling=pooling, dtype=torch.float64)
        assert p32.dtype == np.float32 and p64.dtype == np.float64
        assert np.abs(p32 - p64).max() < 1e-5


@pytest.mark.parametrize("name,cfg,batch,seq", CONFIGS[:2])
def test_emulated_model_without_roundings_is_the_fp64_model(name, cfg, batch, seq):
    cfg, _ = er.truncate_layers(cfg, None, 2)
    w = er.make_weights(cfg, seed=5)
    ids, mask = er.synth_tokens(cfg, batch, seq, seed=6)
    h64 = er.encode_ref(ids, mask, w, cfg, return_hidden=True, dtype=torch.float64)
    assert np.array_equal(er.encode_ref(ids, mask, w, cfg, return_hidden=True, dtype=torch.float64, emulate_fp16=()), h64)
    assert np.array_equal(er.encode_ref(ids, mask, w, cfg, return_hidden=True, dtype=torch.float64, emulate_fp16=False), h64)
    # ... and each rounding point on its own moves the result, by less than all of them do together by more than 3 x
    full = np.abs(er.encode_ref(ids, mask, w, cfg, return_hidden=True, dtype=torch.float64, emulate_fp16=True) - h64).max()
    assert 0 < full < 1e-2
    for point in sorted(er.FP16_ROUNDINGS):
        one = np.abs(er.encode_ref(ids, mask, w, cfg, return_hidden=True, dtype=torch.float64, emulate_fp16=[point]) - h64).max()
        assert 0 < one < 3 * full, point
    with pytest.raises(ValueError):
        er.encode_ref(ids, mask, w, cfg, emulate_fp16=["nope"])


def test_weight_variants_leave_the_default_draw_alone():
    cfg = er.TINY
    base = er.make_weights(cfg, seed=3)
    hard = er.make_weights(cfg, seed=3, qk_mult=3.0, dense_bias_offset=0.5, ln_outliers=4, ln_outlier_gain=4.0, ffn_up_mult=3.0)
    assert base.keys() == hard.keys()
    q, up = "encoder.layer.1.attention.self.query.weight", "encoder.layer.1.intermediate.dense.weight"
    assert np.array_equal(hard[q], base[q] * np.float32(3)) and np.array_equal(hard[up], base[up] * np.float32(3))
    v = "encoder.layer.1.attention.self.value.weight"
    assert np.array_equal(hard[v], base[v])
    b0, b1 = "encoder.layer.0.output.dense.bias", "encoder.layer.1.attention.output.dense.bias"
    assert np.allclose(hard[b0] - base[b0], 0.5) and np.allclose(hard[b1] - base[b1], -1.0)
    g = "encoder.layer.0.output.LayerNorm.weight"
    assert (hard[g] != base[g]).sum() == 4 and np.allclose(hard[g][[1, 17, 33, 49]], 4 * base[g][[1, 17, 33, 49]])
    # ... and the default draw is what it was
    again = er.make_weights(cfg, seed=3)
    assert all(np.array_equal(base[k], again[k]) for k in base)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_truncation_is_a_full_run_stopped_early(n):
    cfg = er.EncoderConfig(vocab_size=500, hidden=64, layers=4, heads=2, ffn=128, max_pos=32, max_seq=32)
    w = er.make_weights(cfg, seed=9, qk_mult=2.0)
    cfg_n, w_n = er.truncate_layers(cfg, w, n)
    assert cfg_n.layers == n and set(w_n) == {name for name, _ in er.weight_names(cfg_n)}
    again = er.make_weights(cfg_n, seed=9, qk_mult=2.0)      # per-tensor streams: the truncated draw IS the first n layers
    assert all(np.array_equal(w_n[k], again[k]) for k in w_n)
    ids, mask = er.synth_tokens(cfg, 3, 20, seed=10)
    for kw in (dict(), dict(dtype=torch.float64), dict(dtype=torch.float64, emulate_fp16=True)):
        stopped = er.encode_ref(ids, mask, w, cfg, return_hidden=True, stop_after=n, **kw)
        assert np.array_equal(er.encode_ref(ids, mask, w_n, cfg_n, return_hidden=True, **kw), stopped)
        assert not np.allclose(stopped, er.encode_ref(ids, mask, w, cfg, return_hidden=True, **kw), atol=1e-3)
    assert er.truncate_layers(cfg, None, 4)[0] == cfg
    with pytest.raises(ValueError):
        er.truncate_layers(cfg, w, 5)


def test_case_tables_are_well_formed():
    for c in ec.ALL_CASES:
        cfg = c.cfg
        assert cfg.hidden % 64 == 0 and cfg.hidden <= 1024 and cfg.head_dim in (16, 32, 64) and cfg.ffn % 64 == 0, c.name
        assert 1 <= c.seq <= cfg.max_pos and 1 <= cfg.layers <= 2, c.name
        ids, mask, lens = ec.case_inputs(c)
        assert ids.shape == mask.shape == (c.batch, c.seq) and lens.min() >= 1 and lens.max() == c.seq, c.name
        assert ids.min() >= 0 and ids.max() < cfg.vocab_size, c.name
        if c.lens == "ragged1" and c.batch > 1:
            assert lens[-1] == 1, c.name
    assert any(c.tokens > 4096 and c.tokens % 128 for c in ec.LAYER_CASES)


@pytest.mark.parametrize("case", ec.ALL_CASES, ids=lambda c: c.name)
def test_conditioning_cap(case):
    """A case is admissible only if its quantisation floor E_q on the hidden state is <= 3e-2 / 2, so that 2 E_q + a is
    never looser than the 3e-2 of test_encoder_gpu.py; and the accumulation term must stay what it is meant to be, a
    small correction (a < E_q / 4), or the bound would be set by a margin instead of by the design's roundings."""
    ref = ec.reference(case)
    print(f"{case.name}: E_q {ref.eq_hidden:.3e}  fp32-fp64 {ref.acc_hidden:.3e}")
    assert 0 < ref.eq_hidden <= ec.COND_CAP
    assert ref.acc_hidden < 1e-4 and ec.ACC_MARGIN * ref.acc_hidden < ref.eq_hidden / 4
    assert ref.bound_hidden() < 3.1e-2
    for mode in ec.POOLED_MODES:
        assert 0 < ref.eq_pooled[mode] and ec.ACC_MARGIN * ref.acc_pooled[mode] < ref.eq_pooled[mode]


def test_hard_regimes_are_hard():
    """The weight variants reach the regime they are in the tables for (measured on the fp64 model's intermediates)."""
    import math
    cfg = ec.MINI1
    ids, mask = er.synth_tokens(cfg, 4, 64, seed=1, ragged=False)

    def probe(**kw):
        w = {k: torch.from_numpy(v).double() for k, v in er.make_weights(cfg, seed=2, **kw).items()}
        x = (w["embeddings.word_embeddings.weight"][torch.from_numpy(ids).long()] + w["embeddings.position_embeddings.weight"][:64][None]
             + w["embeddings.token_type_embeddings.weight"][0])
        x = er._ln(x, w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"], cfg.ln_eps)
        p = "encoder.layer.0."
        q = (x @ w[p + "attention.self.query.weight"].T + w[p + "attention.self.query.bias"]).view(4, 64, 12, 32).transpose(1, 2)
        k = (x @ w[p + "attention.self.key.weight"].T + w[p + "attention.self.key.bias"]).view(4, 64, 12, 32).transpose(1, 2)
        top = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(32), -1).amax(-1).mean().item()
        up = (x @ w[p + "intermediate.dense.weight"].T + w[p + "intermediate.dense.bias"]).abs().max().item()
        return top, up

    top0, up0 = probe()
    top3, _ = probe(qk_mult=3.0)
    _, up3 = probe(ffn_up_mult=3.0)
    assert top0 < 0.3 and top3 > 0.7          # near-uniform -> peaked
    assert up0 < 6.0 and up3 > 9.0            # past the erf clamp at |x| = 4 sqrt 2 = 5.66
