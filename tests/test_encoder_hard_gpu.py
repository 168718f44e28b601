"""B4: the regimes where a subtly wrong kernel shows -- peaked attention on every attention kernel form with ragged lengths
at the edges of the 16- / 32- / 64-key groups, LayerNorm inputs with a large mean and a few wide channels at every split-K
slab count, GELU pre-activations past the erf clamp -- against the fp64 oracle (bound 2 E_q + a, tests/_encoder_cases.py);
the GELU epilogue of crs_gemm_f16 on its own against fp64 erf; and the inputs the kernels clamp (lens 0 / > seq, ids
outside the vocabulary)."""
import math

import numpy as np
import pytest

import _encoder_cases as ec
from oracle import encoder_ref as er

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ec.HARD_CASES, ids=lambda c: c.name)
def test_hard_case(cuda, case):
    ec.check_case_on_gpu(case, cuda)


@pytest.mark.parametrize("case", [c for c in ec.HARD_CASES if c.query_batch], ids=lambda c: c.name)
def test_hard_case_small_lds(cuda, case):
    ec.check_small_lds_on_gpu(case, cuda)


# (m, n, k) -> kernel plan_gemm (csrc/enc_plan.cpp) picks: tiled 128 x 128; row-streaming (m, n >= 512, K = 128); phase-scheduled 256 x 256
# (whole tiles, >= 128 of them); 256-row tiles (K >= 512, n % 256 == 0, m not a multiple of 256)
@pytest.mark.parametrize("m,n,k", [(200, 192, 64), (1024, 512, 128), (4096, 2048, 256), (4100, 2048, 512)])
def test_gelu_epilogue_against_fp64_erf(cuda, m, n, k):
    """crs_gemm_f16 mode 1 with pre-activations spread over [-12, 12] (enc_gelu.h clamps erf's argument at |z| = 4, i.e.
    |x| = 5.66, and claims |gelu error| <= 1.4e-6) against fp64 0.5 x (1 + erf(x / sqrt 2)) of the exact pre-activation.
    Bound: half an fp16 ulp of the result (the output rounding) + 2 x 1.4e-6.  The spread comes from the bias and the
    products stay below 0.25 in magnitude, so that the fp32 accumulation of the pre-activation (<= half an fp32 ulp of 12
    = 4.8e-7 per add, gelu' <= 1.13) fits into the second 1.4e-6."""
    import torch
    from rag._encoder import gemm_f16
    g = torch.Generator().manual_seed(m + n + k)
    a = (torch.randn((m, k), generator=g) * 0.25).half()
    w = (torch.randn((n, k), generator=g) * (0.25 / math.sqrt(k))).half()
    bias = (torch.rand(n, generator=g) * 24.0 - 12.0).float()
    bias[:8] = torch.tensor([-12.0, 12.0, -5.66, 5.66, -4.0, 4.0, 0.0, -0.75])
    x = a.double() @ w.double().T + bias.double()
    assert x.min() < -11.5 and x.max() > 11.5
    ref = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    out = gemm_f16(a.to(cuda), w.to(cuda), bias.to(cuda), None, 1)
    torch.cuda.synchronize()
    out = out.cpu().double()
    assert torch.isfinite(out).all()
    expo = torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -14)))          # fp16: normal ulp 2^(e - 10), subnormal 2^-24
    half_ulp = 0.5 * torch.pow(2.0, expo - 10)
    excess = ((out - ref).abs() - half_ulp).max().item()
    print(f"gelu epilogue {m}x{n}x{k}: max (|err| - half ulp) = {excess:.3e} (allowed 2.8e-6)")
    assert excess <= 2 * 1.4e-6


def _one_layer(cuda, cfg, seed):
    case = ec.Case("robust", cfg, 6, 32, seed, "clamped inputs", "ragged1")
    w = ec.case_weights(case)
    return case, w, ec.hip_encoder(case, cuda, w)


@pytest.mark.parametrize("cfg", [ec.TINY1, ec.MINI1, ec.BGE1], ids=["tiny", "minilm", "bge"])
def test_lens_outside_1_seq_are_clamped(cuda, cfg):
    """lens = 0 and lens > seq: the attention kernels clamp to [1, seq], pool_kernel to [0, seq].  Output finite and equal
    (bit for bit) to the forward on the clamped lengths; a zero-length row pools to sum / clamp(count, 1e-9) = the zero
    vector under mean pooling, to the [CLS] state of a 1-token row under CLS pooling; the other rows are unaffected."""
    case, w, enc = _one_layer(cuda, cfg, 401)
    ids, mask, lens = ec.case_inputs(case)
    bad = lens.copy()
    bad[1], bad[2], bad[3] = 0, case.seq + 7, -3
    att = np.clip(bad, 1, case.seq).astype(np.int32)        # what attention sees
    for pooling in ("mean", "cls"):
        for normalize in (True, False):
            got, hid = ec.guarded_forward(enc, ids, bad, pooling=pooling, normalize=normalize, return_hidden=True)
            want, whid = ec.guarded_forward(enc, ids, att, pooling=pooling, normalize=normalize, return_hidden=True)
            assert np.isfinite(got).all() and np.isfinite(hid).all()
            assert np.array_equal(hid, whid)
            if pooling == "mean":
                assert np.array_equal(got[[1, 3]], np.zeros_like(got[[1, 3]]))
                keep = [0, 2, 4, 5]
            else:
                keep = list(range(6))
            assert np.array_equal(got[keep], want[keep])
            # ... and against the oracle on the clamped inputs
            m_att = (np.arange(case.seq)[None, :] < att[:, None]).astype(np.int32)
            ref = er.encode_ref(ids, m_att, w, cfg, pooling=pooling, normalize=normalize, dtype=__import__("torch").float64)
            tol = 3e-3 if normalize else 2e-2 * max(1.0, np.abs(ref).max())
            assert np.abs(got[keep] - ref[keep]).max() < tol


@pytest.mark.parametrize("cfg", [ec.TINY1, ec.MINI1, ec.H128_2], ids=["tiny", "minilm", "h128"])
def test_ids_outside_the_vocabulary_are_clamped(cuda, cfg):
    """embed_ln clamps ids to [0, vocab): a forward with negative and too-large ids equals, bit for bit, the forward on the
    clamped ids, and rows without bad ids equal the forward on the original batch."""
    case, w, enc = _one_layer(cuda, cfg, 402)
    ids, mask, lens = ec.case_inputs(case)
    bad = ids.copy()
    bad[1, 0], bad[1, 3], bad[3, 0] = -5, cfg.vocab_size, 2 ** 31 - 1
    clamped = np.clip(bad, 0, cfg.vocab_size - 1).astype(np.int32)
    got, hid = ec.guarded_forward(enc, bad, lens, pooling="mean", normalize=True, return_hidden=True)
    want, whid = ec.guarded_forward(enc, clamped, lens, pooling="mean", normalize=True, return_hidden=True)
    orig = ec.guarded_forward(enc, ids, lens, pooling="mean", normalize=True)
    assert np.isfinite(got).all()
    assert np.array_equal(got, want) and np.array_equal(hid, whid)
    assert np.array_equal(got[[0, 2, 4, 5]], orig[[0, 2, 4, 5]])
    ref = er.encode_ref(clamped, mask, w, cfg, pooling="mean")
    assert np.abs(got - ref).max() < 3e-3
