"""GPU: ModernBERT encoders (pre-norm layers, sliding-window attention, GeGLU).  The forward against transformers.ModernBertModel
in fp64 (tests/golden/encoder_modernbert.npz) under the project's forward bounds; the three new kernels launched on their own and
compared element by element with fp64 references of their exact inputs under derived bounds (tests/_attn_win_ref.py,
tests/_row_ref.py, tests/_gated_gelu_ref.py); the CRS_EINVAL cases; a written model directory through EmbeddingModel."""
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_ref as ar  # noqa: E402
import _attn_win_ref as aw  # noqa: E402
import _gated_gelu_ref as gg  # noqa: E402
import _gated_ref as gt  # noqa: E402
import _gemm_ref as gr  # noqa: E402
import _modernbert_cases as mc  # noqa: E402
import _row_ref as rr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.GOLDEN)


def _cos(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


def _encoder(cfg, seed, cuda, weights=None):
    from rag._encoder import HipEncoder
    return HipEncoder(mc.model_shape(cfg), weights or mc.make_weights(cfg, seed), device=cuda)


def _figures(enc, ids, mask, ref_hidden_real, ref_mean, ref_cls):
    import torch
    lens = mask.sum(1).astype(np.int32)
    mean, hidden = enc.forward(ids, lens, return_hidden=True)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens)
    enc.desc.pooling = 0
    torch.cuda.synchronize()
    mean, cls, hidden = mean.cpu().numpy(), cls.cpu().numpy(), hidden.cpu().numpy()
    assert np.isfinite(hidden).all(), "a padding row is not finite"
    return dict(hidden=np.abs(hidden[mask.astype(bool)] - ref_hidden_real).max(), mean_cos=(1.0 - _cos(mean, ref_mean)).max(),
                cls_cos=(1.0 - _cos(cls, ref_cls)).max(), mean_abs=np.abs(mean - ref_mean).max(), cls_abs=np.abs(cls - ref_cls).max())


def _assert_forward_bounds(f):
    assert f["hidden"] < 3e-2
    assert f["mean_cos"] < 2e-4 and f["cls_cos"] < 2e-4
    assert f["mean_abs"] < 3e-3 and f["cls_abs"] < 3e-3


FORWARD_CASES = [(c[0], c[1], c[2]) for c in mc.CASES] + [("a_text", mc.CFG_A, 305)]


@pytest.mark.parametrize("key,cfg,seed", FORWARD_CASES, ids=[c[0] for c in FORWARD_CASES])
def test_forward_matches_transformers_modernbert(cuda, golden, key, cfg, seed):
    assert int(golden[key + ".seed"]) == seed
    enc = _encoder(cfg, seed, cuda)
    assert enc.desc.flags == 2 | 8 | 16 and enc.rope_local is not None and enc.rel_bias is None
    ids, mask = golden[key + ".ids"], golden[key + ".mask"].astype(np.int32)
    plan = enc.prenorm_plan_describe(*ids.shape)
    assert "attention_window_kernel<%d>" % (cfg.hidden // cfg.heads) in plan and "add_layernorm" in plan and "<5" in plan
    assert "qkv_attn_kernel" not in plan and "rowln2" not in plan and "\nlayernorm" not in plan
    f = _figures(enc, ids, mask, golden[key + ".hidden"], golden[key + ".mean_norm"], golden[key + ".cls_norm"])
    print(key, {k: float(v) for k, v in f.items()})
    _assert_forward_bounds(f)


def test_forward_with_checkpoint_biases(cuda):
    """norm_bias / attention_bias / mlp_bias checkpoints: every optional vector reaches its kernel (biases O(0.3): a dropped or
    misplaced one moves the hidden states by far more than the bound)."""
    cfg, seed = mc.CFG_A, 511
    w = mc.make_weights(cfg, seed, biases=True)
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith(".bias"):
            w[k] = (0.3 * rng.standard_normal(w[k].shape)).astype(np.float32)
    ids, mask = mc.synth_tokens(cfg, (80, 21, 5), 80, seed + 1)
    ref = mc.encode_ref(ids, mask, w, cfg)
    plain = mc.encode_ref(ids, mask, {k: v for k, v in w.items() if not k.endswith(".bias")}, cfg)
    real = mask.astype(bool)
    assert np.abs(ref[real] - plain[real]).max() > 0.1
    f = _figures(_encoder(cfg, seed, cuda, w), ids, mask, ref[real], *mc.pooled(ref, mask))
    print({k: float(v) for k, v in f.items()})
    _assert_forward_bounds(f)


# ---- attention_window_kernel on its own ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,heads", [(16, 4), (32, 3), (64, 2)])
@pytest.mark.parametrize("window", [1, 8, 64, 200])
@pytest.mark.parametrize("seq", [16, 80, 144, 200])
def test_window_kernel_alone_under_the_derived_bound(cuda, hd, heads, window, seq):
    """Rows q < len against the fp64 attention over the window's keys; rows q >= len must be finite (len 5 leaves rows without any
    allowed key whenever 5 + W <= seq).  Poisoned padding (K x 4, V = 1000), peaked scores.  W >= seq: also the full-attention
    reference and bound of tests/_attn_ref.py, every row, which is what the blocked kernel is held to."""
    import torch
    from rag import _encoder as enc
    lens = [seq, 5, max(1, (seq * 5) // 8)]
    batch, hidden = len(lens), hd * heads
    line = enc.attention_window_plan_describe(batch, seq, hidden, heads, window)
    assert line == f"attention_window_kernel<{hd}> grid={(seq + 63) // 64}x{heads}x{batch} wg=256x1x1 lds=0\n", line
    qkv = ar.make_inputs(batch, seq, heads, hd, lens, seed=hd * 100000 + window * 1000 + seq, peaked=True)
    frame = 4
    out = torch.full((batch * seq + 2 * frame, hidden), 7.0, dtype=torch.float16, device=cuda)
    d_qkv, d_lens = torch.from_numpy(qkv).to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda)
    enc.attention_window_f16(d_qkv, d_lens, out[frame:frame + batch * seq], batch, seq, heads, window)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:frame] == 7.0).all() and (got[-frame:] == 7.0).all()
    got = got[frame:-frame]
    ref, bound = aw.ref_and_bound(qkv, lens, batch, seq, heads, hd, window)
    r, finite = aw.ratio_real(got, ref, bound, lens, batch, seq)
    print(f"window hd {hd} W {window} seq {seq} ratio {r:.4f}")
    assert finite, "a padding row is not finite"
    assert r <= 1.0
    dead = np.arange(seq) >= 5 + window                      # row 1's queries without any allowed key: zeros
    assert (got[seq:2 * seq][dead] == 0).all()
    if window >= seq:
        full_ref, full_bound, _ = ar.ref_and_bound(qkv, lens, batch, seq, heads, hd)
        rf = ar.ratio(got, full_ref, full_bound)
        blocked = torch.empty((batch * seq, hidden), dtype=torch.float16, device=cuda)
        enc.attention_f16(d_qkv, d_lens, blocked, batch, seq, heads, route=3)        # no whole-sequence, no short kernel: the blocked one
        torch.cuda.synchronize()
        rb = ar.ratio(blocked.cpu().numpy(), full_ref, full_bound)
        print(f"  against full attention: window kernel {rf:.4f}, blocked kernel {rb:.4f}")
        assert rf <= 1.0 and rb <= 1.0


# ---- add_layernorm*_kernel on its own --------------------------------------------------------------------------------------------
TOKENS = 13                     # not a multiple of the four tokens of a workgroup


@pytest.mark.parametrize("hidden", [64, 384, 768, 1024])
@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 6, 8, 16])
def test_add_layernorm_alone_under_the_derived_bounds(cuda, hidden, nsplit):
    import torch
    from rag import _encoder as enc
    pl, two = rr.row_form(hidden)
    want = f"add_layernorm{'2' if two else ''}_kernel<{pl}, {nsplit}> grid={(TOKENS + 3) // 4}x1x1 wg=256x1x1 lds=0\n"
    assert enc.row_plan_describe(enc.ROW_ADD_LAYERNORM, TOKENS, hidden, nsplit) == want
    g = torch.Generator().manual_seed(hidden * 100 + nsplit)
    y = torch.randn((nsplit, TOKENS, hidden), generator=g) * 0.7
    res = torch.randn((TOKENS, hidden), generator=g) * 1.3
    bias_full = torch.randn(hidden, generator=g) * 0.4
    gain = 1.0 + 0.2 * torch.randn(hidden, generator=g)
    beta_full = 0.3 * torch.randn(hidden, generator=g)
    eps = 1e-5
    frame = 4
    for bias, beta, with_n32 in ((bias_full, beta_full, True), (None, None, False), (bias_full, None, True)):
        v, e = rr.sum_ref_and_err(rr.ln_terms(y, bias, res))
        ref, b32, b16, frac = rr.layernorm_ref_and_bound(y, bias, res, gain, beta if beta is not None else torch.zeros(hidden), eps)
        assert frac < rr.SECOND_ORDER_LIMIT
        dev = [None if t is None else t.to(cuda) for t in (y, bias, res, gain, beta)]

        def launch(in_place):
            r32 = torch.full((TOKENS + 2 * frame, hidden), 7.0, dtype=torch.float32, device=cuda)
            x16 = torch.full((TOKENS + 2 * frame, hidden), 7.0, dtype=torch.float16, device=cuda)
            n32 = torch.full((TOKENS + 2 * frame, hidden), 7.0, dtype=torch.float32, device=cuda)
            r_in = dev[2]
            if in_place:
                r32[frame:frame + TOKENS] = dev[2]
                r_in = r32[frame:frame + TOKENS]
            enc.add_layernorm_f32(dev[0], dev[1], r_in, dev[3], dev[4], eps, r32[frame:frame + TOKENS], x16[frame:frame + TOKENS],
                                  n32[frame:frame + TOKENS] if with_n32 else None)
            torch.cuda.synchronize()
            outs = [t.cpu() for t in (r32, x16, n32)]
            for t in outs:
                assert (t[:frame] == 7.0).all() and (t[-frame:] == 7.0).all()
            return [t[frame:-frame] for t in outs]
        r32, x16, n32 = launch(False)
        ratios = dict(r32=rr.ratio(r32, v, e + rr.TINY), x16=rr.ratio(x16, ref, b16))
        if with_n32:
            ratios["n32"] = rr.ratio(n32, ref, b32)
            assert rr.x16_is_a_rounding_of_x32(x16, n32)
        else:
            assert (n32 == 7.0).all()
        print(hidden, nsplit, "bias" if bias is not None else "no bias", "beta" if beta is not None else "no beta", ratios)
        assert all(r <= 1.0 for r in ratios.values())
        again = launch(True)
        assert all(torch.equal(a, b) for a, b in zip((r32, x16, n32), again)), "in place (residual == r32) differs"


# ---- GEMM mode 5 on its own, per family: the routes and sizes of mode 4's test (tests/test_nomic_gpu.py) --------------------------
TILED = [(0, 0, m, f, k) for m in (1, 65, 200) for f in (64, 192, 1536) for k in (64, 384, 768)]
PANEL = [(1, fl, m, f, k) for fl in (0, 1) for m in (1, 65, 200) for f in (64, 192, 1536) for k in (384, 768)]
LARGE = [(0, 0, 512, 1536, 768), (0, 0, 2048, 192, 384)]
GEMM8 = [(0, 0, 2816, 1536, 384), (0, 0, 2816, 1536, 768), (0, 0, 16384, 192, 384), (0, 0, 5632, 1536, 384)]


@pytest.mark.parametrize("route,flags,m,f,k", TILED + PANEL + LARGE + GEMM8)
def test_gelu_gated_gemm_alone_under_the_derived_bound(cuda, route, flags, m, f, k):
    import torch
    from rag._encoder import gemm_f16_routed, gemm_plan_describe
    line, slabs = gemm_plan_describe(m, 2 * f, k, 5, route, flags)
    assert slabs == 1
    if (route, flags, m, f, k) in GEMM8:
        cus = torch.cuda.get_device_properties(cuda).multi_processor_count
        items = (m // 256) * (2 * f // 256)
        assert line.startswith(f"gemm8_kernel<5, {'true' if items > cus else 'false'}, 0> "), line
    elif route == 0:
        assert line.startswith("gemm_f16_kernel<5> ")
    else:
        assert re.match(r"gemm_panel_kernel<5, (64|128)> ", line)
        if flags:
            assert int(re.search(r"lds=(\d+)", line).group(1)) <= 48 * 1024
    a, w, bias = gt.make_inputs(m, f, k)
    ps = gr.products(a, w, 1)
    frame = 8
    for b in (bias, None):
        ref, bound = gg.ref_and_bound(a, w, b, ps=ps)
        out = torch.full((m + 2 * frame, f), 7.0, dtype=torch.float16, device=cuda)
        gemm_f16_routed(a.to(cuda), w.to(cuda), None if b is None else b.to(cuda), None, out[frame:frame + m], 5, route, flags)
        torch.cuda.synchronize()
        got = out.cpu()
        assert (got[:frame] == 7.0).all() and (got[-frame:] == 7.0).all()
        r = gr.ratio(got[frame:-frame], ref, bound)
        print(line.split()[0], m, f, k, "bias" if b is not None else "no bias", "ratio", r)
        assert r <= 1.0


# ---- refusals, the loader, the tokeniser ------------------------------------------------------------------------------------------
def test_einval_cases_launch_nothing(cuda, golden):
    import torch
    from dataclasses import replace
    from rag import _encoder as enc
    from rag import _native as nat
    cfg, seed = mc.CFG_A, 301
    e = _encoder(cfg, seed, cuda)
    ids = torch.from_numpy(golden["a_48.ids"]).to(cuda)
    lens = torch.from_numpy(golden["a_48.mask"].astype(np.int32).sum(1).astype(np.int32)).to(cuda)
    ws = torch.empty(e.workspace_bytes(3, 48), dtype=torch.uint8, device=cuda)
    out = torch.full((3, cfg.hidden), 7.0, device=cuda)
    args = lambda: (ids, lens, e._wlist, e._desc_list, float(e.desc.ln_eps), ws, out, None, 0, True, None)   # noqa: E731

    def refused(match, call):
        with pytest.raises((nat.NativeError, RuntimeError), match=match):
            with nat._translate():
                call()
        torch.cuda.synchronize()
        assert (out == 7.0).all()
    fin = e.final_ln[0]
    refused("window must be >= 1", lambda: nat.ops().encoder_forward_prenorm(*args(), e.rope_table, e.rope_local, 0, 3, fin, None))
    refused("global_every must be >= 1", lambda: nat.ops().encoder_forward_prenorm(*args(), e.rope_table, e.rope_local, 8, 0, fin, None))
    refused("positions 40 must be >= seq 48", lambda: nat.ops().encoder_forward_prenorm(*args(), e.rope_table[:40].contiguous(),
                                                                                       e.rope_local[:40].contiguous(), 8, 3, fin, None))
    # the older entry points carry no tables / window: they refuse the descriptor
    refused("CRS_ENC_PRENORM needs both rope tables", lambda: nat.ops().encoder_forward_rope(*args(), None, e.rope_table))
    refused("CRS_ENC_PRENORM needs both rope tables", lambda: nat.ops().encoder_forward_ex(*args(), None))
    bias = torch.zeros((cfg.heads, 2 * 48 - 1), device=cuda)
    refused("does not combine with a relative-position bias or the pair head", lambda: nat.ops().encoder_forward_rope(*args(), bias, e.rope_table))
    # ... and the pair head: crs_encoder_score_pairs with a pre-norm descriptor and a well-formed head, with and without type ids
    head = [torch.zeros((cfg.hidden, cfg.hidden), device=cuda), torch.zeros(cfg.hidden, device=cuda), torch.zeros(cfg.hidden, device=cuda),
            torch.zeros(1, device=cuda)]
    scores = torch.full((3,), 7.0, device=cuda)
    pooled = torch.full((3, cfg.hidden), 7.0, device=cuda)
    for type_ids in (None, torch.zeros_like(ids)):
        refused("does not combine with a relative-position bias or the pair head",
                lambda: nat.ops().encoder_score_pairs(ids, type_ids, lens, e._wlist, head, e._desc_list, float(e.desc.ln_eps), 0, ws, scores,
                                                      pooled, None))
        assert (scores == 7.0).all() and (pooled == 7.0).all()
    # layer 0 has no attention norm: one given there would be ignored, so it is refused
    with_norm = list(e._wlist)
    with_norm[5 + 4] = e._wlist[5 + 12 + 4]                    # layer 1's attn_norm gain in layer 0's ln1_g slot
    refused("layer 0 has no attention norm",
            lambda: nat.ops().encoder_forward_prenorm(ids, lens, with_norm, e._desc_list, 1e-5, ws, out, None, 0, True, None, e.rope_table,
                                                      e.rope_local, 8, 3, fin, None))
    missing = list(e._wlist)
    missing[5 + 12 + 4] = e._wlist[5 + 4]                      # the empty tensor (NULL) in layer 1's ln1_g slot
    refused("only layer 0 may have a NULL ln1_g",
            lambda: nat.ops().encoder_forward_prenorm(ids, lens, missing, e._desc_list, 1e-5, ws, out, None, 0, True, None, e.rope_table,
                                                      e.rope_local, 8, 3, fin, None))
    # a descriptor without the flag at the pre-norm entry
    plain = e._desc_list[:7] + [2 | 16]
    refused("need a CRS_ENC_PRENORM descriptor",
            lambda: nat.ops().encoder_forward_prenorm(ids, lens, e._wlist, plain, 1e-5, ws, out, None, 0, True, None, e.rope_table, e.rope_local, 8, 3, fin, None))
    with pytest.raises(nat.NativeError, match="crs_encoder_prenorm_plan_describe"):
        nat.encoder_plan_describe(e.desc, 3, 48)
    # the stand-alone entries
    qkv = torch.zeros((48, 3 * cfg.hidden), dtype=torch.float16, device=cuda)
    ctx = torch.full((48, cfg.hidden), 7.0, dtype=torch.float16, device=cuda)
    with pytest.raises(nat.NativeError, match="window must be >= 1"):
        enc.attention_window_f16(qkv, lens[:1], ctx, 1, 48, cfg.heads, 0)
    with pytest.raises(nat.NativeError, match="window must be >= 1"):
        enc.attention_window_plan_describe(1, 48, cfg.hidden, cfg.heads, 0)
    with pytest.raises(nat.NativeError, match="head_dim must be 16, 32 or 64"):
        enc.attention_window_f16(qkv, lens[:1], ctx, 1, 48, 8, 8)
    y = torch.zeros((5, 8, 64), device=cuda)
    with pytest.raises(nat.NativeError, match="nsplit must be"):
        enc.add_layernorm_f32(y, None, None, y[0, 0], None, 1e-5, y[0], ctx[:8, :64], None)
    with pytest.raises(nat.NativeError, match="n / 2 a multiple of 32"):
        enc.gemm_plan_describe(8, 96, 128, 5, 0, 0)
    with pytest.raises(nat.NativeError):                       # the split-K route has no gated mode
        enc.gemm_plan_describe(2048, 768, 3072, 5, 2, 0)
    torch.cuda.synchronize()
    assert (ctx == 7.0).all()
    # shapes no loader builds
    with pytest.raises(NotImplementedError, match="prenorm and gelu_gated come together"):
        enc.HipEncoder(replace(mc.model_shape(cfg), gelu_gated=False, gated=True), mc.make_weights(cfg, seed), device=cuda)
    with pytest.raises(ValueError, match="window >= 1"):
        enc.HipEncoder(replace(mc.model_shape(cfg), window=0), mc.make_weights(cfg, seed), device=cuda)
    with pytest.raises(ValueError, match="layer 0 of a pre-norm model has no attention norm"):
        enc.HipEncoder(mc.model_shape(cfg), {**mc.make_weights(cfg, seed), "layers.0.attn_norm.weight": np.ones(cfg.hidden, dtype=np.float32)},
                       device=cuda)


def test_embedding_model_on_a_written_directory_gives_the_golden(cuda, golden, tmp_path):
    from rag.embedding import EmbeddingModel
    cases = json.load(open(mc.TOKENIZER_CASES, encoding="utf-8"))
    d = mc.write_modernbert_dir(str(tmp_path / "mb"), mc.CFG_A, mc.make_weights(mc.CFG_A, 305), prefix="model.", max_seq=cases["max_seq"])
    model = EmbeddingModel({"model_name": d, "batch_size": 64})
    s = model.shape
    assert s.prenorm and s.gelu_gated and not s.gated and s.window == 8 and s.global_every == 3 and s.max_seq == cases["max_seq"]
    assert s.rotary_theta == mc.GLOBAL_THETA and s.local_theta == mc.LOCAL_THETA and s.ln_eps == 1e-5 and s.pooling == "mean"
    assert model.tokenize(cases["texts"]) == cases["ids"]
    got = model.embed(cases["texts"])
    ref = golden["a_text.mean_norm"]
    print("1 - cos", float((1.0 - _cos(got, ref)).max()), "abs", float(np.abs(got - ref).max()))
    assert (1.0 - _cos(got, ref)).max() < 2e-4 and np.abs(got - ref).max() < 3e-3
    with pytest.raises(NotImplementedError, match="'device' is not supported for ModernBERT"):
        EmbeddingModel({"model_name": d, "tokenize": "device"})


def test_synthetic_models_run(cuda):
    from rag.embedding import EmbeddingModel
    m = EmbeddingModel({"model_name": "synthetic:tiny-modernbert"})
    v = m.embed(["a short text", "another one " * 40])
    assert v.shape == (2, 64) and np.isfinite(v).all() and np.allclose(np.linalg.norm(v, axis=1), 1.0, atol=1e-5)
