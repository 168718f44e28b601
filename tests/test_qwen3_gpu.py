"""Qwen3-Embedding on the device: the three new kernels alone against fp64 under derived bounds (tests/_qwen3_ref.py), the forward
against transformers' Qwen3Model (tests/golden/encoder_qwen3.npz, tools/make_qwen3_golden.py), and EmbeddingModel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_ref as ar  # noqa: E402
import _qwen3_ref as qr  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seq", [17, 64, 65, 130])
@pytest.mark.parametrize("hd,group", [(64, 1), (64, 2), (128, 1), (128, 2)])
def test_causal_attention_alone_under_the_derived_bound(cuda, hd, group, seq):
    """Batch 3, ragged: one length equal to seq, one crossing a 64 boundary where seq allows it, one of 1.  Real rows element by element;
    padding rows finite; the frame around ctx untouched."""
    import torch
    from rag import _encoder as enc
    kv_heads = 2
    heads, lens = kv_heads * group, [seq, min(seq - 1, 70) if seq > 64 else max(1, seq // 2), 1]
    batch = len(lens)
    qkv = qr.grouped_inputs(batch, seq, heads, kv_heads, hd, lens, seed=hd * 1000 + group * 100 + seq)
    ref, bound = qr.causal_ref_and_bound(qkv, lens, batch, seq, heads, kv_heads, hd)
    frame = 4
    out = torch.full((batch * seq + 2 * frame, heads * hd), 7.0, dtype=torch.float16, device=cuda)
    enc.attention_causal_f16(torch.from_numpy(qkv).to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda), out[frame:], batch, seq,
                             heads, kv_heads, hd)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:frame] == 7.0).all() and (got[-frame:] == 7.0).all()
    got = got[frame:-frame]
    real = (np.arange(seq)[None, :] < np.asarray(lens)[:, None]).reshape(-1)
    ratio = ar.ratio(got[real], ref[real], bound[real])
    print(f"hd {hd} G {group} seq {seq}: ratio {ratio:.3f}")
    assert np.isfinite(got.astype(np.float64)).all()
    assert ratio <= 1.0


@pytest.mark.parametrize("hd,heads,kv_heads", [(64, 2, 1), (64, 3, 3), (128, 2, 1), (128, 2, 2)])
def test_qk_norm_rope_alone(cuda, hd, heads, kv_heads):
    """Positions 0 .. seq - 1 with seq = the table's rows (so its last row is used), gains of mixed sign; V bit-identical."""
    import torch
    from rag import _encoder as enc
    batch, seq, eps = 2, 37, 1e-6
    rng = np.random.default_rng(hd + heads)
    qkv = rng.normal(0.0, 2.0, (batch * seq, (heads + 2 * kv_heads) * hd)).astype(np.float16)
    g_q, g_k = (rng.normal(0.0, 1.0, hd).astype(np.float32) for _ in range(2))
    table = enc.rope_table(seq, hd, 1e6)
    ref, bound = qr.qk_norm_rope_ref_and_bound(qkv, table, g_q, g_k, eps, seq, heads, kv_heads, hd)
    d = torch.from_numpy(qkv).to(cuda)
    enc.qk_norm_rope_f16(d, torch.from_numpy(table).to(cuda), torch.from_numpy(g_q).to(cuda), torch.from_numpy(g_k).to(cuda), eps, batch,
                         seq, heads, kv_heads)
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    nqk = (heads + kv_heads) * hd
    assert np.array_equal(got[:, nqk:].view(np.uint16), qkv[:, nqk:].view(np.uint16))
    ratio = ar.ratio(got[:, :nqk], ref, bound)
    print(f"hd {hd} heads {heads}+{kv_heads}: ratio {ratio:.3f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("n32", [False, True])
@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 6, 8, 16])
@pytest.mark.parametrize("hidden", [64, 128, 1024])
def test_add_rmsnorm_alone(cuda, hidden, nsplit, n32):
    """In-place residual (r32 is the residual), 7 tokens (a partial last workgroup), gains of mixed sign."""
    import torch
    from rag import _encoder as enc
    tokens, eps = 7, 1e-6
    rng = np.random.default_rng(hidden + nsplit)
    y = rng.normal(0.0, 1.0, (nsplit, tokens, hidden)).astype(np.float32)
    res, g = rng.normal(0.0, 2.0, (tokens, hidden)).astype(np.float32), rng.normal(0.0, 1.0, hidden).astype(np.float32)
    want = qr.rmsnorm_ref_and_bound(y, res, g, eps)
    r32 = torch.from_numpy(res).to(cuda)
    x16 = torch.zeros((tokens, hidden), dtype=torch.float16, device=cuda)
    n = torch.zeros((tokens, hidden), dtype=torch.float32, device=cuda) if n32 else None
    enc.add_rmsnorm_f32(torch.from_numpy(y).to(cuda), r32, torch.from_numpy(g).to(cuda), eps, r32, x16, n)
    torch.cuda.synchronize()
    outs = {"r": r32, "x16": x16, **({"n32": n} if n32 else {})}
    for name, t in outs.items():
        ratio = ar.ratio(t.cpu().numpy(), *want[name])
        print(f"hidden {hidden} nsplit {nsplit} {name}: ratio {ratio:.3f}")
        assert ratio <= 1.0, name


@pytest.mark.parametrize("key", sorted(qr.CFGS))
def test_forward_matches_transformers_qwen3(cuda, tmp_path, key):
    """Both tiny models from a sentence-transformers directory, all five lengths in one right-padded batch: real rows and the
    last-token embeddings under the project's forward bounds (the values of test_modernbert_gpu._assert_forward_bounds)."""
    from rag.embedding import EmbeddingModel
    golden, cfg = np.load(qr.GOLDEN), qr.CFGS[key]
    w = qr.make_weights(cfg)
    assert qr.weights_digest(w) == str(golden[key + ".weights_sha256"]) and int(golden[key + ".seed"]) == cfg["seed"]
    model = EmbeddingModel({"model_name": qr.write_model_dir(str(tmp_path / key), cfg, w)})
    assert model.shape.causal and model.shape.pooling == "last" and model.shape.kv_heads == cfg["kv_heads"]
    plan = model.model.causal_plan_describe(len(qr.LENS), qr.SEQ)
    assert "attention_causal_kernel<%d, %d>" % (cfg["head_dim"], cfg["heads"] // cfg["kv_heads"]) in plan and "rowln2" not in plan
    ids, lens = golden[key + ".ids"], np.asarray(qr.LENS, dtype=np.int32)
    emb, hid = model.model.forward(ids, lens, return_hidden=True)
    emb, hid = emb.cpu().numpy().astype(np.float64), hid.cpu().numpy().astype(np.float64)
    assert np.isfinite(hid).all()
    real = np.arange(qr.SEQ)[None, :] < lens[:, None]
    ref_e = golden[key + ".last_norm"]
    f = {"hidden": np.abs(hid[real] - golden[key + ".hidden"]).max(), "last_cos": (1 - (emb * ref_e).sum(1)).max(),
         "last_abs": np.abs(emb - ref_e).max()}
    print(key, {k: float(v) for k, v in f.items()})
    assert f["hidden"] < 3e-2 and f["last_cos"] < 2e-4 and f["last_abs"] < 3e-3


def test_embedding_model_public_interface(cuda):
    from rag.embedding import EmbeddingModel
    prefix = "Instruct: retrieve passages that answer the query\nQuery:"
    model = EmbeddingModel({"model_name": "synthetic:tiny-qwen3", "query_prefix": prefix})
    texts = ["the quick brown fox", "retrieval augmented generation", "a", "cosine similarity ranks passages " * 8]
    out = model.embed(texts)
    assert out.shape == (4, 128) and out.dtype == np.float32 and model.get_dimension() == 128
    assert np.isfinite(out).all() and np.allclose(np.linalg.norm(out, axis=1), 1.0, atol=1e-5)
    assert model.tokenize(texts[:1], kind="query") == model.tokenize([prefix + texts[0]])
    assert np.array_equal(model.embed(texts[:2], kind="query"), model.embed([prefix + t for t in texts[:2]]))
    assert not np.allclose(model.embed(texts[:1], kind="query"), out[:1], atol=1e-3)
    with pytest.raises(NotImplementedError, match="tokenize 'device'.*Qwen3"):
        EmbeddingModel({"model_name": "synthetic:tiny-qwen3", "tokenize": "device"})
