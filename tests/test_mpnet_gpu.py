"""GPU parity of the relative-position-bias attention (attention_kernel<HD, true>, csrc/enc_attn.hip) and of everything above it: the _ex
forward against transformers.MPNetModel in fp64 (tests/golden/encoder_mpnet.npz, tools/make_mpnet_golden.py), against
the project's own oracle with an all-zero bias, the rel_span check, the two kernel selections, and the graph-captured
query forward of the retrieval engine.  Tolerances: tests/test_encoder_gpu.py's (same arithmetic + one fp32 add per score)."""
import numpy as np
import pytest

import _mpnet_cases as mc
from oracle import encoder_ref as er

pytestmark = pytest.mark.gpu


def _cos(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


@pytest.fixture(scope="module")
def golden():
    return np.load(mc.GOLDEN)


def _mpnet_encoder(cfg, seed, cuda, **over):
    from dataclasses import replace
    from rag._encoder import HipEncoder
    shape = replace(mc.model_shape(cfg), **over)
    return HipEncoder(shape, mc.make_weights(cfg, seed), device=cuda)


@pytest.mark.parametrize("key", [c[0] for c in mc.CASES])
def test_forward_matches_transformers_mpnet(cuda, golden, key):
    import torch
    _, cfg, seed, batch, seq = next(c for c in mc.CASES if c[0] == key)
    z = golden
    assert int(z[key + ".seed"]) == seed
    enc = _mpnet_encoder(cfg, seed, cuda)
    assert enc.rel_bias is not None and tuple(enc.rel_bias.shape) == (cfg.heads, 2 * cfg.max_seq - 1)
    ids, mask = z[key + ".ids"], z[key + ".mask"].astype(np.int32)
    assert ids.shape == (batch, seq)
    lens = mask.sum(1).astype(np.int32)
    mean, hidden = enc.forward(ids, lens, return_hidden=True)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens)
    torch.cuda.synchronize()
    mean, cls = mean.cpu().numpy(), cls.cpu().numpy()
    hid = hidden.cpu().numpy().reshape(-1, cfg.hidden)[z[key + ".rows"]]
    figures = dict(hidden=np.abs(hid - z[key + ".hidden"]).max(), mean_cos=(1.0 - _cos(mean, z[key + ".mean_norm"])).max(),
                   cls_cos=(1.0 - _cos(cls, z[key + ".cls_norm"])).max(), mean_abs=np.abs(mean - z[key + ".mean_norm"]).max(),
                   cls_abs=np.abs(cls - z[key + ".cls_norm"]).max(),
                   pair=np.abs(mean @ mean.T - z[key + ".mean_norm"] @ z[key + ".mean_norm"].T).max())
    print(key, {k: float(v) for k, v in figures.items()})
    assert figures["hidden"] < 3e-2          # (a random table is asymmetric in +-offset: a transposed bias index fails here)
    assert figures["mean_cos"] < 2e-4 and figures["cls_cos"] < 2e-4
    assert figures["mean_abs"] < 3e-3 and figures["cls_abs"] < 3e-3
    assert figures["pair"] < 1e-3


@pytest.mark.parametrize("name,cfg,seed,batch,seq", [
    ("tiny", er.TINY, 111, 4, 24), ("tiny-1blk-short", er.TINY, 112, 3, 5), ("tiny-64", er.TINY, 113, 2, 64),
    ("minilm2-2blk", er.truncate_layers(er.MINILM_L6, None, 2)[0], 114, 3, 80),
    ("minilm2-3blk", er.truncate_layers(er.MINILM_L6, None, 2)[0], 115, 2, 150)])
def test_zero_bias_forward_matches_the_oracle(cuda, name, cfg, seed, batch, seq):
    """An all-zero table through the relative-bias kernel is plain BERT attention: the new kernel against oracle/encoder_ref.py."""
    import torch
    from rag._encoder import HipEncoder, ModelShape
    w = er.make_weights(cfg, seed=seed)
    wz = dict(w)
    wz[mc.REL_BIAS] = np.zeros((32, cfg.heads), dtype=np.float32)
    enc = HipEncoder(ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, "mean",
                                cfg.max_seq, rel_buckets=32), wz, device=cuda)
    assert enc.rel_bias is not None and not enc.rel_bias.any().item()
    ids, mask = er.synth_tokens(cfg, batch, seq, seed=seed + 1)
    lens = mask.sum(1).astype(np.int32)
    for pooling in ("mean", "cls"):
        enc.desc.pooling = 1 if pooling == "cls" else 0
        out, hidden = enc.forward(ids, lens, return_hidden=True)
        torch.cuda.synchronize()
        out, hidden = out.cpu().numpy(), hidden.cpu().numpy()
        ref = er.encode_ref(ids, mask, w, cfg, pooling=pooling)
        ref_h = er.encode_ref(ids, mask, w, cfg, return_hidden=True)
        valid = mask.astype(bool)
        assert np.abs(hidden[valid] - ref_h[valid]).max() < 3e-2
        assert (1.0 - _cos(out, ref)).max() < 2e-4
        assert np.abs(out - ref).max() < 3e-3
        assert np.abs(out @ out.T - ref @ ref.T).max() < 1e-3


# (config, seq): the shapes at which the bias kernel's indexing can go wrong and that no case above reaches.  TINY at 1 and 64:
# a single query / exactly one key block, the staged table at its smallest padded span (64).  MID at 65 (a second key block
# of one key), 129 (a third block of one key, past the distance clamp at 128) and 256 (its max_seq: a whole number of key
# blocks).  BASE at 65.
KEY_BLOCK_EDGES = [(mc.TINY, 1), (mc.TINY, 64), (mc.MID, 65), (mc.MID, 129), (mc.MID, 256), (mc.BASE, 65)]


@pytest.mark.parametrize("cfg,seq", KEY_BLOCK_EDGES, ids=[f"{c.name}-{s}" for c, s in KEY_BLOCK_EDGES])
def test_relbias_key_block_edges_match_fp64(cuda, cfg, seq):
    """The _ex forward against _mpnet_cases.encode_ref (fp64, the asymmetric random table) at the key-block edges: batch 2,
    one full row and one row of a single token.  Bounds: those of test_forward_matches_transformers_mpnet (encode_ref in
    fp32 against itself in fp64 stays inside them at these shapes by two orders of magnitude)."""
    import torch
    from _encoder_cases import pool
    seed = 300 + seq
    w = mc.make_weights(cfg, seed)
    enc = _mpnet_encoder(cfg, seed, cuda)
    ids = np.random.default_rng(seed + 1).integers(4, cfg.vocab_size, size=(2, seq)).astype(np.int32)
    lens = np.array([seq, 1], dtype=np.int32)
    mask = (np.arange(seq)[None, :] < lens[:, None]).astype(np.int32)
    ids[:, 0], ids[1, 1:] = mc.CLS_ID, mc.PAD_ID                  # <s> ... </s> | <s> <pad> ...
    if seq > 1:
        ids[0, seq - 1] = mc.SEP_ID
    ref_h = mc.encode_ref(ids, mask, w, cfg, enc.rel_bias.cpu().numpy())
    mean, hidden = enc.forward(ids, lens, return_hidden=True)
    enc.desc.pooling = 1
    cls = enc.forward(ids, lens)
    torch.cuda.synchronize()
    valid = mask.astype(bool)
    figures = dict(hidden=np.abs(hidden.cpu().numpy()[valid] - ref_h[valid]).max())
    for name, got in (("mean", mean.cpu().numpy()), ("cls", cls.cpu().numpy())):
        ref = pool(ref_h, mask, name, True)
        figures[name + "_cos"], figures[name + "_abs"] = (1.0 - _cos(got, ref)).max(), np.abs(got - ref).max()
    print(cfg.name, seq, {k: float(v) for k, v in figures.items()})
    assert figures["hidden"] < 3e-2
    assert figures["mean_cos"] < 2e-4 and figures["cls_cos"] < 2e-4
    assert figures["mean_abs"] < 3e-3 and figures["cls_abs"] < 3e-3


def test_rel_span_shorter_than_seq_is_einval_without_a_launch(cuda):
    import torch
    from rag import _native as nat
    enc = _mpnet_encoder(mc.TINY, 101, cuda, max_seq=16)          # table of span 16
    assert tuple(enc.rel_bias.shape) == (4, 31)
    ids, mask = mc.synth_tokens(mc.TINY, 2, 24, 7)
    lens = mask.sum(1).astype(np.int32)
    out = torch.full((2, 64), 7.0, dtype=torch.float32, device=cuda)
    q16 = torch.full((2, nat.padded_dim(64)), 7.0, dtype=torch.float16, device=cuda)
    with pytest.raises(nat.NativeError, match=r"error -1: .*rel_span 16 .*seq 24"):
        enc.forward(ids, lens, out=out)
    with pytest.raises(nat.NativeError, match=r"error -1: .*rel_span"):
        enc.forward(ids, lens, out=out, q16_out=q16)
    torch.cuda.synchronize()
    assert (out == 7.0).all().item() and (q16 == 7.0).all().item()
    assert torch.isfinite(enc.forward(ids[:, :16], np.minimum(lens, 16), out=out)).all().item()     # span == seq is served


@pytest.mark.parametrize("key", ["tiny_4x24", "mid_3x80", "base_2x16"])
def test_small_lds_selection_gives_equal_results(cuda, golden, key):
    import torch
    _, cfg, seed, _, _ = next(c for c in mc.CASES if c[0] == key)
    enc = _mpnet_encoder(cfg, seed, cuda)
    ids, mask = golden[key + ".ids"], golden[key + ".mask"].astype(np.int32)
    lens = mask.sum(1).astype(np.int32)
    a, ha = enc.forward(ids, lens, return_hidden=True)
    b, hb = enc.forward(ids, lens, return_hidden=True, small_lds=True)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(ha, hb)


def test_engine_query_forward_carries_the_bias(cuda):
    """retrieve_batch through the engine (graph-captured query forwards, CRS_ENC_SMALL_LDS) finds what search_batch finds
    for embeddings of a direct forward call -- and a forward without the bias does not."""
    import torch
    from rag import RAGPipeline
    from rag.chunking import Chunk
    from rag.tokenizer import pad_batch

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    words = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine similarity "
             "vector index chunk context answer question compression memory latency throughput kernel softmax bias bucket").split()
    p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny-mpnet", "device": "cuda", "batch_size": 256, "normalize": True},
                     "retrieval": {"top_k": 5, "similarity_threshold": -1.0, "rerank": False, "diversity_penalty": 0.0, "batch_queries": 64},
                     "vector_store": {"collection_name": "mpnet-e2e"}})
    p.setup(Stub())
    model = p.embedding_model
    assert model.shape.rel_buckets == 32 and model.shape.pos_offset == 2 and model.model.rel_bias is not None
    rng = np.random.default_rng(31)
    chunks = [Chunk(text=" ".join(rng.choice(words, size=int(rng.integers(4, 11)))) + f" {r}", chunk_id=f"c_{r}", start_char=0, end_char=1,
                    page_number=None) for r in range(2048)]
    p.vector_store.create_index(chunks, model.embed_chunks_device(chunks))
    questions = [" ".join(rng.choice(words, size=int(rng.integers(3, 10)))) + f" {q}" for q in range(128)]
    got = p.retrieve_batch(questions)
    assert p.retriever._engine is not None, "the call did not take the engine"
    toks = model.tokenize(questions)
    assert all(t[0] == 0 and t[-1] == 2 for t in toks) and max(len(t) for t in toks) <= 16
    ids, lens = pad_batch(toks, model.tokenizer.pad_id, short_steps=(16,))
    assert model.tokenizer.pad_id == 1 and ids.shape == (128, 16)
    emb = model.model.forward(ids, lens)
    want = p.vector_store.search_batch(emb, top_k=5)["ids"]
    assert [[c["chunk_id"] for c in g] for g in got] == want
    # the same weights without the table: other embeddings, other lists (the comparison above can tell)
    keep, model.model.rel_bias = model.model.rel_bias, None
    plain = p.vector_store.search_batch(model.model.forward(ids, lens), top_k=5)["ids"]
    model.model.rel_bias = keep
    assert sum(a != b for a, b in zip(plain, want)) > 32
