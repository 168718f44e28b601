"""GPU: XLM-RoBERTa checkpoints through the encoder.  The forward against transformers.XLMRobertaModel in fp64
(tests/golden/encoder_xlmr.npz) and score_pairs against XLMRobertaForSequenceClassification (crossenc_xlmr.npz), both written by
tools/make_xlmr_golden.py; then RAGPipeline on written directories.  Tolerances: tests/test_mpnet_gpu.py's, which are
tests/test_encoder_gpu.py's, and tests/test_crossenc_gpu.py's logit bound -- the arithmetic is the same kernels, with no new term."""
import numpy as np
import pytest

import _crossenc_cases as cc
import _unigram_cases as uc
import _xlmr_cases as xc

pytestmark = pytest.mark.gpu


def _cos(a, b):
    return (a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))


@pytest.fixture(scope="module")
def golden():
    return np.load(xc.GOLDEN)


@pytest.fixture(scope="module")
def ce_golden():
    return np.load(xc.CE_GOLDEN)


@pytest.mark.parametrize("key", [c[0] for c in xc.CASES])
def test_forward_matches_transformers_xlmr(cuda, golden, key):
    import torch
    from rag._encoder import HipEncoder
    _, cfg, seed, batch, seq = next(c for c in xc.CASES if c[0] == key)
    z = golden
    assert int(z[key + ".seed"]) == seed
    enc = HipEncoder(xc.model_shape(cfg), xc.make_weights(cfg, seed), device=cuda)
    assert enc.rel_bias is None
    ids, mask = z[key + ".ids"], z[key + ".mask"].astype(np.int32)
    assert ids.shape == (batch, seq)
    if key == "tiny_1x64":
        assert seq == cfg.max_seq == cfg.max_pos - xc.POS_OFFSET and mask.all()       # the table's last row is read
    if key == "top_2x16":
        assert cfg.vocab_size == 250002 and ids.max() == cfg.vocab_size - 1 and (ids >= cfg.vocab_size - 64).sum() >= 4
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
    assert figures["hidden"] < 3e-2          # (position rows one off, or a zeroed token-type row, fail here: both are ~N(0, 0.05))
    assert figures["mean_cos"] < 2e-4 and figures["cls_cos"] < 2e-4
    assert figures["mean_abs"] < 3e-3 and figures["cls_abs"] < 3e-3
    assert figures["pair"] < 1e-3


@pytest.mark.parametrize("key", [c[0] for c in xc.CE_CASES])
def test_score_pairs_matches_transformers_xlmr(cuda, ce_golden, key):
    import torch
    from dataclasses import replace
    from rag._encoder import HipEncoder
    _, cfg, seed, batch, seq = next(c for c in xc.CE_CASES if c[0] == key)
    z = ce_golden
    assert int(z[key + ".seed"]) == seed
    enc = HipEncoder(replace(xc.model_shape(cfg, "cls")), xc.make_ce_weights(cfg, seed), device=cuda)
    ids, mask = z[key + ".ids"], z[key + ".mask"].astype(np.int32)
    assert ids.shape == (batch, seq) and ((ids == xc.SEP_ID).sum(1) == 3).all()
    lens = mask.sum(1).astype(np.int32)
    got = enc.score_pairs(ids, None, lens)
    zeros = enc.score_pairs(ids, np.zeros_like(ids), lens)
    torch.cuda.synchronize()
    err = np.abs(got.cpu().numpy().astype(np.float64) - z[key + ".logits"]).max()
    print(f"xlmr crossenc {key}: logit error {err:.3e} (bound {cc.LOGIT_TOL:.3e})")
    assert err < cc.LOGIT_TOL
    assert torch.equal(got, zeros)


def test_pipeline_end_to_end_on_written_directories(cuda, tmp_path, monkeypatch):
    """Embedding model and re-ranker from written XLM-R directories; eight chunks, two of them not in a Latin script; a query
    equal to a chunk finds that chunk, with similarity >= 0.999, first among what passes the threshold, and the cross-encoder
    scored what is returned."""
    from rag import RAGPipeline
    from rag.chunking import Chunk
    monkeypatch.setenv("CRS_TOKENIZER", "python")
    emb_dir, ce_dir = str(tmp_path / "emb"), str(tmp_path / "ce")
    n_vocab = len(uc.vocab())
    xc.write_xlmr_dir(emb_dir, uc.NFKC_JSON, seed=21, vocab_size=n_vocab)
    xc.write_xlmr_dir(ce_dir, uc.NFKC_JSON, seed=22, head=True, vocab_size=n_vocab)

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    texts = ["hello world the quick fox", "the model is in the tokens", "hello fox of the world", "quick tokens to the model",
             "привет мир", "日本語 中文 日本", "the fox is quick, hello!", "world of tokens in the model 123"]
    chunks = [Chunk(text=t, chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=None) for r, t in enumerate(texts)]
    for mode in ("host", "device"):
        p = RAGPipeline({"embedding": {"model_name": emb_dir, "device": "cuda", "batch_size": 32, "normalize": True, "tokenize": mode},
                         "vector_store": {"collection_name": "xlmr-e2e-" + mode},
                         "retrieval": {"top_k": 3, "rerank": True, "rerank_model": ce_dir, "similarity_threshold": -1.0,
                                       "diversity_penalty": 0.0}})
        p.setup(Stub())
        model, r = p.embedding_model, p.retriever
        assert model.shape.pos_offset == 2 and type(model.tokenizer).__name__ == "UnigramTokenizer"
        assert r.cross_encoder is not None and r.cross_encoder.shape.pos_offset == 2 and r.cross_encoder._pair_seps == 2
        p.vector_store.create_index(chunks, model.embed_chunks_device(chunks))
        for q in (0, 4, 5):
            r.similarity_threshold = -1.0
            got = p.retrieve(texts[q])
            assert r.last_rerank["mode"] == "cross-encoder" and len(got) == 3
            rr = [c["rerank_score"] for c in got]
            assert rr == sorted(rr, reverse=True)
            again = r.cross_encoder.predict([(texts[q], c["text"]) for c in got])
            assert np.abs(again - np.array(rr)).max() <= cc.LOGIT_TOL
            hits = p.vector_store.search(query_embedding=model.embed(texts[q]), top_k=8)
            assert hits["ids"][0][0] == f"c_{q}"
            sims = [r._distance_to_similarity(d) for d in hits["distances"][0]]
            assert sims[0] >= 0.999 and sims[0] > sims[1], sims
            # seeded random weights put every text within 1e-3 of every other, and a random re-ranker orders by its own logits:
            # with the threshold between the chunk itself and its nearest neighbour only the chunk passes, and it comes first
            r.similarity_threshold = (sims[0] + sims[1]) / 2
            got = p.retrieve(texts[q])
            assert [c["chunk_id"] for c in got] == [f"c_{q}"] and got[0]["score"] >= 0.999 and "rerank_score" in got[0]
