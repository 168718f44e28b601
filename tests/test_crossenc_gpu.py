"""GPU: cross-encoder re-ranking.  crs_encoder_score_pairs (per-token type ids at the embedding step, the pooler + classifier head
kernel; csrc/enc_misc.hip, csrc/enc_pair.hip) against transformers' BertForSequenceClassification in fp64 (tests/golden/crossenc.npz, written by
tools/make_crossenc_golden.py), the head alone against a bound computed from its own inputs, the all-zero and out-of-range type
ids, CrossEncoderReranker.predict and the retriever's rerank_model switch.

The logit bound of the parity test (cc.LOGIT_TOL) is provisional: four times the error of an fp16-rounding model, not yet four
times a figure measured on the device (tests/_crossenc_cases.py says how to replace it)."""
import numpy as np
import pytest

import _crossenc_cases as cc

pytestmark = pytest.mark.gpu

KEYS = [c[0] for c in cc.CASES]
HIDDEN_TOL = 3e-2                     # the encoder tests' bound on final hidden states (fp16 GEMM operands)
U = 2.0 ** -24


@pytest.fixture(scope="module")
def golden():
    return np.load(cc.GOLDEN)


_ENCODERS = {}


def encoder(key, cuda):
    """One HipEncoder per case (its weights are seeded per case), uploaded once for the module."""
    if key not in _ENCODERS:
        from rag._encoder import HipEncoder
        _, cfg, seed, _, _ = cc.case(key)
        w = cc.make_weights(cfg, seed)
        _ENCODERS[key] = (HipEncoder(cc.model_shape(cfg), w, device=cuda), w, cfg)
    return _ENCODERS[key]


def inputs(golden, key):
    ids, types, mask = golden[key + ".ids"], golden[key + ".type_ids"].astype(np.int32), golden[key + ".mask"]
    return ids, types, mask.sum(1).astype(np.int32)


@pytest.mark.parametrize("small_lds", [False, True])
@pytest.mark.parametrize("key", KEYS)
def test_parity_with_transformers(cuda, golden, key, small_lds):
    enc, w, cfg = encoder(key, cuda)
    ids, types, lens = inputs(golden, key)
    scores, pooled, hidden = enc.score_pairs(ids, types, lens, return_pooled=True, return_hidden=True, small_lds=small_lds)
    assert scores.dtype.is_floating_point and tuple(scores.shape) == (ids.shape[0],) and scores.is_cuda
    hid = hidden.cpu().numpy().reshape(-1, cfg.hidden)[golden[key + ".rows"]]
    e_hid = np.abs(hid - golden[key + ".hidden"]).max()
    e_pool = np.abs(pooled.cpu().numpy().astype(np.float64) - golden[key + ".pooled"])
    e_logit = np.abs(scores.cpu().numpy().astype(np.float64) - golden[key + ".logits"]).max()
    # |d pooled_j| <= sum_k |W_p[j, k]| |d h_k| (tanh's slope is <= 1) with every |d h_k| under the hidden-state bound
    pool_bound = HIDDEN_TOL * np.abs(w[cc.HEAD[0]].astype(np.float64)).sum(1)
    print(f"crossenc parity {key} small_lds={int(small_lds)}: hidden {e_hid:.3e} pooled {e_pool.max():.3e} (bound {pool_bound.min():.3e}) "
          f"logit {e_logit:.3e} (bound {cc.LOGIT_TOL:.3e})")
    assert e_hid < HIDDEN_TOL
    assert (e_pool < pool_bound[None, :]).all()
    assert e_logit < cc.LOGIT_TOL
    assert cc.LOGIT_TOL * 10 <= cc.ZEROED_TYPES_GAP


@pytest.mark.parametrize("key", KEYS)
def test_head_alone_against_a_bound_from_its_inputs(cuda, golden, key):
    enc, w, cfg = encoder(key, cuda)
    ids, types, lens = inputs(golden, key)
    scores, pooled, hidden = enc.score_pairs(ids, types, lens, return_pooled=True, return_hidden=True)
    h = hidden[:, 0].cpu().numpy().astype(np.float64)                  # what the head kernel read
    ref_pooled, ref_logit = cc.head_ref(h, w)
    Wp, bp = np.abs(w[cc.HEAD[0]].astype(np.float64)), np.abs(w[cc.HEAD[1]].astype(np.float64))
    wc, bc = np.abs(w[cc.HEAD[2]].astype(np.float64).reshape(-1)), abs(float(w[cc.HEAD[3]].reshape(-1)[0]))
    H = cfg.hidden
    pool_bound = 4 * H * U * (np.abs(h) @ Wp.T + bp)                   # [B, H]; carried through tanh (slope <= 1)
    logit_bound = pool_bound @ wc + 4 * H * U * (np.abs(ref_pooled) @ wc + bc)
    got_pooled, got = pooled.cpu().numpy().astype(np.float64), scores.cpu().numpy()
    print(f"crossenc head {key}: pooled err {np.abs(got_pooled - ref_pooled).max():.3e} (bound {pool_bound.min():.3e}), "
          f"logit err {np.abs(got - ref_logit).max():.3e} (bound {logit_bound.min():.3e})")
    assert (np.abs(got_pooled - ref_pooled) <= pool_bound).all()
    assert (np.abs(got.astype(np.float64) - ref_logit) <= logit_bound).all()
    sig = enc.score_pairs(ids, types, lens, activation="sigmoid").cpu().numpy()
    want = (1.0 / (1.0 + np.exp(-got.astype(np.float64)))).astype(np.float32)
    ulps = np.abs(sig.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    assert sig.dtype == np.float32 and ulps.max() <= 2, (sig, want)


@pytest.mark.parametrize("small_lds", [False, True])
@pytest.mark.parametrize("key", ["tiny_4x24", "mid_3x80", "base_2x150"])
def test_all_zero_type_ids_are_the_plain_forward(cuda, golden, key, small_lds):
    import torch
    enc, _, _ = encoder(key, cuda)
    ids, types, lens = inputs(golden, key)
    s0, p0, h0 = enc.score_pairs(ids, np.zeros_like(types), lens, return_pooled=True, return_hidden=True, small_lds=small_lds)
    s1, p1, h1 = enc.score_pairs(ids, None, lens, return_pooled=True, return_hidden=True, small_lds=small_lds)
    assert torch.equal(s0, s1) and torch.equal(p0, p1) and torch.equal(h0, h1)
    _, hf = enc.forward(ids, lens, return_hidden=True, small_lds=small_lds)
    assert torch.equal(h0, hf)
    st, _, ht = enc.score_pairs(ids, types, lens, return_pooled=True, return_hidden=True, small_lds=small_lds)
    assert not torch.equal(ht, h0) and not torch.equal(st, s0)           # and the true type ids are seen


@pytest.mark.parametrize("key", ["tiny_4x24", "mid_3x80"])
def test_out_of_range_ids_are_clamped(cuda, golden, key):
    import torch
    enc, _, cfg = encoder(key, cuda)
    ids, types, lens = inputs(golden, key)
    s_ref, h_ref = enc.score_pairs(ids, types, lens, return_hidden=True)
    s7, h7 = enc.score_pairs(ids, np.where(types == 1, 7, types).astype(np.int32), lens, return_hidden=True)
    assert torch.equal(s7, s_ref) and torch.equal(h7, h_ref)            # type id 7 with two rows behaves as 1
    last, above = ids.copy(), ids.copy()
    last[:, 1], above[:, 1] = cfg.vocab_size - 1, cfg.vocab_size + 5    # a token id above the vocabulary behaves as its last row
    s_last, h_last = enc.score_pairs(last, types, lens, return_hidden=True)
    s_above, h_above = enc.score_pairs(above, types, lens, return_hidden=True)
    assert torch.equal(s_above, s_last) and torch.equal(h_above, h_last)
    assert torch.isfinite(s_above).all() and torch.isfinite(h_above).all() and torch.isfinite(s7).all()


WORDS = ("alpha beta gamma delta epsilon zeta eta theta iota kappa lambda mu nu xi omicron pi rho sigma tau upsilon phi chi psi "
         "omega retrieval vector index chunk query answer").split()


def _texts(rng, n, lo, hi):
    return [" ".join(rng.choice(WORDS, size=int(rng.integers(lo, hi)))) for _ in range(n)]


@pytest.fixture(scope="module")
def reranker(cuda):
    from rag.reranking import CrossEncoderReranker
    return CrossEncoderReranker({"model_name": "synthetic:tiny-ce", "batch_size": 64})


def test_predict_equals_per_pair_calls_and_follows_a_permutation(cuda, reranker):
    rng = np.random.default_rng(7)
    pairs = list(zip(_texts(rng, 300, 1, 12), _texts(rng, 300, 1, 70)))   # ragged; the long ones are truncated at 64 tokens
    got = reranker.predict(pairs)
    assert got.dtype == np.float32 and got.shape == (300,) and np.isfinite(got).all() and np.unique(got).size > 250
    ids, types = reranker.tokenize_pairs(pairs)
    assert max(len(i) for i in ids) == 64 and min(len(i) for i in ids) < 16
    order = sorted(range(300), key=lambda i: (-len(ids[i]), ids[i]))
    width = {}
    for lo in range(0, 300, 64):
        for i in order[lo:lo + 64]:
            width[i] = len(ids[order[lo]])                                # a batch is padded to its longest pair
    single = np.empty(300, dtype=np.float32)
    for i in range(300):
        b_ids = np.zeros((1, width[i]), dtype=np.int32)
        b_types = np.zeros((1, width[i]), dtype=np.int32)
        b_ids[0, :len(ids[i])], b_types[0, :len(ids[i])] = ids[i], types[i]
        single[i] = reranker.model.score_pairs(b_ids, b_types, np.array([len(ids[i])], dtype=np.int32)).item()
    assert np.array_equal(single.view(np.int32), got.view(np.int32))
    perm = rng.permutation(300)
    assert np.array_equal(reranker.predict([pairs[j] for j in perm]).view(np.int32), got[perm].view(np.int32))
    assert reranker.predict([]).shape == (0,)


@pytest.fixture(scope="module")
def pipelines(cuda):
    """Two pipelines over the same 2048 seeded chunks (synthetic:tiny embeddings), with and without rerank_model, and 132
    questions.  The similarity threshold is the median 7th-best score of the 2 * top_k hits: about half of the lists lose
    hits to it, the others are cut to top_k."""
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    rng = np.random.default_rng(11)
    chunks = [Chunk(text=t + f" {r}", chunk_id=f"c_{r}", start_char=0, end_char=1, page_number=None)
              for r, t in enumerate(_texts(rng, 2048, 6, 30))]
    questions = _texts(rng, 132, 2, 9)

    def build(name, extra):
        p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny", "device": "cuda", "batch_size": 256, "normalize": True},
                         "vector_store": {"collection_name": name},
                         "retrieval": dict({"top_k": 5, "rerank": True, "similarity_threshold": 0.0, "diversity_penalty": 0.0,
                                            "batch_queries": 64}, **extra)})
        p.setup(Stub())
        p.vector_store.create_index(chunks, p.embedding_model.embed_chunks_device(chunks))
        return p

    with_ce, lexical = build("ce-on", {"rerank_model": "synthetic:tiny-ce"}), build("ce-off", {})
    r = lexical.retriever
    seventh = []
    for q in questions:
        hits = r.vector_store.search(query_embedding=r.embedding_model.embed(q), top_k=10)
        seventh.append(r._distance_to_similarity(hits["distances"][0][6]))
    with_ce.retriever.similarity_threshold = lexical.retriever.similarity_threshold = float(np.median(seventh))
    return with_ce, lexical, questions


def test_retriever_reranks_with_the_cross_encoder(cuda, pipelines):
    with_ce, lexical, questions = pipelines
    r = with_ce.retriever
    k = r.top_k
    lists = with_ce.retrieve_batch(questions[:128])
    assert r.last_rerank == {"mode": "cross-encoder", "lists": 128}
    singles = [with_ce.retrieve(q) for q in questions[128:]]
    assert r.last_rerank["mode"] == "cross-encoder"
    lengths = set()
    for q, chunks in zip(questions, lists + singles):
        hits = r.vector_store.search(query_embedding=r.embedding_model.embed(q), top_k=2 * k)
        survivors = r._hits_to_chunks(hits["ids"][0], hits["documents"][0], hits["metadatas"][0], hits["distances"][0])
        rank = {c["chunk_id"]: pos for pos, c in enumerate(survivors)}
        assert len(chunks) == min(k, len(survivors)) and all(c["chunk_id"] in rank for c in chunks)
        lengths.add(len(survivors))
        rr = [c["rerank_score"] for c in chunks]
        assert rr == sorted(rr, reverse=True)
        for a, b in zip(chunks, chunks[1:]):                              # stable: ties keep the search order
            assert a["rerank_score"] > b["rerank_score"] or rank[a["chunk_id"]] < rank[b["chunk_id"]]
        if chunks:
            again = r.cross_encoder.predict([(q, c["text"]) for c in chunks])
            assert np.abs(again - np.array(rr)).max() <= cc.LOGIT_TOL
            assert all(c["score"] >= r.similarity_threshold for c in chunks)
    assert len(lengths) > 1 and max(lengths) > k, lengths                  # the threshold cut some lists short, others were cut to top_k
    # the same pipeline without rerank_model: the token-overlap rule, as before
    lr = lexical.retriever
    assert lr.cross_encoder is None
    plain = lexical.retrieve_batch(questions[:128])
    assert lr.last_rerank == {"mode": "host", "lists": 128}
    for q, chunks in zip(questions[:8], plain):
        assert [(c["chunk_id"], c.get("rerank_score")) for c in chunks] == [(c["chunk_id"], c.get("rerank_score")) for c in lexical.retrieve(q)]
        for c in chunks:
            if "rerank_score" in c:
                hits_q = len(set(q.lower().split()) & set(c["text"].lower().split())) / max(len(set(q.lower().split())), 1)
                assert c["rerank_score"] == c["score"] * 0.7 + hits_q * 0.3
