"""CPU: loading XLM-RoBERTa checkpoints.  rag.embedding._load_local_dir and rag.reranking.load_cross_encoder_dir on written
directories (shape, tensor names, tokeniser), the pair format against the `tokenizers` library, and what still raises."""
import json

import numpy as np
import pytest

import _unigram_cases as uc
import _xlmr_cases as xc

N_VOCAB = len(uc.vocab())


def test_embedding_loader_reads_an_xlmr_directory(tmp_path):
    from rag.embedding import _load_local_dir
    from rag.tokenizer import FastUnigramTokenizer, UnigramTokenizer
    cfg = xc.write_xlmr_dir(str(tmp_path), uc.NFKC_JSON, seed=3, vocab_size=N_VOCAB)
    shape, weights, tok, pre_lower, has_normalize = _load_local_dir(str(tmp_path))
    assert (shape.pos_offset, shape.rel_buckets, shape.max_seq, shape.max_pos, shape.ln_eps) == (2, 0, 64, 66, 1e-5)
    assert (shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.ffn, shape.pooling) == (N_VOCAB, 64, 2, 4, 256, "mean")
    assert not pre_lower and has_normalize
    want = xc.make_weights(cfg, 3)
    assert set(weights) == set(want) and not any("roberta" in k for k in weights)
    for k, v in want.items():
        assert np.array_equal(weights[k], v), k
    assert weights["embeddings.token_type_embeddings.weight"].shape == (1, 64)
    assert weights["embeddings.token_type_embeddings.weight"].any()            # as shipped, not zeroed
    assert isinstance(tok, (FastUnigramTokenizer, UnigramTokenizer))
    assert (tok.cls_id, tok.sep_id, tok.pad_id) == (0, 2, 1) and (tok.pair_seps, tok.pair_typed) == (2, False)
    assert tok.encode("ab", 8) == uc.load_json(uc.IDS_JSON)["ids"]["nfkc.8"][uc.load_json(uc.IDS_JSON)["names"].index("tie")]


def test_max_seq_leaves_room_for_the_position_offset(tmp_path):
    from rag.embedding import _load_local_dir
    xc.write_xlmr_dir(str(tmp_path), uc.NFKC_JSON, vocab_size=N_VOCAB)
    with open(tmp_path / "sentence_bert_config.json", "w") as fh:
        json.dump({"max_seq_length": 512}, fh)
    shape = _load_local_dir(str(tmp_path))[0]
    assert shape.max_seq == 66 - 2


def test_python_tokeniser_is_the_fallback(tmp_path, monkeypatch):
    from rag.tokenizer import UnigramTokenizer, tokenizer_from_model_dir
    xc.write_xlmr_dir(str(tmp_path), uc.NFKC_JSON, vocab_size=N_VOCAB)
    monkeypatch.setenv("CRS_TOKENIZER", "python")
    tok = tokenizer_from_model_dir(str(tmp_path))
    assert isinstance(tok, UnigramTokenizer) and tok.encode("axyb", 8) == [0, tok.pieces[uc.META + "a"][0], 3, tok.pieces["b"][0], 2]


def test_cross_encoder_loader_maps_the_head(tmp_path):
    from rag.reranking import CrossEncoderReranker, load_cross_encoder_dir
    cfg = xc.write_xlmr_dir(str(tmp_path), uc.NFKC_JSON, seed=5, head=True, vocab_size=N_VOCAB)
    shape, weights, tok, conf = load_cross_encoder_dir(str(tmp_path))
    assert (shape.pos_offset, shape.max_seq, shape.max_pos, shape.pooling, shape.ln_eps) == (2, 64, 66, "cls", 1e-5)
    want = xc.make_ce_weights(cfg, 5)
    assert set(weights) == set(want)
    for k, v in want.items():
        assert np.array_equal(weights[k], v), k
    assert weights["classifier.weight"].shape == (1, 64) and weights["pooler.dense.weight"].shape == (64, 64)
    assert (tok.pair_seps, tok.pair_typed) == (2, False)
    rr = CrossEncoderReranker({"model_name": str(tmp_path), "max_seq_length": 512})
    assert rr.shape.max_seq == 64 and rr.activation == "identity"


def test_pair_ids_equal_the_library(tmp_path):
    """<s> a </s></s> b </s>, every type id 0, `longest_first` over a budget of max_seq - 4, at widths that cut one side, both
    sides and neither."""
    pytest.importorskip("tokenizers")
    from tokenizers import Tokenizer
    from rag.reranking import CrossEncoderReranker
    xc.write_xlmr_dir(str(tmp_path), uc.NFKC_JSON, head=True, vocab_size=N_VOCAB)
    lib = Tokenizer.from_file(uc.NFKC_JSON)
    a = "hello world the quick fox ab cd axyb"
    b = "the fox is in the model tokens of hello"
    c = "ab"
    n_a, n_b = len(lib.encode(a, add_special_tokens=False).ids), len(lib.encode(b, add_special_tokens=False).ids)
    for max_seq in (5, 6, 9, 12, 13, 24, 64):
        rr = CrossEncoderReranker({"model_name": str(tmp_path), "max_seq_length": max_seq})
        lib.enable_truncation(max_length=max_seq, strategy="longest_first")
        for x, y in ((a, b), (b, a), (a, c), (c, a), (a, a)):
            ids, types = rr.tokenize_pairs([(x, y)])
            want = lib.encode(x, y)
            assert ids[0] == want.ids and types[0] == want.type_ids == [0] * len(ids[0]), (max_seq, x, y)
            assert rr.tokenizer.encode_pair(x, y, max_seq) == (want.ids, want.type_ids)
        assert len(rr._tokens[a][0]) == min(n_a, max_seq - 4) and rr._tokens[a][1] == n_a
    # 9, 12 and 13 cut both sides (the shorter one is longer than half the budget), 24 the longer one, 64 neither
    assert n_a != n_b and min(n_a, n_b) > (13 - 4) // 2 and min(n_a, n_b) <= (24 - 4) // 2 < max(n_a, n_b) and n_a + n_b + 4 <= 64


def test_bert_pairs_keep_three_special_tokens():
    from rag.tokenizer import HashTokenizer, join_pair
    ids, types = join_pair([5, 6, 7, 8], [9, 10, 11], 1, 2, 8)
    assert ids == [1, 5, 6, 7, 2, 9, 10, 2] and types == [0, 0, 0, 0, 0, 1, 1, 1]
    ids, types = join_pair([5, 6, 7, 8], [9, 10, 11], 0, 2, 8, seps=2, typed=False)
    assert ids == [0, 5, 6, 2, 2, 9, 10, 2] and types == [0] * 8
    assert HashTokenizer(1000).encode_pair("a b", "c", 16)[1] == [0, 0, 0, 0, 1, 1]


def test_roberta_and_two_label_classifiers_still_raise(tmp_path):
    from rag.embedding import _load_local_dir
    from rag.reranking import load_cross_encoder_dir
    xc.write_xlmr_dir(str(tmp_path / "emb"), uc.NFKC_JSON, model_type="roberta", vocab_size=N_VOCAB)
    with pytest.raises(NotImplementedError, match=r"roberta.*bert, mpnet and xlm-roberta"):
        _load_local_dir(str(tmp_path / "emb"))
    xc.write_xlmr_dir(str(tmp_path / "ce"), uc.NFKC_JSON, head=True, model_type="roberta", vocab_size=N_VOCAB)
    with pytest.raises(NotImplementedError, match=r"roberta.*bert and xlm-roberta"):
        load_cross_encoder_dir(str(tmp_path / "ce"))
    xc.write_xlmr_dir(str(tmp_path / "two"), uc.NFKC_JSON, head=True, labels=2, vocab_size=N_VOCAB)
    with pytest.raises(NotImplementedError, match="2 labels"):
        load_cross_encoder_dir(str(tmp_path / "two"))


def test_synthetic_names():
    from rag.embedding import _KNOWN
    from rag.reranking import _KNOWN_CE, CrossEncoderReranker
    assert _KNOWN["tiny-xlmr"] == dict(vocab_size=1000, hidden=64, layers=2, heads=4, ffn=256, max_pos=66, pooling="mean", max_seq=64,
                                       ln_eps=1e-5, pos_offset=2)
    for name, vocab, hidden, ffn, max_seq in (("multilingual-minilm", 250037, 384, 1536, 128), ("multilingual-e5-base", 250002, 768, 3072, 512)):
        k = _KNOWN[name]
        assert (k["vocab_size"], k["hidden"], k["layers"], k["heads"], k["ffn"], k["max_pos"], k["pooling"], k["max_seq"], k["pos_offset"]) == \
            (vocab, hidden, 12, 12, ffn, 514, "mean", max_seq, 2)
    assert _KNOWN_CE["tiny-xlmr-ce"]["pos_offset"] == 2 and _KNOWN_CE["tiny-xlmr-ce"]["max_pos"] == 66
    rr = CrossEncoderReranker("synthetic:tiny-xlmr-ce")
    assert (rr.shape.pos_offset, rr.shape.max_seq) == (2, 64)
    ids, types = rr.tokenize_pairs([("alpha beta", "gamma")])
    assert ids[0][0] == 0 and ids[0][3:5] == [2, 2] and ids[0][-1] == 2 and len(ids[0]) == 7 and types[0] == [0] * 7
