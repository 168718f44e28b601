"""Cross-encoder re-ranking, host side (no GPU): the fp64 restatement of the pair forward against transformers'
BertForSequenceClassification (tests/golden/crossenc.npz, tools/make_crossenc_golden.py), the C entry point, the torch op and the
binding, argument checks before any HIP call, pair encoding against the installed transformers tokenizer, the model-directory
loader, the activation rule and the retriever's rerank_model key."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _crossenc_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("key", [c[0] for c in cc.CASES])
def test_fp64_restatement_reproduces_transformers(key):
    _, cfg, seed, batch, seq = cc.case(key)
    z = np.load(cc.GOLDEN)
    ids, types, mask = z[key + ".ids"], z[key + ".type_ids"], z[key + ".mask"]
    assert ids.shape == (batch, seq) and int(z[key + ".seed"]) == seed and z[key + ".rows"].size <= cc.HIDDEN_ROWS_CAP
    g_ids, g_types, g_mask = cc.synth_pairs(cfg, batch, seq, seed + 1000)
    assert np.array_equal(ids, g_ids) and np.array_equal(types, g_types) and np.array_equal(mask, g_mask)
    w = cc.make_weights(cfg, seed)
    hidden, pooled, logits = cc.pair_forward_ref(ids, types, mask, w, cfg)
    assert np.abs(logits - z[key + ".logits"]).max() < 1e-9
    assert np.abs(pooled - z[key + ".pooled"]).max() < 1e-9
    assert np.abs(hidden.reshape(-1, cfg.hidden)[z[key + ".rows"]] - z[key + ".hidden"]).max() < 2e-6     # stored as fp32
    # a forward that ignores the type ids is far outside the GPU test's logit bound
    _, _, zeroed = cc.pair_forward_ref(ids, np.zeros_like(types), mask, w, cfg)
    assert np.abs(zeroed - logits).max() > cc.ZEROED_TYPES_GAP >= 10 * cc.LOGIT_TOL
    assert cc.LOGIT_TOL == 4 * max(cc.MODELLED_LOGIT_ERR.values()) and set(cc.MODELLED_LOGIT_ERR) == {c[0] for c in cc.CASES}


def test_cases_cover_what_they_claim():
    z = np.load(cc.GOLDEN)
    t = z["tiny_4x24.type_ids"]
    lens = z["tiny_4x24.mask"].sum(1)
    assert len(set(lens.tolist())) == 4                                        # ragged
    firsts = [int(r.argmax()) if r.any() else -1 for r in t]
    assert firsts.count(-1) == 1 and len(set(firsts)) == 4                       # one all-type-0 row, every boundary elsewhere
    assert z["tiny_3x5.type_ids"].tolist() == [[0, 0, 0, 1, 1]] * 3              # [CLS] a [SEP] b [SEP]
    assert os.path.getsize(cc.GOLDEN) < (1 << 20)


def test_symbol_is_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    import rag._encoder as enc
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_encoder.h")).read(), flags=re.S)
    lib = nat.load()
    assert re.search(r"\bint crs_encoder_score_pairs\s*\(", text), "crs_encoder_score_pairs is not declared"
    assert hasattr(lib, "crs_encoder_score_pairs") and "crs_encoder_score_pairs" in nat.exported_symbols()
    assert re.search(r"typedef struct crs_encoder_head \{\s*const float\* w_pool; const float\* b_pool;\s*const float\* w_cls;\s*"
                     r"const float\* b_cls;\s*int32_t type_rows;\s*int32_t activation;\s*\} crs_encoder_head;", text)
    assert lib.crs_abi_version() == 3
    assert [f[0] for f in enc.EncoderHead._fields_] == ["w_pool", "b_pool", "w_cls", "b_cls", "type_rows", "activation"]
    nat.ops()
    assert str(torch.ops.crs.encoder_score_pairs.default._schema) == \
        ("crs::encoder_score_pairs(Tensor ids, Tensor? type_ids, Tensor lens, Tensor[] weights, Tensor[] head, int[] desc, float ln_eps, "
         "int activation, Tensor(a!) workspace, Tensor(b!) scores, Tensor(c!)? pooled_out, Tensor(d!)? hidden_out) -> ()")
    assert callable(enc.HipEncoder.score_pairs)


def test_argument_validation_without_gpu():
    from rag import _native as nat
    import rag._encoder as enc
    lib = nat.load()
    buf = (ctypes.c_char * 4096)()                     # host memory standing in for device pointers: never dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    desc = enc.EncoderDesc(1000, 64, 2, 4, 256, 64, 1e-12, 1, 0)
    layers = (enc.EncoderLayer * 2)()
    w = enc.EncoderWeights(p, p, p, p, p, ctypes.cast(layers, ctypes.POINTER(enc.EncoderLayer)))

    def call(head, batch=2, seq=8):
        rc = lib.crs_encoder_score_pairs(ctypes.byref(desc), ctypes.byref(w), ctypes.byref(head) if head is not None else None,
                                         p, p, p, batch, seq, p, 1 << 30, p, None, None, None)
        return rc, lib.crs_last_error()

    good = lambda **kw: enc.EncoderHead(**{**dict(w_pool=p, b_pool=p, w_cls=p, b_cls=p, type_rows=2, activation=0), **kw})
    for head, kw, word in ((None, {}, b"null head"), (good(w_pool=None), {}, b"null pointer"), (good(b_pool=None), {}, b"null pointer"),
                           (good(w_cls=None), {}, b"null pointer"), (good(b_cls=None), {}, b"null pointer"),
                           (good(type_rows=0), {}, b"type_rows"), (good(type_rows=-1), {}, b"type_rows"),
                           (good(activation=2), {}, b"activation"), (good(activation=-1), {}, b"activation"),
                           (good(), {"batch": 0}, b"batch"), (good(), {"seq": 65}, b"max_pos"), (good(), {"seq": 0}, b"seq")):
        rc, msg = call(head, **kw)
        assert rc == -1 and word in msg, (kw, rc, msg)


def test_new_kernels_use_no_scratch():
    """The pair head (enc_pair.hip: 2 kernels) and the TYPES instantiations of the embedding kernels (enc_misc.hip: 37 kernels)."""
    import re
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), "--list", "enc_misc.hip", "enc_pair.hip"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout and "39 kernels in 2 files" in r.stdout, r.stdout
    assert "pair_head_kernel" in r.stdout
    for kernel, n in (("embed_ln2_kernel", 3), ("embed_ln2_kernel", 6), ("embed_ln_kernel", 1), ("embed_ln_kernel", 16)):
        # <N, true>, demangled or (where the demangler does not know _Float16) as the mangled name spells it
        assert re.search(r"%s(<%d, true>|ILi%dELb1EE)" % (kernel, n, n), r.stdout), (kernel, n, r.stdout)


# ---- pair encoding ---------------------------------------------------------------------------------------------------------------
def _hf_tokenizer(tmp_path):
    from transformers import BertTokenizer
    from _modeldir import make_vocab
    path = os.path.join(str(tmp_path), "vocab.txt")
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(make_vocab()) + "\n")
    return BertTokenizer(path, do_lower_case=True), path


def test_pair_lengths_rule_is_pinned():
    from rag.tokenizer import pair_lengths
    assert pair_lengths(3, 4, 15) == (3, 4)                          # fits
    assert pair_lengths(3, 30, 15) == (3, 12) and pair_lengths(30, 3, 15) == (12, 3)     # the shorter side stays whole
    assert pair_lengths(30, 20, 15) == (8, 7) and pair_lengths(20, 30, 15) == (7, 8)     # odd budget: the extra token to the longer side
    assert pair_lengths(10, 10, 15) == (7, 8)                        # tie: the extra token to the SECOND text
    assert pair_lengths(10, 10, 14) == (7, 7) and pair_lengths(12, 9, 15) == (8, 7)
    assert pair_lengths(0, 30, 15) == (0, 15) and pair_lengths(30, 0, 15) == (15, 0)


@pytest.mark.parametrize("backend", ["", "python"])
def test_encode_pair_equals_transformers_longest_first(tmp_path, monkeypatch, backend):
    """transformers reads text_pair == "" as "no second text" (a call convention, not tokenisation): an empty second side is
    passed as " " there."""
    from rag.tokenizer import make_wordpiece_tokenizer
    from _modeldir import WORDS
    monkeypatch.setenv("CRS_TOKENIZER", backend)
    hf, vocab_path = _hf_tokenizer(tmp_path)
    tok = make_wordpiece_tokenizer(vocab_path)
    assert type(tok).__name__ == ("WordPieceTokenizer" if backend == "python" else "FastWordPieceTokenizer")
    rng = np.random.default_rng(5)
    words = list(WORDS) + ["jumping", "embedded", "zzzz", "cafes", "Naïve", "fox.", "a-b"]
    text = lambda n: " ".join(rng.choice(words, size=n))
    cases = []
    for _ in range(160):
        cases.append((text(int(rng.integers(0, 25))), text(int(rng.integers(0, 25))), int(rng.integers(5, 40))))
    for n in (1, 4, 9, 16):                                          # equal lengths, budgets that fit, cut one token, cut many
        for seq in (2 * n + 3, 2 * n + 2, 2 * n + 1, n + 4, 6, 5):
            cases.append((" ".join(["fox"] * n), " ".join(["dog"] * n), max(seq, 5)))
    for seq in (5, 8, 20):                                           # one side empty; both
        cases += [("", text(12), seq), (text(12), "", seq), ("", "", seq)]
    for na, nb in ((30, 3), (3, 30), (30, 20), (20, 30), (30, 29), (29, 30)):     # cuts on the first side, the second, both
        cases += [(text(na), text(nb), 18), (text(na), text(nb), 19)]
    assert len(cases) >= 200
    cut = {"a": 0, "b": 0, "both": 0}
    for a, b, seq in cases:
        ids, types = tok.encode_pair(a, b, seq)
        want = hf(a, b if b else " ", truncation="longest_first", max_length=seq)
        assert ids == want["input_ids"] and types == want["token_type_ids"], (a, b, seq)
        na, nb = len(tok.encode_body(a)), len(tok.encode_body(b))
        ka, kb = types.count(0) - 2, types.count(1) - 1
        assert len(ids) <= seq and ids[0] == tok.cls_id and ids[ka + 1] == tok.sep_id and ids[-1] == tok.sep_id
        cut["both" if ka < na and kb < nb else "a" if ka < na else "b" if kb < nb else "both"] += ka < na or kb < nb
    assert min(cut.values()) >= 10, cut


def test_hash_tokenizer_encodes_pairs():
    from rag.tokenizer import HashTokenizer
    tok = HashTokenizer(1000)
    ids, types = tok.encode_pair("alpha beta", "gamma delta epsilon", 64)
    assert ids[0] == tok.cls_id and ids[3] == ids[-1] == tok.sep_id and types == [0, 0, 0, 0, 1, 1, 1, 1]
    assert ids[1:3] == tok.encode("alpha beta", 64)[1:-1] and ids[4:7] == tok.encode("gamma delta epsilon", 64)[1:-1]
    ids, types = tok.encode_pair("a " * 40, "b " * 50, 16)
    assert len(ids) == 16 and types.count(0) == 8 and types.count(1) == 8          # 13 tokens to share: 6 + 7, the longer side 7
    with pytest.raises(ValueError):
        tok.encode_pair("a", "b", 4)


# ---- the loader ------------------------------------------------------------------------------------------------------------------
def test_loader_reads_a_cross_encoder_directory(tmp_path):
    from rag.reranking import CrossEncoderReranker, load_cross_encoder_dir
    from _modeldir import make_vocab
    raw = cc.write_crossenc_dir(str(tmp_path))
    shape, w, tok, cfg = load_cross_encoder_dir(str(tmp_path))
    assert (shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.ffn, shape.max_pos, shape.max_seq) == \
        (len(make_vocab()), 64, 2, 4, 128, 64, 64)
    for name in cc.HEAD + (cc.TYPE_EMB, "encoder.layer.1.output.dense.weight"):
        assert np.array_equal(w[name], raw[name]), name
    assert w[cc.HEAD[2]].shape == (1, 64) and w[cc.TYPE_EMB].shape == (2, 64)
    assert (tok.cls_id, tok.sep_id, tok.pad_id) == (2, 3, 0)
    r = CrossEncoderReranker({"model_path": str(tmp_path), "max_seq_length": 32, "batch_size": 16})
    assert r.shape.max_seq == 32 and r.batch_size == 16 and r.activation == "sigmoid"
    ids, types = r.tokenize_pairs([("the quick fox", "lazy dog jumps"), ("fox", "")])
    assert ids[0] == [2] + tok.encode_body("the quick fox") + [3] + tok.encode_body("lazy dog jumps") + [3]
    assert types[0] == [0] * 5 + [1] * 4 and ids[1][-2:] == [3, 3] and types[1][-1] == 1
    assert CrossEncoderReranker(str(tmp_path)).model_name == str(tmp_path)       # a string is the model name


@pytest.mark.parametrize("kw,word", [({"labels": 2}, "2 labels"), ({"pooler": False}, "pooler.dense.weight"),
                                     ({"classifier": False}, "classifier.weight"), ({"model_type": "roberta"}, "roberta")])
def test_loader_names_what_it_cannot_load(tmp_path, kw, word):
    from rag.reranking import CrossEncoderReranker
    cc.write_crossenc_dir(str(tmp_path), **kw)
    with pytest.raises(NotImplementedError, match=word):
        CrossEncoderReranker({"model_path": str(tmp_path)})


@pytest.mark.parametrize("fn,setting,want", [(None, "auto", "sigmoid"), ("torch.nn.modules.linear.Identity", "auto", "identity"),
                                             ("torch.nn.modules.activation.Sigmoid", "auto", "sigmoid"),
                                             ("torch.nn.modules.linear.Identity", "sigmoid", "sigmoid"), (None, "identity", "identity")])
def test_activation_auto_follows_the_config_key(tmp_path, fn, setting, want):
    from rag.reranking import CrossEncoderReranker
    cc.write_crossenc_dir(str(tmp_path), activation_fn=fn)
    assert CrossEncoderReranker({"model_path": str(tmp_path), "activation": setting}).activation == want
    with pytest.raises(ValueError, match="activation"):
        CrossEncoderReranker({"model_path": str(tmp_path), "activation": "softmax"})


def test_synthetic_cross_encoders():
    from rag.reranking import CrossEncoderReranker, _KNOWN_CE
    r = CrossEncoderReranker("synthetic:tiny-ce")
    s = r.shape
    assert (s.hidden, s.layers, s.heads, s.max_pos, s.max_seq) == (64, 2, 4, 64, 64) and r.batch_size == 128 and r.activation == "identity"
    assert r._weights[cc.TYPE_EMB].shape == (2, 64) and r._weights[cc.TYPE_EMB][1].any() and r._weights[cc.HEAD[2]].shape == (1, 64)
    m = _KNOWN_CE["minilm-ce"]
    assert [m[k] for k in ("vocab_size", "hidden", "layers", "heads", "ffn", "max_pos")] == [30522, 384, 6, 12, 1536, 512]


# ---- the retriever's key ---------------------------------------------------------------------------------------------------------
class _NoStore:
    collection = None


def test_retriever_without_rerank_model_is_unchanged_and_an_unknown_one_raises():
    from rag.retrieval import ContextRetriever
    r = ContextRetriever(_NoStore(), None, {"rerank": True})
    assert r.cross_encoder is None and r.last_rerank == {"mode": "host", "lists": 0}
    chunks = [{"text": "alpha beta", "score": 0.5, "chunk_id": "a"}, {"text": "gamma", "score": 0.6, "chunk_id": "b"},
              {"text": "alpha", "score": 0.4, "chunk_id": "c"}]
    out = r._post_process("alpha beta", [dict(c) for c in chunks], 2)
    assert [c["chunk_id"] for c in out] == ["a", "c"] and out[0]["rerank_score"] == 0.5 * 0.7 + 0.3     # the token-overlap rule
    r = ContextRetriever(_NoStore(), None, {"rerank": True, "rerank_model": {"model_name": "synthetic:tiny-ce", "batch_size": 32}})
    assert r.cross_encoder.batch_size == 32 and r.cross_encoder.model_name == "synthetic:tiny-ce"
    assert ContextRetriever(_NoStore(), None, {"rerank_model": "synthetic:tiny-ce"}).cross_encoder is not None
    with pytest.raises(FileNotFoundError, match="no-such-model"):
        ContextRetriever(_NoStore(), None, {"rerank": True, "rerank_model": "cross-encoder/no-such-model"})
