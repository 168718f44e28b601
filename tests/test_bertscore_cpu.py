"""CPU: the BERTScore matching entry point (crs_token_match, csrc/token_match.hip) is declared, exported and bound, the ABI
version did not move, its argument checks answer CRS_EINVAL before any HIP call, its kernel uses no scratch; rag.bertscore's
configuration errors, RoBERTa loader and tokenizer, token weights; the golden file separates layer L from layer L - 1."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _bertscore_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_is_declared_exported_and_bound():
    import torch
    from rag import _native as nat
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_hip.h")).read(), flags=re.S)
    lib = nat.load()
    assert re.search(r"\bint crs_token_match\s*\(", header), "crs_token_match not declared in include/crs_hip.h"
    assert hasattr(lib, "crs_token_match"), "crs_token_match not exported"
    assert "crs_token_match" in nat.exported_symbols()
    assert lib.crs_abi_version() == 3
    declared = set(re.findall(r"\b(crs_\w+)\s*\(", header))
    assert set(nat._SIGNATURES) & declared == declared, sorted(declared - set(nat._SIGNATURES))
    assert hasattr(nat.ops(), "token_match_out") and callable(nat.token_match)
    assert str(torch.ops.crs.token_match_out.default._schema) == \
        "crs::token_match_out(Tensor a, Tensor len_a, Tensor b, Tensor len_b, Tensor? w_a, Tensor? w_b, Tensor(a!) out) -> ()"


def test_argument_validation_without_gpu():
    from rag import _native as nat
    lib = nat.load()
    buf = (ctypes.c_char * 4096)()                     # host memory standing in for device pointers: never dereferenced
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)             # 16-byte aligned
    odd = ctypes.c_void_p(p.value + 4)
    EINVAL = -1

    # crs_token_match(a, len_a, seq_a, b, len_b, seq_b, n_pairs, hidden, w_a, w_b, out, stream)
    def call(a=p, len_a=p, seq_a=24, b=p, len_b=p, seq_b=17, n_pairs=4, hidden=384, w_a=None, w_b=None, out=p):
        return lib.crs_token_match(a, len_a, seq_a, b, len_b, seq_b, n_pairs, hidden, w_a, w_b, out, None)

    for bad, word in (({"seq_a": 0}, b"seq_a"), ({"seq_a": 513}, b"seq_a"), ({"seq_a": -1}, b"seq_a"),
                      ({"seq_b": 0}, b"seq_b"), ({"seq_b": 513}, b"seq_b"),
                      ({"hidden": 0}, b"hidden"), ({"hidden": 32}, b"hidden"), ({"hidden": 100}, b"hidden"), ({"hidden": 1088}, b"hidden"),
                      ({"hidden": -64}, b"hidden"), ({"n_pairs": -1}, b"n_pairs"),
                      ({"a": None}, b"a_dev"), ({"len_a": None}, b"len_a_dev"), ({"b": None}, b"b_dev"), ({"len_b": None}, b"len_b_dev"),
                      ({"out": None}, b"out_dev"), ({"a": odd}, b"a_dev"), ({"b": odd}, b"b_dev")):
        assert call(**bad) == EINVAL, bad
        assert word in lib.crs_last_error(), (bad, lib.crs_last_error())
    # the checks come before the empty-launch return, and nothing is launched for no pairs
    assert call(n_pairs=0, seq_a=600) == EINVAL
    assert call(n_pairs=0) == 0
    assert call(n_pairs=0, w_a=p, w_b=p, seq_a=512, seq_b=1, hidden=1024) == 0


def test_kernel_uses_no_scratch():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_resources.py"), "token_match.hip"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "0 violation(s)" in r.stdout and "1 kernels in 1 files" in r.stdout, r.stdout


# ---- configuration -----------------------------------------------------------------------------------------------
def test_layer_table_and_exports():
    import rag
    from rag import bertscore as bs
    assert bs.MODEL_LAYERS == {"bert-base-uncased": 9, "bert-large-uncased": 18, "roberta-base": 10, "roberta-large": 17}
    assert bs.LANG_MODELS["en"] == "roberta-large"
    assert rag.BertScorer is bs.BertScorer and "BertScorer" in rag.__all__
    assert "unpinned" in bs.__doc__.lower() and "model2layers" in bs.__doc__


def test_config_errors_come_before_the_gpu(tmp_path, monkeypatch):
    from rag import bertscore as bs
    monkeypatch.delenv("CRS_MODEL_DIR", raising=False)
    with pytest.raises(ValueError, match="pass num_layers"):
        bs.BertScorer({"model_name": "synthetic:tiny"})
    for bad in (0, 3, -1):
        with pytest.raises(ValueError, match=r"num_layers must be in 1\.\.2"):
            bs.BertScorer({"model_name": "synthetic:tiny", "num_layers": bad})
    with pytest.raises(NotImplementedError, match="baseline"):
        bs.BertScorer({"model_name": "synthetic:tiny", "num_layers": 2, "rescale_with_baseline": True})
    with pytest.raises(NotImplementedError, match="baseline"):
        bs.score(["a"], ["b"], model_type="synthetic:tiny", num_layers=2, rescale_with_baseline=True)
    with pytest.raises(FileNotFoundError, match="No local checkpoint for 'roberta-large'"):
        bs.score(["a"], ["b"], lang="en")
    with pytest.raises(ValueError, match="lang 'xx'"):
        bs.score(["a"], ["b"], lang="xx")
    with pytest.raises(ValueError, match="idf must be"):
        bs.BertScorer({"model_name": "synthetic:tiny", "num_layers": 2, "idf": True})
    d = tmp_path / "distil"
    d.mkdir()
    (d / "config.json").write_text(json.dumps({"model_type": "distilbert"}))
    (d / "model.safetensors").write_bytes(b"")
    with pytest.raises(NotImplementedError, match="model_type 'distilbert' is not supported by BertScorer"):
        bs.BertScorer({"model_path": str(d), "model_name": "distil", "num_layers": 1})
    # CRS_MODEL_DIR/<basename> resolves like EmbeddingModel's
    monkeypatch.setenv("CRS_MODEL_DIR", str(tmp_path))
    with pytest.raises(NotImplementedError, match="distilbert"):
        bs.BertScorer({"model_name": "someone/distil", "num_layers": 1})


# ---- RoBERTa directory: tokenizer and loader ---------------------------------------------------------------------
CORPUS = ["The quick brown fox jumps over the lazy dog.", "Retrieval augmented generation answers questions from documents.",
          "BERTScore compares candidate and reference sentences token by token.", "Numbers like 3.14159 and 2024 appear, too!",
          "café naïve über straße", "Tokens  with   odd spacing\tand\nnewlines", "An answer: yes, no; maybe?"] * 3
TEXTS = ["", "The lazy dog answers questions.", "  leading and trailing spaces  ", "unseen wörds \U0001F600 and symbols #@!",
         "<s> literal specials </s> <mask> in text", "quick " * 200, "a"]
SPECIALS = ["<s>", "<pad>", "</s>", "<unk>", "<mask>"]


def _write_roberta_dir(path, with_weights=False):
    from tokenizers import Tokenizer, pre_tokenizers, trainers
    from tokenizers.models import BPE
    tok = Tokenizer(BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    trainer = trainers.BpeTrainer(vocab_size=420, special_tokens=SPECIALS, initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tok.train_from_iterator(iter(CORPUS), trainer=trainer)
    os.makedirs(path, exist_ok=True)
    tok.model.save(str(path))                          # vocab.json + merges.txt
    vocab = tok.get_vocab_size()
    cfg = {"model_type": "roberta", "vocab_size": vocab, "hidden_size": 64, "num_hidden_layers": 2, "num_attention_heads": 4,
           "intermediate_size": 128, "max_position_embeddings": 34, "type_vocab_size": 1, "layer_norm_eps": 1e-5,
           "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2}
    with open(os.path.join(path, "config.json"), "w") as fh:
        json.dump(cfg, fh)
    if with_weights:
        from safetensors.numpy import save_file
        c = bc.BsCfg("t", "roberta", vocab, 64, 2, 4, 128, 34, ln_eps=1e-5, pad_id=1, cls_id=0, sep_id=2, pos_offset=2, type_rows=1)
        w = {"roberta." + k: v for k, v in bc.make_weights(c, 7).items()}
        w["lm_head.bias"] = np.zeros(vocab, dtype=np.float32)
        save_file(w, os.path.join(path, "model.safetensors"))
    return cfg


@pytest.mark.parametrize("max_len", [32, 12])
def test_roberta_tokenizer_matches_transformers(tmp_path, max_len):
    """The ids of transformers' `tokenizers`-backed RoBERTa tokenizer for the same directory.  In transformers 5 that class is
    `RobertaTokenizer` (`RobertaTokenizerFast` remains as a legacy name whose constructor no longer reads vocab.json +
    merges.txt); with transformers 4 it is `RobertaTokenizerFast`."""
    import transformers
    from rag import bertscore as bs
    d = str(tmp_path / "rob")
    cfg = _write_roberta_dir(d)
    cls = transformers.RobertaTokenizer if int(transformers.__version__.split(".")[0]) >= 5 else transformers.RobertaTokenizerFast
    hf = cls.from_pretrained(d, local_files_only=True)
    assert hf.is_fast
    want = [hf(t, truncation=True, max_length=max_len)["input_ids"] for t in TEXTS]
    assert want[0] == [0, 2] and len(want[5]) == max_len and want[5][-1] == 2
    tok = bs._roberta_tokenizer(d, cfg)                # vocab.json + merges.txt
    assert (tok.cls_id, tok.sep_id, tok.pad_id) == (0, 2, 1)
    assert tok.encode_batch(TEXTS, max_len) == want
    assert [tok.encode(t, max_len) for t in TEXTS] == want
    hf.backend_tokenizer.save(os.path.join(d, "tokenizer.json"))
    tok2 = bs._roberta_tokenizer(d, cfg)               # tokenizer.json as shipped
    assert tok2.encode_batch(TEXTS, max_len) == want


def test_roberta_tokenizer_needs_the_library(tmp_path, monkeypatch):
    from rag import bertscore as bs
    d = str(tmp_path / "rob")
    cfg = _write_roberta_dir(d)
    monkeypatch.setitem(sys.modules, "tokenizers", None)
    with pytest.raises(NotImplementedError, match="tokenizers"):
        bs._roberta_tokenizer(d, cfg)


def test_load_hf_dir_roberta(tmp_path):
    from rag import bertscore as bs
    d = str(tmp_path / "rob")
    cfg = _write_roberta_dir(d, with_weights=True)
    shape, weights, tok = bs.load_hf_dir(d)
    assert (shape.pos_offset, shape.max_pos, shape.max_seq, shape.layers, shape.ln_eps) == (2, 34, 32, 2, 1e-5)
    assert (shape.hidden, shape.heads, shape.ffn, shape.vocab_size, shape.rel_buckets) == (64, 4, 128, cfg["vocab_size"], 0)
    assert weights["embeddings.token_type_embeddings.weight"].shape == (1, 64)
    assert weights["embeddings.position_embeddings.weight"].shape == (34, 64)
    assert "encoder.layer.1.output.LayerNorm.bias" in weights and not any(k.startswith("roberta.") for k in weights)
    assert tok.encode("", 32) == [0, 2]
    # the embedding and cross-encoder loaders still reject the type
    from rag.embedding import _load_local_dir
    with pytest.raises(NotImplementedError, match="roberta"):
        _load_local_dir(d)


# ---- token weights -----------------------------------------------------------------------------------------------
def test_idf_and_special_token_weights_match_a_hand_computation():
    from rag import bertscore as bs
    CLS, SEP = 1, 2
    refs = [[CLS, 10, 11, 12, SEP], [CLS, 10, 11, SEP], [CLS, 10, 13, 13, SEP], [CLS, 14, SEP], [CLS, SEP]]
    table, default = bs.idf_weights(refs, (CLS, SEP))
    n = 5
    assert default == math.log(n + 1)
    want = {10: math.log(6 / 4), 11: math.log(6 / 3), 12: math.log(6 / 2), 13: math.log(6 / 2), 14: math.log(6 / 2), CLS: 0.0, SEP: 0.0}
    assert table == want                                # 13 twice in one sentence counts once
    assert bs.sentence_weights([CLS, 10, 99, 13, SEP], (table, default)) == [0.0, math.log(1.5), math.log(6), math.log(3), 0.0]
    assert bs.sentence_weights([CLS, 10, 99, 13, SEP]) == [0.0, 1.0, 1.0, 1.0, 0.0]
    assert bs.sentence_weights([CLS, SEP]) == [0.0, 0.0] and bs.sentence_weights([]) == []
    # a body token that happens to equal a special id keeps the table's 0; position decides only first and last
    assert bs.sentence_weights([CLS, SEP, 10, SEP], (table, default)) == [0.0, 0.0, math.log(1.5), 0.0]


# ---- golden file -------------------------------------------------------------------------------------------------
def test_golden_separates_the_layers_and_matches_the_cases():
    g = np.load(bc.GOLDEN)
    assert os.path.getsize(bc.GOLDEN) < (1 << 20)
    ceilings = []
    for key, cfg, seed, pairs, seq_a, seq_b in bc.CASES:
        ids_a, mask_a, ids_b, mask_b = bc.synth_pairs(cfg, pairs, seq_a, seq_b, seed + 1000)
        assert np.array_equal(g[key + ".ids_a"], ids_a) and np.array_equal(g[key + ".ids_b"], ids_b)
        assert np.array_equal(g[key + ".mask_a"], mask_a) and np.array_equal(g[key + ".mask_b"], mask_b)
        prf = g[key + ".prf"]
        assert prf.shape == (pairs, 3) and prf.dtype == np.float64 and np.isfinite(prf).all()
        assert mask_a[0].all() and mask_b[0].all()
        if pairs > 1:
            assert not mask_a[1:].all() and not mask_b[1:].all()       # ragged apart from row 0
        ceilings.append(bc.e2e_ceiling(cfg.hidden, float(g[key + ".min_norm"])))
    assert 0 < bc.E2E_TOL <= min(ceilings)
    for key in bc.LAYER_CHECK:
        gap = np.abs(g[key + ".prf"][:, 2] - g[key + ".prf_prev"][:, 2]).min()
        assert gap >= 10 * bc.E2E_TOL, (key, gap)
    for key in ("tiny_4", "mid_3"):
        assert np.abs(g[key + ".prf"][:, 0] - g[key + ".prf"][:, 1]).max() >= 0.039      # P and R are told apart
