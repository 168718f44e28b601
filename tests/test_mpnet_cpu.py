"""MPNet support, host side (no GPU): the bucket rule and the resolved bias table against transformers' own (committed in
tests/golden/encoder_mpnet.npz by tools/make_mpnet_golden.py), the _ex entry points of the C ABI, the loader and the
tokenizers on an MPNet model directory, and BERT directories resolving to the ids they always had."""
import json
import os
import re

import numpy as np
import pytest

import _mpnet_cases as mc
from _modeldir import make_vocab, write_model_dir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bucket_function_equals_transformers_at_all_1023_offsets():
    from rag._encoder import relative_position_bucket
    z = np.load(mc.GOLDEN)
    assert z["bucket_offsets"].tolist() == list(range(-511, 512))
    got = relative_position_bucket(z["bucket_offsets"], 32, 128)
    assert np.array_equal(got, z["bucket_index"])
    # the rule as the model card states it: |n| < 8 exact, keys after the query + 16, clamp at 15 from distance 128 on
    at = dict(zip(z["bucket_offsets"].tolist(), got.tolist()))
    assert [at[-d] for d in range(8)] == list(range(8)) and [at[d] for d in range(1, 8)] == [16 + d for d in range(1, 8)]
    assert at[-127] == 15 and at[-511] == 15 and at[511] == 31 and at[-8] == 8 and at[8] == 24


def test_bias_table_is_indexed_by_key_minus_query():
    from rag._encoder import relative_bias_table
    w = np.arange(32 * 3, dtype=np.float32).reshape(32, 3)
    t = relative_bias_table(w, 10, 32)
    assert t.shape == (3, 19) and t.dtype == np.float32
    assert t[1, 9] == w[0, 1] and t[1, 9 - 2] == w[2, 1] and t[1, 9 + 2] == w[18, 1] and t[2, 18] == w[16 + 8, 2]
    with pytest.raises(ValueError):
        relative_bias_table(w, 10, 16)


@pytest.mark.parametrize("key", ["tiny_4x24", "tiny_3x5", "mid_3x80"])
def test_host_table_and_name_mapping_reproduce_transformers_in_fp64(key):
    """The resolved table, the position offset and the zero token-type row, through an fp64 restatement of what the library
    computes: MPNetModel's hidden states to fp32 storage error."""
    from rag._encoder import relative_bias_table
    _, cfg, seed, _, _ = next(c for c in mc.CASES if c[0] == key)
    z = np.load(mc.GOLDEN)
    w = mc.make_weights(cfg, seed)
    table = relative_bias_table(w[mc.REL_BIAS], cfg.max_seq, mc.BUCKETS)
    hid = mc.encode_ref(z[key + ".ids"], z[key + ".mask"], w, cfg, table).reshape(-1, cfg.hidden)[z[key + ".rows"]]
    assert np.abs(hid - z[key + ".hidden"]).max() < 2e-6
    flipped = mc.encode_ref(z[key + ".ids"], z[key + ".mask"], w, cfg, table[:, ::-1].copy()).reshape(-1, cfg.hidden)[z[key + ".rows"]]
    assert np.abs(flipped - z[key + ".hidden"]).max() > 3e-2, "the hidden states do not see a transposed bias index"


def test_ex_entry_points_are_declared_exported_and_bound():
    from rag import _native as nat
    import rag._encoder as enc
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crs_encoder.h")).read(), flags=re.S)
    lib = nat.load()
    for name in ("crs_encoder_forward_ex", "crs_encoder_forward_queries_ex"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared"
        assert hasattr(lib, name) and name in nat.exported_symbols()
    assert "const crs_encoder_ext* ext" in text and re.search(r"const float\* rel_bias_dev;\s*int32_t rel_span;", text)
    assert lib.crs_abi_version() == 3
    assert [f[0] for f in enc.EncoderExt._fields_] == ["rel_bias_dev", "rel_span"]
    assert hasattr(nat.ops(), "encoder_forward_ex") and hasattr(nat.ops(), "encoder_forward")
    s = enc.ModelShape(1000, 64, 2, 4, 256, 64)
    assert (s.rel_buckets, s.rel_max_distance, s.pos_offset) == (0, 128, 0)


# ---- an MPNet model directory, written by hand (no transformers) -----------------------------------------------------------------
def _mpnet_vocab():
    return ["<s>", "<pad>", "</s>", "<unk>"] + [t for t in make_vocab() if t not in ("[PAD]", "[CLS]", "[SEP]", "[MASK]")] + ["<mask>"]


def write_mpnet_dir(path, *, prefix="mpnet.", model_type="mpnet", tokenizer_json=False, hidden=64, layers=2, heads=4, ffn=128,
                    max_pos=66, max_seq=48, seed=0):
    from safetensors.numpy import save_file
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    vocab = _mpnet_vocab()
    cfg = {"architectures": ["MPNetModel"], "model_type": model_type, "vocab_size": len(vocab), "hidden_size": hidden,
           "num_hidden_layers": layers, "num_attention_heads": heads, "intermediate_size": ffn, "max_position_embeddings": max_pos,
           "layer_norm_eps": 1e-5, "relative_attention_num_buckets": 32, "pad_token_id": 1, "bos_token_id": 0, "eos_token_id": 2,
           "hidden_act": "gelu"}
    json.dump(cfg, open(os.path.join(path, "config.json"), "w"))
    json.dump({"max_seq_length": max_seq, "do_lower_case": False}, open(os.path.join(path, "sentence_bert_config.json"), "w"))
    json.dump({"do_lower_case": True, "tokenizer_class": "MPNetTokenizer"}, open(os.path.join(path, "tokenizer_config.json"), "w"))
    json.dump({"bos_token": "<s>", "eos_token": "</s>", "cls_token": {"content": "<s>", "lstrip": False}, "sep_token": "</s>",
               "pad_token": "<pad>", "unk_token": "[UNK]", "mask_token": "<mask>"}, open(os.path.join(path, "special_tokens_map.json"), "w"))
    json.dump({"word_embedding_dimension": hidden, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
               "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(path, "1_Pooling", "config.json"), "w"))
    with open(os.path.join(path, "vocab.txt"), "w", encoding="utf-8") as fh:
        fh.write("\n".join(vocab) + "\n")
    if tokenizer_json:
        from rag.tokenizer import FastWordPieceTokenizer
        FastWordPieceTokenizer.from_vocab({t: i for i, t in enumerate(vocab)}, unk="[UNK]", cls_tok="<s>", sep="</s>",
                                          pad="<pad>")._tok.save(os.path.join(path, "tokenizer.json"))
    rng = np.random.default_rng(seed)
    h, f = hidden, ffn
    shapes = {"embeddings.word_embeddings.weight": (len(vocab), h), "embeddings.position_embeddings.weight": (max_pos, h),
              "embeddings.LayerNorm.weight": (h,), "embeddings.LayerNorm.bias": (h,), "encoder.relative_attention_bias.weight": (32, heads),
              "pooler.dense.weight": (h, h)}
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for n in "qkvo":
            shapes[p + f"attention.attn.{n}.weight"], shapes[p + f"attention.attn.{n}.bias"] = (h, h), (h,)
        shapes.update({p + "attention.LayerNorm.weight": (h,), p + "attention.LayerNorm.bias": (h,),
                       p + "intermediate.dense.weight": (f, h), p + "intermediate.dense.bias": (f,),
                       p + "output.dense.weight": (h, f), p + "output.dense.bias": (h,),
                       p + "output.LayerNorm.weight": (h,), p + "output.LayerNorm.bias": (h,)})
    disk = {prefix + k: (0.08 * rng.standard_normal(s)).astype(np.float32) for k, s in shapes.items()}
    save_file(disk, os.path.join(path, "model.safetensors"))
    return {k[len(prefix):]: v for k, v in disk.items()}, vocab


@pytest.mark.parametrize("prefix", ["mpnet.", ""])
def test_loader_reads_an_mpnet_directory(tmp_path, prefix):
    from rag.embedding import _load_local_dir
    raw, vocab = write_mpnet_dir(str(tmp_path), prefix=prefix)
    shape, w, tok, pre_lower, has_norm = _load_local_dir(str(tmp_path))
    assert (shape.vocab_size, shape.hidden, shape.layers, shape.heads, shape.ffn, shape.max_pos) == (len(vocab), 64, 2, 4, 128, 66)
    assert (shape.rel_buckets, shape.rel_max_distance, shape.pos_offset, shape.pooling, shape.max_seq) == (32, 128, 2, "mean", 48)
    assert abs(shape.ln_eps - 1e-5) < 1e-12
    for i in range(2):
        p = f"encoder.layer.{i}."
        # what HipEncoder stacks into w_qkv [3H, H] / b_qkv, and the other renamed tensors
        qkv = np.concatenate([w[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")])
        assert qkv.shape == (192, 64)
        assert np.array_equal(qkv, np.concatenate([raw[p + f"attention.attn.{n}.weight"] for n in "qkv"]))
        assert np.array_equal(np.concatenate([w[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")]),
                              np.concatenate([raw[p + f"attention.attn.{n}.bias"] for n in "qkv"]))
        assert np.array_equal(w[p + "attention.output.dense.weight"], raw[p + "attention.attn.o.weight"])
        assert np.array_equal(w[p + "attention.output.LayerNorm.bias"], raw[p + "attention.LayerNorm.bias"])
        assert np.array_equal(w[p + "output.LayerNorm.weight"], raw[p + "output.LayerNorm.weight"])
    assert np.array_equal(w["encoder.relative_attention_bias.weight"], raw["encoder.relative_attention_bias.weight"])
    assert w["embeddings.token_type_embeddings.weight"].shape == (1, 64) and not w["embeddings.token_type_embeddings.weight"].any()
    assert w["embeddings.position_embeddings.weight"].shape == (66, 64)


@pytest.mark.parametrize("tokenizer_json,backend", [(False, ""), (False, "python"), (True, "")])
def test_mpnet_directory_tokenizes_with_its_own_special_tokens(tmp_path, monkeypatch, tokenizer_json, backend):
    from rag.tokenizer import pad_batch, tokenizer_from_model_dir
    monkeypatch.setenv("CRS_TOKENIZER", backend)
    _, vocab = write_mpnet_dir(str(tmp_path), tokenizer_json=tokenizer_json)
    tok = tokenizer_from_model_dir(str(tmp_path))
    v = {t: i for i, t in enumerate(vocab)}
    assert (tok.cls_id, tok.sep_id, tok.pad_id) == (0, 2, 1)
    ids = tok.encode("The quick brown fox zzzz", 16)
    assert ids == [0, v["the"], v["quick"], v["brown"], v["fox"], v["[UNK]"], 2]
    assert tok.encode("the " * 40, 8) == [0] + [v["the"]] * 6 + [2]
    padded, lens = pad_batch([ids, ids[:3]], tok.pad_id)
    assert lens.tolist() == [7, 3] and padded[1].tolist() == ids[:3] + [1] * 4


def test_unknown_model_type_is_named(tmp_path):
    from rag.embedding import _load_local_dir
    write_mpnet_dir(str(tmp_path), model_type="roberta", prefix="roberta.")
    with pytest.raises(NotImplementedError, match="roberta"):
        _load_local_dir(str(tmp_path))


@pytest.mark.parametrize("tokenizer_json,backend", [(False, ""), (False, "python"), (True, "")])
def test_bert_directory_tokenizes_to_the_same_ids_as_before(tmp_path, monkeypatch, tokenizer_json, backend):
    from rag.embedding import _load_local_dir
    from rag.tokenizer import WordPieceTokenizer
    monkeypatch.setenv("CRS_TOKENIZER", backend)
    write_model_dir(str(tmp_path), tokenizer_json=tokenizer_json)
    shape, w, tok, _, _ = _load_local_dir(str(tmp_path))
    assert (shape.rel_buckets, shape.pos_offset) == (0, 0) and "encoder.relative_attention_bias.weight" not in w
    v = {t: i for i, t in enumerate(make_vocab())}
    spec = WordPieceTokenizer(v)                                   # [CLS] / [SEP] / [PAD] / [UNK]: the fixed names of before
    assert (tok.cls_id, tok.sep_id, tok.pad_id) == (v["[CLS]"], v["[SEP]"], v["[PAD]"]) == (2, 3, 0)
    for text in ("The quick brown fox jumps over the lazy dog.", "retrieval augmented generation embeds chunks", "zzzz qqq!", ""):
        assert tok.encode(text, 48) == spec.encode(text, 48)
    assert tok.encode("zzzz", 8) == [2, v["[UNK]"], 3]


def test_synthetic_mpnet_shapes():
    from rag._encoder import ModelShape
    from rag.embedding import _KNOWN, synthetic_weights
    big = _KNOWN["all-mpnet-base-v2"]
    assert [big[k] for k in ("vocab_size", "hidden", "layers", "heads", "ffn", "max_pos", "pooling", "max_seq", "ln_eps", "rel_buckets")] == \
        [30527, 768, 12, 12, 3072, 514, "mean", 384, 1e-5, 32]
    tiny = ModelShape(**{"ln_eps": 1e-12, **_KNOWN["tiny-mpnet"]})
    assert {k: v for k, v in _KNOWN["tiny-mpnet"].items() if k in _KNOWN["tiny"] and k != "max_pos"} == \
        {k: v for k, v in _KNOWN["tiny"].items() if k != "max_pos"}
    assert (tiny.max_pos, tiny.rel_buckets, tiny.pos_offset) == (66, 32, 2)
    w = synthetic_weights(tiny, 5)
    assert w["encoder.relative_attention_bias.weight"].shape == (32, 4) and w["encoder.relative_attention_bias.weight"].std() > 0.1
    assert not w["embeddings.token_type_embeddings.weight"].any()
    plain = synthetic_weights(ModelShape(ln_eps=1e-12, **_KNOWN["tiny"]), 5)
    assert "encoder.relative_attention_bias.weight" not in plain and plain["embeddings.token_type_embeddings.weight"].any()
