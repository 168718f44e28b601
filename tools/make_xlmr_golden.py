#!/usr/bin/env python3
"""Regenerates the XLM-RoBERTa fixtures under tests/golden/ with the locally installed tokenizers / sentencepiece / transformers:

* unigram_nfkc.json, unigram_spm.json.xz: tokenizer.json files over the vocabulary of tests/_unigram_cases.py with XLM-R's
  pipeline (WhitespaceSplit + Metaspace, Unigram, <s> $A </s> / <s> $A </s> </s> $B </s>); the normaliser is NFKC + Replace in the
  first and Precompiled + Replace in the second, the nmt_nfkc charsmap taken from the model proto of a throw-away
  sentencepiece model trained here;
* unigram_ids.json.xz: the edge corpus and the library's ids for both at every row width;
* encoder_xlmr.npz: XLMRobertaModel in fp64 on the CPU with the seeded weights of tests/_xlmr_cases.py (as
  tools/make_mpnet_golden.py does for MPNet);
* crossenc_xlmr.npz: XLMRobertaForSequenceClassification fp64 logits.

    python tools/make_xlmr_golden.py [tokenizer|encoder|crossenc ...]
"""
import io
import json
import lzma
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "compressed-rag-suite_amd"))
import _unigram_cases as uc  # noqa: E402
import _xlmr_cases as xc  # noqa: E402


def nmt_nfkc_charsmap() -> bytes:
    import sentencepiece as spm
    from sentencepiece import sentencepiece_model_pb2 as pb
    model = io.BytesIO()
    lines = ["hello world this is a test of the tokenizer"] * 50 + ["abc def ghi jkl mno pqr stu vwx yz"] * 20
    spm.SentencePieceTrainer.train(sentence_iterator=iter(lines), model_writer=model, vocab_size=30, model_type="unigram",
                                   normalization_rule_name="nmt_nfkc", hard_vocab_limit=False, minloglevel=2)
    proto = pb.ModelProto()
    proto.ParseFromString(model.getvalue())
    assert proto.normalizer_spec.name == "nmt_nfkc"
    return proto.normalizer_spec.precompiled_charsmap


def build_tokenizer(first_normalizer):
    from tokenizers import AddedToken, Regex, Tokenizer, normalizers, pre_tokenizers
    from tokenizers.models import Unigram
    from tokenizers.processors import TemplateProcessing
    tok = Tokenizer(Unigram(uc.vocab(), unk_id=uc.UNK_ID, byte_fallback=False))
    tok.normalizer = normalizers.Sequence([first_normalizer, normalizers.Replace(Regex(" {2,}"), uc.META)])
    tok.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.WhitespaceSplit(),
                                                 pre_tokenizers.Metaspace(replacement=uc.META, prepend_scheme="always")])
    tok.post_processor = TemplateProcessing(single="<s> $A </s>", pair="<s> $A </s> </s> $B </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    tok.add_special_tokens([AddedToken(t, normalized=False, special=True) for t in ("<s>", "<pad>", "</s>", "<unk>")])
    return tok


def tokenizer_fixtures():
    from tokenizers import normalizers
    from rag import _native as nat
    toks = {"nfkc": build_tokenizer(normalizers.NFKC()), "spm": build_tokenizer(normalizers.Precompiled(nmt_nfkc_charsmap()))}
    for name, path in (("nfkc", uc.NFKC_JSON), ("spm", uc.SPM_JSON)):
        with (lzma.open(path, "wt", encoding="utf-8", preset=9) if path.endswith(".xz") else open(path, "w", encoding="utf-8")) as fh:
            json.dump(json.loads(toks[name].to_str()), fh, ensure_ascii=False, separators=(",", ":"))
        print(f"wrote {path}: {os.path.getsize(path)} bytes")
    corpus = uc.edge_corpus(nat.UNIGRAM_MAX_WORD, nat.UNIGRAM_TILE_BYTES)
    out = {"cap": nat.UNIGRAM_MAX_WORD, "tile": nat.UNIGRAM_TILE_BYTES, "names": [n for n, _ in corpus], "texts": [t for _, t in corpus],
           "ids": {}}
    for name, tok in toks.items():
        for width in uc.WIDTHS:
            tok.enable_truncation(max_length=width)
            out["ids"][f"{name}.{width}"] = [e.ids for e in tok.encode_batch([t for _, t in corpus])]
    with lzma.open(uc.IDS_JSON, "wt", encoding="utf-8", preset=9) as fh:
        json.dump(out, fh, ensure_ascii=True, separators=(",", ":"))
    print(f"wrote {uc.IDS_JSON}: {os.path.getsize(uc.IDS_JSON)} bytes")


def hf_config(cfg, **extra):
    from transformers import XLMRobertaConfig
    return XLMRobertaConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                            num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos,
                            layer_norm_eps=cfg.ln_eps, type_vocab_size=1, hidden_act="gelu", hidden_dropout_prob=0.0,
                            attention_probs_dropout_prob=0.0, pad_token_id=xc.PAD_ID, bos_token_id=xc.CLS_ID, eos_token_id=xc.SEP_ID,
                            **extra)


def encoder_fixture():
    import torch
    from transformers import XLMRobertaModel
    out = {}
    with torch.no_grad():
        for key, cfg, seed, batch, seq in xc.CASES:
            model = XLMRobertaModel(hf_config(cfg), add_pooling_layer=False).double().eval()
            state = {k: torch.from_numpy(v).double() for k, v in xc.make_weights(cfg, seed).items()}
            missing, unexpected = model.load_state_dict(state, strict=False)
            assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
            ids, mask = xc.synth_tokens(cfg, batch, seq, seed + 1000)
            hid = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).last_hidden_state
            m = torch.from_numpy(mask).double()
            mean = (hid * m[..., None]).sum(1) / m.sum(1, keepdim=True)
            mean = mean / mean.norm(dim=1, keepdim=True)
            cls = hid[:, 0] / hid[:, 0].norm(dim=1, keepdim=True)
            rows = xc.hidden_rows(mask)
            out[key + ".seed"] = np.int64(seed)
            out[key + ".ids"], out[key + ".mask"] = ids, mask.astype(np.int8)
            out[key + ".rows"] = rows.astype(np.int32)
            out[key + ".hidden"] = hid.reshape(-1, cfg.hidden)[torch.from_numpy(rows)].numpy().astype(np.float32)
            out[key + ".mean_norm"] = mean.numpy().astype(np.float32)
            out[key + ".cls_norm"] = cls.numpy().astype(np.float32)
            print(f"{key}: {batch} x {seq}, lens {mask.sum(1).tolist()}, {rows.size} hidden rows")
    np.savez(xc.GOLDEN, **out)
    print(f"wrote {xc.GOLDEN}: {os.path.getsize(xc.GOLDEN)} bytes")


def crossenc_fixture():
    import torch
    from transformers import XLMRobertaForSequenceClassification
    out = {}
    with torch.no_grad():
        for key, cfg, seed, batch, seq in xc.CE_CASES:
            model = XLMRobertaForSequenceClassification(hf_config(cfg, num_labels=1)).double().eval()
            state = {k: torch.from_numpy(v).double() for k, v in xc.checkpoint_names(xc.make_ce_weights(cfg, seed)).items()}
            missing, unexpected = model.load_state_dict(state, strict=False)
            assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
            ids, mask = xc.synth_pairs(cfg, batch, seq, seed + 1000)
            logits = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).logits[:, 0]
            out[key + ".seed"] = np.int64(seed)
            out[key + ".ids"], out[key + ".mask"] = ids, mask.astype(np.int8)
            out[key + ".logits"] = logits.numpy().astype(np.float64)
            print(f"{key}: {batch} x {seq}, logits {logits.numpy().round(4).tolist()}")
    np.savez(xc.CE_GOLDEN, **out)
    print(f"wrote {xc.CE_GOLDEN}: {os.path.getsize(xc.CE_GOLDEN)} bytes")


if __name__ == "__main__":
    what = sys.argv[1:] or ["tokenizer", "encoder", "crossenc"]
    if "tokenizer" in what:
        tokenizer_fixtures()
    if "encoder" in what:
        encoder_fixture()
    if "crossenc" in what:
        crossenc_fixture()
