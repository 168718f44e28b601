#!/usr/bin/env python3
"""Regenerates the ModernBERT fixtures under tests/golden/ with the locally installed transformers and tokenizers:

  modernbert_tokenizer.json         a small byte-level BPE tokenizer ([PAD] [CLS] [SEP], 256 byte symbols, a few merges; [CLS] $A [SEP]
                                    post-processor), trained on the inline corpus below
  modernbert_tokenizer_cases.json   a dozen texts and the ids the library gives them
  encoder_modernbert.npz            ModernBertModel with the seeded weights of tests/_modernbert_cases.py, fp64, eager attention, every sequence on its own
                                    (unpadded).  Per case: seed, ids, mask, last_hidden_state of the real rows (fp64), mean- and CLS-pooled normalised
                                    outputs; the case "a_text" runs the tokenised fixture texts through config (a)

    python tools/make_modernbert_golden.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _modernbert_cases as mc  # noqa: E402

CORPUS = [
    "the quick brown fox jumps over the lazy dog", "retrieval augmented generation grounds an answer in retrieved passages",
    "a sliding window lets every token attend to its neighbours only", "every third layer attends to the whole sequence",
    "rotary position embeddings rotate queries and keys", "the encoder maps a passage to one vector",
    "cosine similarity ranks the passages for a query", "long documents are split into overlapping chunks",
    "the feed-forward block multiplies a gate with an activated input", "layer normalisation comes before every block",
] * 4
TEXTS = [
    "the quick brown fox", "Retrieval-augmented generation", "a", "", "sliding window attention over 8192 tokens",
    "naïve café — déjà vu", "日本語のテキスト", "tabs\tand\nnewlines", "UPPER lower MiXeD", "  leading and trailing spaces  ",
    "numbers 0123456789 and punctuation !?.,;:", "the encoder maps a passage to one vector " * 6,
]
TEXT_MAX_SEQ = 48      # the long text above is cut to it
TEXT_SEED = 305


def train_tokenizer():
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    tok = Tokenizer(models.BPE())
    tok.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = decoders.ByteLevel()
    trainer = trainers.BpeTrainer(vocab_size=mc.CFG_A.vocab_size, special_tokens=["[PAD]", "[CLS]", "[SEP]"],
                                  initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tok.train_from_iterator(CORPUS, trainer)
    assert [tok.token_to_id(t) for t in ("[PAD]", "[CLS]", "[SEP]")] == [mc.PAD_ID, mc.CLS_ID, mc.SEP_ID]
    assert tok.get_vocab_size() <= mc.CFG_A.vocab_size
    tok.post_processor = processors.TemplateProcessing(single="[CLS] $A [SEP]", special_tokens=[("[CLS]", mc.CLS_ID), ("[SEP]", mc.SEP_ID)])
    tok.save(mc.TOKENIZER_JSON)
    return tok


def all_fp64():
    """transformers runs two steps of a double-precision ModernBertModel in fp32 whatever the model's dtype -- the softmax of eager
    attention and the rotation of queries and keys (q.float() * cos ...) -- which leaves its "fp64" output 1e-7 to 4e-6 from the exact
    value.  Both are replaced by the same statements without the casts.  (The angles stay as the library computes them, in fp32:
    tests/_modernbert_cases.py: rope_cos_sin_fp32.)"""
    import transformers.models.modernbert.modeling_modernbert as mm

    def eager_attention_forward(module, query, key, value, attention_mask, scaling, dropout=0.0, **kwargs):
        w = torch.matmul(query, key.transpose(2, 3)) * scaling
        if attention_mask is not None:
            w = w + attention_mask
        w = torch.softmax(w, dim=-1)
        return torch.matmul(w, value).transpose(1, 2).contiguous(), w

    def apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=1):
        cos, sin = cos.unsqueeze(unsqueeze_dim), sin.unsqueeze(unsqueeze_dim)
        return q * cos + mm.rotate_half(q) * sin, k * cos + mm.rotate_half(k) * sin

    mm.eager_attention_forward, mm.apply_rotary_pos_emb = eager_attention_forward, apply_rotary_pos_emb


def build_model(cfg, weights):
    from transformers import ModernBertConfig, ModernBertModel
    d = mc.hf_config_dict(cfg)
    for k in ("architectures", "model_type"):
        d.pop(k)
    hf = ModernBertConfig(**d)
    hf._attn_implementation = "eager"
    model = ModernBertModel(hf).double().eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v).double() for k, v in weights.items()}, strict=False)
    assert not unexpected and all("inv_freq" in m for m in missing), (missing, unexpected)
    return model


@torch.no_grad()
def run_case(out, key, cfg, seed, ids, mask):
    model = build_model(cfg, mc.make_weights(cfg, seed))
    # one sequence at a time at its own length: a PADDED batch gives NaN here -- a padding query further than the window from
    # the last real token has no allowed key in a sliding layer, eager attention's softmax over an all-masked row is NaN, and the
    # next layer multiplies that row's value vector by a weight of 0 (0 x NaN).  Real rows do not depend on the padding.
    hid = np.zeros(ids.shape + (cfg.hidden,))
    for b, n in enumerate(mask.sum(1)):
        hid[b, :n] = model(input_ids=torch.from_numpy(ids[b:b + 1, :n]).long()).last_hidden_state[0].numpy()
    mean, cls = mc.pooled(hid, mask)
    out[key + ".seed"] = np.int64(seed)
    out[key + ".ids"], out[key + ".mask"] = ids, mask.astype(np.int8)
    out[key + ".hidden"] = hid[mask.astype(bool)].astype(np.float64)          # the real rows, in row-major order
    out[key + ".mean_norm"], out[key + ".cls_norm"] = mean.astype(np.float64), cls.astype(np.float64)
    print(f"{key}: {ids.shape[0]} x {ids.shape[1]}, lens {mask.sum(1).tolist()}")


def main():
    all_fp64()
    tok = train_tokenizer()
    tok.enable_truncation(max_length=TEXT_MAX_SEQ)
    rows = [tok.encode(t.strip()).ids for t in TEXTS]
    json.dump({"max_seq": TEXT_MAX_SEQ, "texts": TEXTS, "ids": rows}, open(mc.TOKENIZER_CASES, "w"), ensure_ascii=False, indent=0)
    out = {}
    for key, cfg, seed, lens, seq in mc.CASES:
        ids, mask = mc.synth_tokens(cfg, lens, seq, seed + 1000)
        run_case(out, key, cfg, seed, ids, mask)
    ids = np.full((len(rows), TEXT_MAX_SEQ), mc.PAD_ID, dtype=np.int32)
    mask = np.zeros_like(ids)
    for i, r in enumerate(rows):
        ids[i, :len(r)], mask[i, :len(r)] = r, 1
    run_case(out, "a_text", mc.CFG_A, TEXT_SEED, ids, mask)
    # what made the file, for a later regeneration to be compared with: the library's version, and that two of its functions ran
    # as this tool's cast-free copies (all_fp64) on unpadded sequences
    import transformers
    out["meta.transformers_version"] = np.array(transformers.__version__)
    out["meta.patched"] = np.array("eager_attention_forward, apply_rotary_pos_emb: fp32 casts removed; one sequence per call, unpadded")
    np.savez(mc.GOLDEN, **out)
    print(f"wrote {mc.GOLDEN}: {os.path.getsize(mc.GOLDEN)} bytes; tokenizer {os.path.getsize(mc.TOKENIZER_JSON)} bytes")


if __name__ == "__main__":
    main()
