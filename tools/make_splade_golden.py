#!/usr/bin/env python3
"""Writes tests/golden/splade.npz: a tiny seeded transformers.BertForMaskedLM (random init, then the decoder bias shifted down by
1.5 standard deviations of a logit so that a text activates a few ids of this 88-word vocabulary, as a trained SPLADE model does and a random one does
not), a padded batch of token ids, and what `transformers` computes from them in fp32 on the CPU:

  w::<name>     every tensor of the state dict under its checkpoint name (cls.predictions.decoder.weight is tied to
                bert.embeddings.word_embeddings.weight and left out, as safetensors leaves it out; the bias is saved once, as
                cls.predictions.bias)
  config        the BertConfig as JSON
  ids, lens     int32 [batch, seq] right-padded with [PAD], int32 [batch]
  hidden        fp32 [batch, seq, H]   bert(...).last_hidden_state
  transform     fp32 [batch, seq, H]   cls.predictions.transform(hidden)
  weights       fp32 [batch, V]        max over the real tokens of log1p(relu(logits)): the SPLADE vector

Run from the repository root with transformers installed (written with 5.15):  python tools/make_splade_golden.py
tests/test_sparse_cpu.py holds tests/_sparse_ref.py and the loader of rag/sparse.py against this file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED, BATCH, SEQ, SHIFT_SIGMAS = 7, 6, 24, 1.5


def main(out_path):
    import torch
    import transformers
    from _modeldir import make_vocab
    vocab = make_vocab()
    cfg = transformers.BertConfig(vocab_size=len(vocab), hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128,
                                  max_position_embeddings=64, type_vocab_size=2, layer_norm_eps=1e-12, hidden_act="gelu",
                                  initializer_range=0.08, tie_word_embeddings=True)
    torch.manual_seed(SEED)
    model = transformers.BertForMaskedLM(cfg).eval()
    rng = np.random.default_rng(SEED)
    with torch.no_grad():
        sigma = np.sqrt(cfg.hidden_size) * cfg.initializer_range          # of a logit: the transform's output has unit variance
        bias = torch.from_numpy((0.02 * rng.standard_normal(len(vocab)) - SHIFT_SIGMAS * sigma).astype(np.float32))
        model.cls.predictions.bias.copy_(bias)
        for name, p in model.named_parameters():                            # LayerNorms and biases off their trivial init
            if name.endswith("LayerNorm.weight"):
                p.copy_(1.0 + 0.05 * torch.randn_like(p))
            elif name.endswith(".bias") and "predictions.bias" not in name and "decoder" not in name:
                p.copy_(0.02 * torch.randn_like(p))
    lens = np.array([SEQ, 1, 5, 17, 2, 11], dtype=np.int32)
    ids = np.zeros((BATCH, SEQ), dtype=np.int32)                           # [PAD] = 0
    for b in range(BATCH):
        body = rng.integers(5, len(vocab), size=max(int(lens[b]) - 2, 0))
        row = ([2] + body.tolist() + [3])[: int(lens[b])] if lens[b] > 1 else [2]     # [CLS] ... [SEP]
        ids[b, : len(row)] = row
    mask = (np.arange(SEQ)[None, :] < lens[:, None]).astype(np.int64)
    with torch.no_grad():
        hidden = model.bert(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask)).last_hidden_state
        transform = model.cls.predictions.transform(hidden)
        logits = model.cls.predictions.decoder(transform)
        w = torch.log1p(torch.relu(logits)) * torch.from_numpy(mask)[..., None]
        weights = w.max(dim=1).values
    state = {k: v.detach().numpy().astype(np.float32) for k, v in model.state_dict().items()}
    assert np.array_equal(state["cls.predictions.decoder.weight"], state["bert.embeddings.word_embeddings.weight"])
    assert np.array_equal(state["cls.predictions.decoder.bias"], state["cls.predictions.bias"])
    del state["cls.predictions.decoder.weight"], state["cls.predictions.decoder.bias"]
    state = {k: v for k, v in state.items() if not k.endswith("position_ids")}
    out = {"w::" + k: v for k, v in state.items()}
    out.update(config=np.frombuffer(json.dumps(cfg.to_dict(), sort_keys=True).encode(), dtype=np.uint8), ids=ids, lens=lens,
               hidden=hidden.numpy().astype(np.float32), transform=transform.numpy().astype(np.float32),
               weights=weights.numpy().astype(np.float32))
    np.savez_compressed(out_path, **out)
    nz = (weights.numpy() > 0).sum(1)
    print(f"{out_path}: {os.path.getsize(out_path)} bytes; V = {len(vocab)}; positive ids per text: {nz.tolist()}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "splade.npz"))
