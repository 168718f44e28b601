#!/usr/bin/env python3
"""Regenerates tests/golden/encoder_nomic.npz with the locally installed transformers: NomicBertModel with the seeded weights
of tests/_nomic_cases.py, in fp64 on the CPU.  Per case: seed, ids, mask, the final hidden states of a sample of real
tokens (`rows`: flat indices into [B * S]; all tokens of a small case), mean- and CLS-pooled normalised outputs.

    python tools/make_nomic_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _nomic_cases as nc  # noqa: E402


def build_model(cfg, weights):
    from transformers import NomicBertConfig, NomicBertModel
    hf = NomicBertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                         num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos,
                         layer_norm_eps=cfg.ln_eps, hidden_act="silu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                         pad_token_id=nc.PAD_ID, rope_parameters={"rope_type": "default", "rope_theta": nc.THETA})
    hf._attn_implementation = "eager"
    model = NomicBertModel(hf).double().eval()
    state = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    # what is not a weight of the checkpoint: buffers (rotary inv_freq, position ids) and an optional pooler
    assert not unexpected and all(("inv_freq" in m or "position_ids" in m or m.startswith("pooler.")) for m in missing), (missing, unexpected)
    return model


@torch.no_grad()
def main():
    out = {}
    for key, cfg, seed, batch, seq in nc.CASES:
        model = build_model(cfg, nc.make_weights(cfg, seed))
        ids, mask = nc.synth_tokens(cfg, batch, seq, seed + 1000)
        hid = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).last_hidden_state
        m = torch.from_numpy(mask).double()
        mean = (hid * m[..., None]).sum(1) / m.sum(1, keepdim=True)
        mean = mean / mean.norm(dim=1, keepdim=True)
        cls = hid[:, 0] / hid[:, 0].norm(dim=1, keepdim=True)
        rows = nc.hidden_rows(mask)
        out[key + ".seed"] = np.int64(seed)
        out[key + ".ids"], out[key + ".mask"] = ids, mask.astype(np.int8)
        out[key + ".rows"] = rows.astype(np.int32)
        out[key + ".hidden"] = hid.reshape(-1, cfg.hidden)[torch.from_numpy(rows)].numpy().astype(np.float64)
        out[key + ".mean_norm"] = mean.numpy().astype(np.float32)
        out[key + ".cls_norm"] = cls.numpy().astype(np.float32)
        print(f"{key}: {batch} x {seq}, lens {mask.sum(1).tolist()}, {rows.size} hidden rows")
    np.savez(nc.GOLDEN, **out)
    print(f"wrote {nc.GOLDEN}: {os.path.getsize(nc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
