#!/usr/bin/env python3
"""Regenerates tests/golden/encoder_mpnet.npz with the locally installed transformers: MPNetModel with the seeded weights
of tests/_mpnet_cases.py, in fp64 on the CPU.  Per case: seed, ids, mask, the final hidden states of a sample of real
tokens (`rows`: flat indices into [B * S]; all tokens of a small case), mean- and CLS-pooled normalised outputs; plus the
bucket index of the offsets key - query = -511 .. 511 from MPNetEncoder.relative_position_bucket.

    python tools/make_mpnet_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _mpnet_cases as mc  # noqa: E402

# internal (BertModel) names -> MPNetModel's, inside "encoder.layer.<i>."
TO_MPNET = {"attention.self.query.": "attention.attn.q.", "attention.self.key.": "attention.attn.k.",
            "attention.self.value.": "attention.attn.v.", "attention.output.dense.": "attention.attn.o.",
            "attention.output.LayerNorm.": "attention.LayerNorm."}


def build_model(cfg, weights):
    from transformers import MPNetConfig, MPNetModel
    hf = MPNetConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers,
                     num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos,
                     layer_norm_eps=cfg.ln_eps, relative_attention_num_buckets=mc.BUCKETS, hidden_act="gelu",
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, pad_token_id=mc.PAD_ID)
    model = MPNetModel(hf, add_pooling_layer=False).double().eval()
    state = {}
    for k, v in weights.items():
        if k == "embeddings.token_type_embeddings.weight":
            continue
        if k.startswith("encoder.layer."):
            parts = k.split(".", 3)
            for old, new in TO_MPNET.items():
                if parts[3].startswith(old):
                    parts[3] = new + parts[3][len(old):]
                    break
            k = ".".join(parts)
        state[k] = torch.from_numpy(v).double()
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all("position_ids" in m for m in missing), (missing, unexpected)
    return model


@torch.no_grad()
def main():
    from transformers.models.mpnet.modeling_mpnet import MPNetEncoder
    out = {"bucket_offsets": np.arange(-511, 512, dtype=np.int32)}
    out["bucket_index"] = MPNetEncoder.relative_position_bucket(torch.arange(-511, 512), num_buckets=mc.BUCKETS,
                                                                 max_distance=128).numpy().astype(np.int32)
    for key, cfg, seed, batch, seq in mc.CASES:
        model = build_model(cfg, mc.make_weights(cfg, seed))
        ids, mask = mc.synth_tokens(cfg, batch, seq, seed + 1000)
        hid = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long()).last_hidden_state
        m = torch.from_numpy(mask).double()
        mean = (hid * m[..., None]).sum(1) / m.sum(1, keepdim=True)
        mean = mean / mean.norm(dim=1, keepdim=True)
        cls = hid[:, 0] / hid[:, 0].norm(dim=1, keepdim=True)
        rows = mc.hidden_rows(mask)
        out[key + ".seed"] = np.int64(seed)
        out[key + ".ids"], out[key + ".mask"] = ids, mask.astype(np.int8)
        out[key + ".rows"] = rows.astype(np.int32)
        out[key + ".hidden"] = hid.reshape(-1, cfg.hidden)[torch.from_numpy(rows)].numpy().astype(np.float32)
        out[key + ".mean_norm"] = mean.numpy().astype(np.float32)
        out[key + ".cls_norm"] = cls.numpy().astype(np.float32)
        print(f"{key}: {batch} x {seq}, lens {mask.sum(1).tolist()}, {rows.size} hidden rows")
    np.savez(mc.GOLDEN, **out)
    print(f"wrote {mc.GOLDEN}: {os.path.getsize(mc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
