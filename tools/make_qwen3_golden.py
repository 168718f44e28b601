#!/usr/bin/env python3
"""Regenerates tests/golden/encoder_qwen3.npz with the locally installed transformers: Qwen3Model in fp64 with the seeded weights of
tests/_qwen3_ref.py, eager attention, every sequence on its own (unpadded, causal mask only).

Two tiny models (tests/_qwen3_ref.CFGS): "g2" head_dim 128 with 2 query heads on 1 key / value head, "g1" head_dim 64 with 2 on 2;
hidden 128, 2 layers.  Per model: the ids [5, 130] (lengths 1, 63, 64, 65, 130, right-padded with 0), the final hidden states of the
real rows, the normalised last-token embeddings, and -- instead of the ~1.5 MB of weights, which would not fit a committed file -- the
seed and a SHA-256 of the weights that tests/_qwen3_ref.make_weights regenerates (the tests compare the digest).  Hidden states are
stored as fp32 (a relative 6e-8, five orders below the forward's bounds) to halve the file.

    python tools/make_qwen3_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressed-rag-suite_amd"))     # rag.embedding.synthetic_weights makes the weights
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _qwen3_ref as qr  # noqa: E402


def all_fp64():
    """transformers' eager attention runs its softmax in fp32 whatever the model's dtype; replaced by the same statements without the
    cast (grouped heads repeated as the library does).  The rotation's angles stay as the library computes them, in fp32."""
    import transformers.models.qwen3.modeling_qwen3 as mq

    def eager_attention_forward(module, query, key, value, attention_mask, scaling, dropout=0.0, **kwargs):
        key, value = mq.repeat_kv(key, module.num_key_value_groups), mq.repeat_kv(value, module.num_key_value_groups)
        w = torch.matmul(query, key.transpose(2, 3)) * scaling
        if attention_mask is not None:
            w = w + attention_mask[:, :, :, : key.shape[-2]]
        w = torch.softmax(w, dim=-1)
        return torch.matmul(w, value).transpose(1, 2).contiguous(), w

    mq.eager_attention_forward = eager_attention_forward


def build_model(cfg, weights):
    from transformers import Qwen3Config, Qwen3Model
    d = qr.hf_config(cfg)
    theta = d.pop("rope_theta")
    for k in ("architectures", "model_type"):
        d.pop(k)
    hf = Qwen3Config(**d, rope_parameters={"rope_type": "default", "rope_theta": theta})
    hf._attn_implementation = "eager"
    model = Qwen3Model(hf).double().eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v).double() for k, v in weights.items()}, strict=False)
    assert not unexpected and all("inv_freq" in m for m in missing), (missing, unexpected)
    return model


@torch.no_grad()
def main():
    all_fp64()
    out = {}
    for key, cfg in qr.CFGS.items():
        w = qr.make_weights(cfg)
        model = build_model(cfg, w)
        ids = qr.synth_ids(cfg)
        rows, last = [], []
        for b, n in enumerate(qr.LENS):
            hid = model(input_ids=torch.from_numpy(ids[b:b + 1, :n]).long()).last_hidden_state[0].numpy()
            rows.append(hid)
            last.append(hid[n - 1] / np.linalg.norm(hid[n - 1]))
        out[key + ".seed"] = np.int64(cfg["seed"])
        out[key + ".weights_sha256"] = np.array(qr.weights_digest(w))
        out[key + ".ids"] = ids
        out[key + ".hidden"] = np.concatenate(rows).astype(np.float32)       # the real rows, in row-major order
        out[key + ".last_norm"] = np.stack(last).astype(np.float64)
        print(key, "rows", sum(qr.LENS), "max |hidden|", float(np.abs(out[key + ".hidden"]).max()))
    import transformers
    out["meta.transformers_version"] = np.array(transformers.__version__)
    out["meta.patched"] = np.array("eager_attention_forward: fp32 softmax cast removed; one sequence per call, unpadded")
    np.savez(qr.GOLDEN, **out)
    print(f"wrote {qr.GOLDEN}: {os.path.getsize(qr.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
