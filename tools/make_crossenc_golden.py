#!/usr/bin/env python3
"""Regenerates tests/golden/crossenc.npz with the locally installed transformers: BertForSequenceClassification (one label) with
the seeded weights of tests/_crossenc_cases.py, in fp64 on the CPU.  Per case: seed, ids, type ids, mask, the logits and the
pooler outputs (fp64), and the final hidden states of a sample of real tokens (`rows`: flat indices into [B * S]; token 0 of
every pair among them).  Inputs and outputs only.

Before it writes it asserts, per case, that the fp64 logits with the type ids zeroed differ from the true ones by more than
ten times the parity test's logit tolerance (largest change over the rows): a kernel that ignores type ids cannot pass.

    python tools/make_crossenc_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _crossenc_cases as cc  # noqa: E402


def build_model(cfg, weights):
    from transformers import BertConfig, BertForSequenceClassification
    hf = BertConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                    intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos, type_vocab_size=2, layer_norm_eps=cfg.ln_eps,
                    hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, classifier_dropout=0.0,
                    num_labels=1, pad_token_id=cc.PAD_ID)
    hf._attn_implementation = "eager"
    model = BertForSequenceClassification(hf).double().eval()
    state = {(k if k.startswith("classifier.") else "bert." + k): torch.from_numpy(v).double() for k, v in weights.items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    return model


@torch.no_grad()
def main():
    out = {}
    for key, cfg, seed, batch, seq in cc.CASES:
        model = build_model(cfg, cc.make_weights(cfg, seed))
        ids, types, mask = cc.synth_pairs(cfg, batch, seq, seed + 1000)
        t = lambda a: torch.from_numpy(a).long()
        res = model(input_ids=t(ids), token_type_ids=t(types), attention_mask=t(mask), output_hidden_states=True)
        logits = res.logits.reshape(-1).numpy()
        hid = res.hidden_states[-1]
        pooled = model.bert.pooler(hid).numpy()
        zeroed = model(input_ids=t(ids), token_type_ids=t(np.zeros_like(types)), attention_mask=t(mask)).logits.reshape(-1).numpy()
        gap = np.abs(zeroed - logits)
        paired = types.any(1)
        assert paired.any() and gap.max() > cc.ZEROED_TYPES_GAP, \
            f"{key}: zeroing the type ids moves the logits by {gap.tolist()}, need > {cc.ZEROED_TYPES_GAP}: widen CLS_SCALE"
        assert (gap[~paired] == 0).all()
        rows = cc.hidden_rows(mask)
        assert all(b * seq in rows for b in range(batch))
        out[key + ".seed"] = np.int64(seed)
        out[key + ".ids"], out[key + ".type_ids"], out[key + ".mask"] = ids, types.astype(np.int8), mask.astype(np.int8)
        out[key + ".rows"] = rows.astype(np.int32)
        out[key + ".hidden"] = hid.reshape(-1, cfg.hidden)[torch.from_numpy(rows)].numpy().astype(np.float32)
        out[key + ".pooled"] = pooled.astype(np.float64)
        out[key + ".logits"] = logits.astype(np.float64)
        print(f"{key}: {batch} x {seq}, lens {mask.sum(1).tolist()}, first type-1 token {[int(r.argmax()) if r.any() else -1 for r in types]}, "
              f"logits {np.round(logits, 4).tolist()}, zeroed-types gap {np.round(gap, 4).tolist()}, {rows.size} hidden rows")
    np.savez(cc.GOLDEN, **out)
    print(f"wrote {cc.GOLDEN}: {os.path.getsize(cc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
