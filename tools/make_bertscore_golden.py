#!/usr/bin/env python3
"""Regenerates tests/golden/bertscore.npz with the locally installed transformers: BertModel / RobertaModel with the seeded
weights of tests/_bertscore_cases.py, in fp64 on the CPU, output_hidden_states=True.  Per case: ids and masks of both sides,
P / R / F in fp64 from the plain restatement of the matching step (_bertscore_cases.match_ref, the package's weights: 1 on
real tokens, 0 on the two specials) on the hidden states of layer L = the case's layer count (`prf`) and of layer L - 1
(`prf_prev`), and the smallest token-state norm at layer L (`min_norm`, the denominator of the provable tolerance ceiling).

    python tools/make_bertscore_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _bertscore_cases as bc  # noqa: E402


def build_model(cfg, weights):
    common = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads,
                  intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos, layer_norm_eps=cfg.ln_eps,
                  type_vocab_size=cfg.type_rows, hidden_act="gelu", hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                  pad_token_id=cfg.pad_id)
    if cfg.kind == "roberta":
        from transformers import RobertaConfig, RobertaModel
        model = RobertaModel(RobertaConfig(bos_token_id=cfg.cls_id, eos_token_id=cfg.sep_id, **common), add_pooling_layer=False)
    else:
        from transformers import BertConfig, BertModel
        model = BertModel(BertConfig(**common), add_pooling_layer=False)
    model = model.double().eval()
    state = {k: torch.from_numpy(v).double() for k, v in weights.items()}
    missing, unexpected = model.load_state_dict(state, strict=False)
    assert not unexpected and all("position_ids" in m or "token_type_ids" in m for m in missing), (missing, unexpected)
    return model


@torch.no_grad()
def main():
    out = {}
    for key, cfg, seed, pairs, seq_a, seq_b in bc.CASES:
        model = build_model(cfg, bc.make_weights(cfg, seed))
        ids_a, mask_a, ids_b, mask_b = bc.synth_pairs(cfg, pairs, seq_a, seq_b, seed + 1000)

        def states(ids, mask):
            r = model(input_ids=torch.from_numpy(ids).long(), attention_mask=torch.from_numpy(mask).long(), output_hidden_states=True)
            return [h.numpy() for h in r.hidden_states]

        ha, hb = states(ids_a, mask_a), states(ids_b, mask_b)
        la, lb = mask_a.sum(1), mask_b.sum(1)
        wa, wb = bc.token_weights(mask_a), bc.token_weights(mask_b)
        L = cfg.layers
        out[key + ".ids_a"], out[key + ".mask_a"] = ids_a, mask_a.astype(np.int8)
        out[key + ".ids_b"], out[key + ".mask_b"] = ids_b, mask_b.astype(np.int8)
        out[key + ".prf"] = bc.match_ref(ha[L], la, hb[L], lb, wa, wb)
        out[key + ".prf_prev"] = bc.match_ref(ha[L - 1], la, hb[L - 1], lb, wa, wb)
        norms = [np.linalg.norm(h[p, :n], axis=1).min() for h, ls in ((ha[L], la), (hb[L], lb)) for p, n in enumerate(ls)]
        out[key + ".min_norm"] = np.float64(min(norms))
        print(f"{key}: {pairs} x ({seq_a} vs {seq_b}), lens {la.tolist()} / {lb.tolist()}, min|h| {min(norms):.3f}, "
              f"ceiling {bc.e2e_ceiling(cfg.hidden, min(norms)):.4f}\n  L   {np.round(out[key + '.prf'], 4).tolist()}\n"
              f"  L-1 {np.round(out[key + '.prf_prev'], 4).tolist()}")
    np.savez_compressed(bc.GOLDEN, **out)
    print(f"wrote {bc.GOLDEN}: {os.path.getsize(bc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
