#!/usr/bin/env python3
"""Throughput of BERTScore on the device (rag/bertscore.py, crs_token_match) for a MiniLM-class shape (H 384, 6 layers) and a
base-class one (H 768, layer 9 of 12: bert-base-uncased's published layer), seeded weights, 64 pairs per launch, both sides
exactly 32, 128 or 512 tokens long.

  python tools/bench_bertscore.py --out profiles/bertscore_bench.json

Per shape and length, hipEvent spans after a warm-up, median of --reps spans of --iters back-to-back calls each, clocks as
found: the whole scoring step from token ids (two encoder forwards + the matching launch; pairs/s), the matching kernel alone
on the forwards' hidden states, its share of the whole, and the same matching step written with torch ops on the same device
(normalize, bmm, masked max, weighted mean -- the bert_score package's form).  A report, not a pass condition."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

PAIRS, SEQS = 64, (32, 128, 512)
SHAPES = {"minilm-class": ("all-minilm-l6-v2", 6), "base-class": ("bge-base-en-v1.5", 9)}


def span_ms(fn, iters, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}


def torch_match(ha, hb, mask_a, mask_b, wa, wb):
    import torch
    an, bn = torch.nn.functional.normalize(ha, dim=-1), torch.nn.functional.normalize(hb, dim=-1)
    sim = torch.bmm(an, bn.transpose(1, 2))
    sim = sim.masked_fill(~(mask_a[:, :, None] & mask_b[:, None, :]), float("-inf"))
    P = (sim.max(2).values.masked_fill(~mask_a, 0) * wa).sum(1) / wa.sum(1)
    R = (sim.max(1).values.masked_fill(~mask_b, 0) * wb).sum(1) / wb.sum(1)
    return torch.stack([P, R, 2 * P * R / (P + R)], 1)


def run(args):
    import numpy as np
    import torch
    from rag import _native as nat
    from rag._encoder import ModelShape
    from rag.bertscore import BertScorer
    from rag.embedding import _KNOWN, synthetic_weights
    rng = np.random.default_rng(0)
    rows = []
    for label, (arch, layers) in SHAPES.items():
        shape = ModelShape(**{"ln_eps": 1e-12, **_KNOWN[arch]})
        scorer = BertScorer({"model_name": arch, "num_layers": layers}, shape=shape, weights=synthetic_weights(shape, 0), tokenizer=None)
        for seq in SEQS:
            ids_a = rng.integers(1000, shape.vocab_size, (PAIRS, seq)).astype(np.int32)
            ids_b = rng.integers(1000, shape.vocab_size, (PAIRS, seq)).astype(np.int32)
            lens = np.full(PAIRS, seq, dtype=np.int32)
            whole = lambda: scorer.score_ids_device(ids_a, lens, ids_b, lens)
            got = whole()
            _, ha = scorer.model.forward(ids_a, lens, normalize=False, return_hidden=True)
            _, hb = scorer.model.forward(ids_b, lens, normalize=False, return_hidden=True)
            dl = torch.from_numpy(lens).to(scorer.device)
            w = torch.ones((PAIRS, seq), dtype=torch.float32, device=scorer.device)
            w[:, 0] = 0
            w[:, -1] = 0
            out = torch.empty((PAIRS, 3), dtype=torch.float32, device=scorer.device)
            mask = torch.ones((PAIRS, seq), dtype=torch.bool, device=scorer.device)
            kernel = lambda: nat.token_match(ha, dl, hb, dl, w, w, out=out)
            ref = lambda: torch_match(ha, hb, mask, mask, w, w)
            diff = float((kernel() - ref()).abs().max())
            assert float((kernel() - got).abs().max()) == 0.0
            for fn in (whole, kernel, ref):
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t_whole, t_kernel, t_ref = (span_ms(fn, args.iters, args.reps) for fn in (whole, kernel, ref))
            rows.append({"shape": label, "hidden": shape.hidden, "layers": layers, "seq": seq, "pairs": PAIRS,
                         "pairs_per_s": round(PAIRS / (t_whole["median"] / 1e3), 1), "score_ms": t_whole,
                         "token_match_ms": t_kernel, "token_match_share": round(t_kernel["median"] / t_whole["median"], 4),
                         "torch_ops_match_ms": t_ref, "torch_over_kernel": round(t_ref["median"] / t_kernel["median"], 3),
                         "max_abs_diff_vs_torch": diff})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    import torch
    result = {"device": torch.cuda.get_device_name(0), "clocks": "as found", "reps": args.reps, "iters_per_span": args.iters,
              "rows": run(args)}
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
