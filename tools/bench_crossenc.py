#!/usr/bin/env python3
"""Throughput of cross-encoder re-ranking (rag/reranking.py, crs_encoder_score_pairs) for synthetic:minilm-ce
(ms-marco-MiniLM-L-6-v2's shape, seeded weights): 64 queries x 20 candidates = 1280 pairs, every pair exactly 64, 128 or 256
tokens long, 128 pairs per launch.

  python tools/bench_crossenc.py --out profiles/crossenc_bench.json
      per sequence length: pairs/s of CrossEncoderReranker.predict (wall: tokenisation with a warm per-text cache, padding, ten
      launches, the readback) and of the device work alone (events around the ten score_pairs calls); median of --reps after a
      warm-up
  rocprofv3 --kernel-trace --stats -d DIR -o ce -- python tools/bench_crossenc.py --once
  python tools/bench_crossenc.py --stats DIR/.../ce_kernel_stats.csv --out profiles/crossenc_bench.json
      a run of its own for the profiler (one predict per length, no timing), then the share of device time spent in the two new
      kernels (embed_ln*_kernel<N, true>, pair_head_kernel) read from its kernel statistics and merged into the same file
Anything not measured is written as "unmeasured"."""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

QUERIES, CANDIDATES, SEQS = 64, 20, (64, 128, 256)
WORDS = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine similarity "
         "vector index chunk context answer question compression memory latency throughput accuracy benchmark kernel").split()


def make_pairs(rng, seq):
    """64 x 20 (query, text) pairs whose joined length is exactly `seq` tokens: 12-word queries, texts filling the rest
    (the hash tokeniser gives one token per word)."""
    queries = [" ".join(rng.choice(WORDS, size=12)) for _ in range(QUERIES)]
    return [(q, " ".join(rng.choice(WORDS, size=seq - 3 - 12))) for q in queries for _ in range(CANDIDATES)]


def run(args):
    import numpy as np
    import torch
    from rag.reranking import CrossEncoderReranker
    rng = np.random.default_rng(0)
    ce = CrossEncoderReranker({"model_name": "synthetic:minilm-ce", "batch_size": 128})
    rows = []
    for seq in SEQS:
        pairs = make_pairs(rng, seq)
        ids, _ = ce.tokenize_pairs(pairs)
        assert {len(i) for i in ids} == {seq}
        ce.predict(pairs)                                        # warm-up: weights up, workspace sized, token cache filled
        if args.once:
            continue
        wall, dev = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ce.predict(pairs)
            wall.append(time.perf_counter() - t0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ce.predict_device(pairs)
            e1.record()
            torch.cuda.synchronize()
            dev.append(e0.elapsed_time(e1) / 1e3)
        n = len(pairs)
        rows.append({"seq": seq, "pairs": n, "batch_size": ce.batch_size, "reps": args.reps,
                     "predict_pairs_per_s": round(n / statistics.median(wall), 1),
                     "predict_ms": {"median": round(1e3 * statistics.median(wall), 3), "min": round(1e3 * min(wall), 3), "max": round(1e3 * max(wall), 3)},
                     "device_span_pairs_per_s": round(n / statistics.median(dev), 1),
                     "device_span_ms": {"median": round(1e3 * statistics.median(dev), 3), "min": round(1e3 * min(dev), 3), "max": round(1e3 * max(dev), 3)}})
        print(json.dumps(rows[-1]))
    return rows


def kernel_share(path):
    """Share of the summed kernel time spent in the two new kernels, from rocprofv3's *_kernel_stats.csv."""
    total, new = 0.0, {"embed_ln_types": 0.0, "pair_head": 0.0}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            total += ns
            name = row.get("Name", "")
            if "pair_head_kernel" in name:
                new["pair_head"] += ns
            elif re.search(r"embed_ln2?_kernel(<\d+, true>|ILi\d+ELb1EE)", name):      # the TYPES instantiations (csrc/enc_misc.hip)
                new["embed_ln_types"] += ns
    if total <= 0:
        return "unmeasured"
    return {"kernel_time_ms": round(total / 1e6, 3), **{k + "_share": round(v / total, 5) for k, v in new.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", action="store_true", help="one predict per length and nothing else (the profiler's run)")
    ap.add_argument("--stats", help="rocprofv3 kernel statistics CSV of a --once run")
    ap.add_argument("--out")
    args = ap.parse_args()
    result = {"model": "synthetic:minilm-ce", "queries": QUERIES, "candidates": CANDIDATES, "throughput": "unmeasured",
              "new_kernels_share_of_device_time": "unmeasured"}
    if args.out and os.path.exists(args.out):
        with open(args.out) as fh:
            result.update(json.load(fh))
    if args.stats:
        result["new_kernels_share_of_device_time"] = kernel_share(args.stats)
    else:
        rows = run(args)
        if rows:
            result["throughput"] = rows
    if args.out and not args.once:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
