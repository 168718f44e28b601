#!/usr/bin/env python3
"""Timing of the ModernBERT encoder family, synthetic weights, tools/bench_nomic.py's conventions: same process,
alternating forms, --rounds rounds of --reps launches each, device events around each form, median [min - max].

(a) forward: synthetic:modernbert-base (768 / 12 heads / ffn 1152 / 22 layers / window 64) against synthetic:bge (768 / 12 / 3072 / 12)
             on the same token blocks, every row at full length: 256 x 128, 64 x 512, and 8 x 8192 -- where bge-base, whose position
             table ends at 512, runs the same 65536 tokens as 128 x 512.  Reported, no pass / fail.
(b) window:  attention_window_kernel (W = 64) against the blocked kernel (crs_attention_f16, route 3) on the SAME QKV buffer of
             65536 tokens, 12 heads of 64, at seq 512, 2048 and 8192, beside the block-count prediction 3 / (seq / 64).
(c) rows:    crs_add_layernorm_f32 and crs_rope_qk_f16 alone on buffers of each shape, times their launches per forward (2 and 1 per
             layer), as shares of (a)'s forward: isolated launches over the forward's median, so launch gaps inside the forward
             are not in the numerator.
A JSON array, one record per line, to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

SHAPES = ((256, 128, 256, 128), (64, 512, 64, 512), (8, 8192, 128, 512))      # modernbert batch, seq; bge batch, seq
WINDOW_SHAPES = ((128, 512), (32, 2048), (8, 8192))


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": len(ts)}


def timed(fn, reps, warm=2):
    import torch
    out = []
    for rep in range(reps + warm):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        if rep >= warm:
            out.append(e0.elapsed_time(e1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two forms (at least three)")
    ap.add_argument("--reps", type=int, default=5, help="timed launches per form and round (after 2 warm-up launches)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modernbert_bench.json"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import logging
    import numpy as np
    import torch
    logging.disable(logging.WARNING)
    from rag._encoder import add_layernorm_f32, attention_f16, attention_window_f16, rope_qk_f16
    from rag.embedding import EmbeddingModel
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as out:                    # rewritten after every record: a run cut short keeps what it measured
            out.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")

    dev = torch.device("cuda:0")
    mb = EmbeddingModel({"model_name": "synthetic:modernbert-base", "device": "cuda", "batch_size": 256, "normalize": True}).model
    bge = EmbeddingModel({"model_name": "synthetic:bge", "device": "cuda", "batch_size": 256, "normalize": True}).model
    h, layers, heads, window = mb.shape.hidden, mb.shape.layers, mb.shape.heads, mb.shape.window
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev); g.manual_seed(6)
    for batch, seq, bbatch, bseq in SHAPES:
        t = batch * seq
        ids = torch.from_numpy(rng.integers(1000, 30000, size=(batch, seq)).astype(np.int32)).to(dev)
        lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
        bids, blens = ids.view(bbatch, bseq), torch.full((bbatch,), bseq, dtype=torch.int32, device=dev)
        t_m, t_b = [], []
        for _ in range(args.rounds):
            t_m += timed(lambda: mb.forward(ids, lens), args.reps)
            t_b += timed(lambda: bge.forward(bids, blens), args.reps)
        mm, mbg = statistics.median(t_m), statistics.median(t_b)
        emit({"level": "forward", "batch": batch, "seq": seq, "bge_batch": bbatch, "bge_seq": bseq, "modernbert": spread(t_m), "bge": spread(t_b),
              "modernbert_docs_per_s": round(batch / mm * 1e3, 1), "bge_docs_per_s": round(bbatch / mbg * 1e3, 1),
              "modernbert_tokens_per_s": round(t / mm * 1e3), "bge_tokens_per_s": round(t / mbg * 1e3),
              "modernbert_over_bge_tokens_per_s": round(mbg / mm, 3), "modernbert_plan": mb.prenorm_plan_describe(batch, seq).splitlines()})
        # (c)
        y = torch.randn((1, t, h), generator=g, device=dev)
        r32 = torch.randn((t, h), generator=g, device=dev)
        x16 = torch.empty((t, h), dtype=torch.float16, device=dev)
        gain = torch.ones(h, device=dev)
        qkv = torch.randn((t, 3 * h), generator=g, device=dev).half()
        t_a, t_r = [], []
        for _ in range(args.rounds):
            t_a += timed(lambda: add_layernorm_f32(y, None, None, gain, None, 1e-5, r32, x16), args.reps)
            t_r += timed(lambda: rope_qk_f16(qkv, mb.rope_table, batch, seq, heads), args.reps)
        ma, mr = statistics.median(t_a), statistics.median(t_r)
        emit({"level": "rows", "batch": batch, "seq": seq, "add_layernorm": spread(t_a), "rope": spread(t_r),
              "add_layernorm_gb_per_s": round(10 * t * h / ma / 1e6, 1), "add_layernorm_launches_per_forward": 2 * layers,
              "rope_launches_per_forward": layers, "add_layernorm_share_of_forward": round(2 * layers * ma / mm, 4),
              "rope_share_of_forward": round(layers * mr / mm, 4),
              "note": "isolated launches x count over the forward's median; the forward's add_layernorm reads one fp32 slab (mode-2 GEMM) at these sizes"})
        del y, r32, x16, qkv
    # (b)
    for batch, seq in WINDOW_SHAPES:
        t = batch * seq
        qkv = (torch.randn((t, 3 * h), generator=g, device=dev) * 1.6).half()
        lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
        cw = torch.empty((t, h), dtype=torch.float16, device=dev)
        cb = torch.empty((t, h), dtype=torch.float16, device=dev)
        t_w, t_k = [], []
        for _ in range(args.rounds):
            t_w += timed(lambda: attention_window_f16(qkv, lens, cw, batch, seq, heads, window), args.reps)
            t_k += timed(lambda: attention_f16(qkv, lens, cb, batch, seq, heads, route=3), args.reps)
        mw, mk = statistics.median(t_w), statistics.median(t_k)
        emit({"level": "window", "batch": batch, "seq": seq, "heads": heads, "head_dim": h // heads, "window": window, "windowed": spread(t_w),
              "blocked": spread(t_k), "windowed_over_blocked_time": round(mw / mk, 4), "predicted_by_block_count": round(3.0 / (seq / 64), 4),
              "windowed_range_below_blocked": max(t_w) < min(t_k)})


if __name__ == "__main__":
    main()
