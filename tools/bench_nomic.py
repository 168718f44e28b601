#!/usr/bin/env python3
"""Timing of the rotary, gated encoder family, synthetic weights, tools/bench_sparse.py's conventions: same process,
alternating forms, --rounds rounds of --reps launches each, device events around each form, median [min - max].

(a) forward: synthetic:nomic-embed-text against synthetic:bge (the same H / heads / F / layers) on the same token blocks, every row
             at full length: index side 256 x 128 and 64 x 512, query side 64 x 16.  Nomic's layer has 16 H^2 against 12 H^2 GEMM
             FLOPs per token, so ~0.75x is what arithmetic alone predicts; the measured ratio is reported, it is no pass / fail.
(b) rope:    crs_rope_qk_f16 alone on a [T, 3H] buffer of each shape, times the layer count, as a share of (a)'s nomic forward.
(c) gated:   the fused mode-4 GEMM (the route the forward's plan takes at that row count) against the unfused alternative: a mode-0
             GEMM of the same interleaved weight to fp16 [T, 2F] and silu(gate) * up in torch on its de-interleaved halves.
A JSON array, one record per line, to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

SHAPES = (("index", 256, 128), ("index", 64, 512), ("query", 64, 16))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nomic_bench.json"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import logging
    import numpy as np
    import torch
    logging.disable(logging.WARNING)
    from rag import _native as nat
    from rag._encoder import gemm_f16, gemm_f16_routed, rope_qk_f16
    from rag.embedding import EmbeddingModel
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as out:                    # rewritten after every record: a run cut short keeps what it measured
            out.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")

    dev = torch.device("cuda:0")
    nomic = EmbeddingModel({"model_name": "synthetic:nomic-embed-text", "device": "cuda", "batch_size": 256, "normalize": True}).model
    bge = EmbeddingModel({"model_name": "synthetic:bge", "device": "cuda", "batch_size": 256, "normalize": True}).model
    h, f, layers, heads = nomic.shape.hidden, nomic.shape.ffn, nomic.shape.layers, nomic.shape.heads
    assert (h, f, layers, heads) == (bge.shape.hidden, bge.shape.ffn, bge.shape.layers, bge.shape.heads)
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev); g.manual_seed(6)
    for side, batch, seq in SHAPES:
        t = batch * seq
        ids = torch.from_numpy(rng.integers(1000, 30000, size=(batch, seq)).astype(np.int32)).to(dev)
        lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
        # (a)
        t_n, t_b = [], []
        for _ in range(args.rounds):
            t_n += timed(lambda: nomic.forward(ids, lens), args.reps)
            t_b += timed(lambda: bge.forward(ids, lens), args.reps)
        mn, mb = statistics.median(t_n), statistics.median(t_b)
        plan = nat.encoder_plan_describe(nomic.desc, batch, seq).splitlines()
        emit({"level": "forward", "side": side, "batch": batch, "seq": seq, "nomic": spread(t_n), "bge": spread(t_b),
              "nomic_docs_per_s": round(batch / mn * 1e3, 1), "bge_docs_per_s": round(batch / mb * 1e3, 1),
              "nomic_over_bge_docs_per_s": round(mb / mn, 3), "predicted_by_gemm_flops": 0.75, "nomic_plan": plan})
        # (b)
        qkv = (torch.randn((t, 3 * h), generator=g, device=dev)).half()
        t_r = []
        for _ in range(args.rounds):
            t_r += timed(lambda: rope_qk_f16(qkv, nomic.rope_table, batch, seq, heads), args.reps)
        mr = statistics.median(t_r)
        emit({"level": "rope", "batch": batch, "seq": seq, "per_launch": spread(t_r), "bytes_moved": 8 * t * h,
              "gb_per_s": round(8 * t * h / mr / 1e6, 1), "launches_per_forward": layers,
              "share_of_nomic_forward": round(layers * mr / mn, 4),
              "note": "one isolated launch x layers over the forward's median: launch gaps inside the forward are not in the numerator"})
        # (c)
        a = (torch.randn((t, h), generator=g, device=dev) * 0.5).half()
        w = (torch.randn((2 * f, h), generator=g, device=dev) * 0.05).half()
        up_line = next(ln for ln in plan if "_kernel<4" in ln)
        route = 1 if up_line.startswith("gemm_panel") else 0
        out = torch.empty((t, f), dtype=torch.float16, device=dev)

        def fused():
            gemm_f16_routed(a, w, None, None, out, 4, route, 0)

        def unfused():
            y = gemm_f16(a, w, None, None, 0).view(t, f // 16, 2, 16)
            return (torch.nn.functional.silu(y[:, :, 0].float()) * y[:, :, 1].float()).half().reshape(t, f)

        fused(); ref = unfused(); torch.cuda.synchronize()
        diff = float((out.float() - ref.float()).abs().max())      # the unfused form rounds gate and up to fp16 first
        t_f, t_u = [], []
        for _ in range(args.rounds):
            t_f += timed(fused, args.reps)
            t_u += timed(unfused, args.reps)
        mf, mu = statistics.median(t_f), statistics.median(t_u)
        flop = 2.0 * t * h * 2 * f
        emit({"level": "gated", "batch": batch, "seq": seq, "m": t, "n": 2 * f, "k": h, "fused_kernel": up_line.split()[0], "fused": spread(t_f),
              "unfused": spread(t_u), "fused_range_below_unfused": max(t_f) < min(t_u), "unfused_over_fused": round(mu / mf, 3),
              "fused_tflops": round(flop / mf / 1e9, 1), "unfused_intermediate_bytes": t * 2 * f * 2, "max_abs_diff": round(diff, 5)})


if __name__ == "__main__":
    main()
