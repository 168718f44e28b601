#!/usr/bin/env python3
"""Timing of the Qwen3-Embedding encoder family, synthetic weights, tools/bench_modernbert.py's conventions: same
process, alternating forms, --rounds rounds of --reps launches each, device events around each form, median [min - max].

(a) forward: synthetic:qwen3-embedding-0.6b (1024 / 16 query + 8 key-value heads of 128 / ffn 3072 / 28 layers) at 256 x 128 and
             64 x 512 tokens, every row at full length.  Reported, no pass / fail.
(b) kernels: crs_attention_causal_f16, crs_qk_norm_rope_f16 and crs_add_rmsnorm_f32 alone on buffers of each shape, times their
             launches per forward (1, 1 and 2 per layer), as shares of (a)'s forward: isolated launches over the forward's median, so
             launch gaps inside the forward are not in the numerator.
(c) causal:  attention_causal_kernel<64, 2> (16 query heads on 8 key / value heads) against attention_kernel<64, false>
             (crs_attention_f16, route 3) on the SAME Q, K and V, expanded to one key / value head per query head for the blocked
             kernel, 65536 tokens at seq 512 and 2048, beside the block-count prediction (nb + 1) / (2 nb), nb = seq / 64.
A JSON array, one record per line, to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

SHAPES = ((256, 128), (64, 512))
CAUSAL_SHAPES = ((128, 512), (32, 2048))


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
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the forms (at least three)")
    ap.add_argument("--reps", type=int, default=5, help="timed launches per form and round (after 2 warm-up launches)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen3_bench.json"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    import logging
    import numpy as np
    import torch
    logging.disable(logging.WARNING)
    from rag._encoder import add_rmsnorm_f32, attention_causal_f16, attention_f16, qk_norm_rope_f16
    from rag.embedding import EmbeddingModel
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as out:                    # rewritten after every record: a run cut short keeps what it measured
            out.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")

    dev = torch.device("cuda:0")
    qw = EmbeddingModel({"model_name": "synthetic:qwen3-embedding-0.6b", "device": "cuda", "batch_size": 256, "normalize": True}).model
    s = qw.shape
    h, layers, hq, hkv, hd = s.hidden, s.layers, s.heads, s.kv_heads, s.head_dim
    rng = np.random.default_rng(5)
    g = torch.Generator(device=dev); g.manual_seed(6)
    for batch, seq in SHAPES:
        t = batch * seq
        ids = torch.from_numpy(rng.integers(1000, 30000, size=(batch, seq)).astype(np.int32)).to(dev)
        lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
        y = torch.randn((1, t, h), generator=g, device=dev)
        r32 = torch.randn((t, h), generator=g, device=dev)
        x16 = torch.empty((t, h), dtype=torch.float16, device=dev)
        qkv = torch.randn((t, (hq + 2 * hkv) * hd), generator=g, device=dev).half()
        ctx = torch.empty((t, hq * hd), dtype=torch.float16, device=dev)
        gq, gk = qw.qk_gains[0][0], qw.qk_gains[1][0]
        t_f, t_a, t_n, t_r = [], [], [], []
        for _ in range(args.rounds):
            t_f += timed(lambda: qw.forward(ids, lens), args.reps)
            t_a += timed(lambda: attention_causal_f16(qkv, lens, ctx, batch, seq, hq, hkv, hd), args.reps)
            t_n += timed(lambda: qk_norm_rope_f16(qkv, qw.rope_table, gq, gk, 1e-6, batch, seq, hq, hkv), args.reps)
            t_r += timed(lambda: add_rmsnorm_f32(y, r32, qw.final_g, 1e-6, r32, x16), args.reps)
        mf, ma, mn, mr = (statistics.median(x) for x in (t_f, t_a, t_n, t_r))
        emit({"level": "forward", "batch": batch, "seq": seq, "qwen3": spread(t_f), "docs_per_s": round(batch / mf * 1e3, 1),
              "tokens_per_s": round(t / mf * 1e3), "plan": qw.causal_plan_describe(batch, seq).splitlines()})
        emit({"level": "kernels", "batch": batch, "seq": seq, "attention_causal": spread(t_a), "qk_norm_rope": spread(t_n),
              "add_rmsnorm": spread(t_r), "launches_per_forward": {"attention_causal": layers, "qk_norm_rope": layers, "add_rmsnorm": 2 * layers},
              "attention_causal_share_of_forward": round(layers * ma / mf, 4), "qk_norm_rope_share_of_forward": round(layers * mn / mf, 4),
              "add_rmsnorm_share_of_forward": round(2 * layers * mr / mf, 4),
              "note": "isolated launches x count over the forward's median; add_rmsnorm timed on one fp32 slab, in place"})
        del y, r32, x16, qkv, ctx
    # (c) head_dim 64: 16 query heads on 8 key / value heads against the blocked kernel on the expanded buffer
    cq, ckv, chd = 16, 8, 64
    for batch, seq in CAUSAL_SHAPES:
        t = batch * seq
        q = (torch.randn((t, cq, chd), generator=g, device=dev) * 1.6).half()
        k = (torch.randn((t, ckv, chd), generator=g, device=dev) * 1.6).half()
        v = torch.randn((t, ckv, chd), generator=g, device=dev).half()
        grouped = torch.cat([q, k, v], dim=1).reshape(t, -1).contiguous()
        full = torch.cat([q, k.repeat_interleave(cq // ckv, dim=1), v.repeat_interleave(cq // ckv, dim=1)], dim=1).reshape(t, -1).contiguous()
        lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
        cc = torch.empty((t, cq * chd), dtype=torch.float16, device=dev)
        cb = torch.empty((t, cq * chd), dtype=torch.float16, device=dev)
        t_c, t_k = [], []
        for _ in range(args.rounds):
            t_c += timed(lambda: attention_causal_f16(grouped, lens, cc, batch, seq, cq, ckv, chd), args.reps)
            t_k += timed(lambda: attention_f16(full, lens, cb, batch, seq, cq, route=3), args.reps)
        mc, mk = statistics.median(t_c), statistics.median(t_k)
        nb = seq // 64
        emit({"level": "causal", "batch": batch, "seq": seq, "heads": cq, "kv_heads": ckv, "head_dim": chd, "causal": spread(t_c),
              "blocked_full": spread(t_k), "causal_over_blocked_time": round(mc / mk, 4),
              "predicted_by_block_count": round((nb + 1) / (2 * nb), 4), "causal_range_below_blocked": max(t_c) < min(t_k)})


if __name__ == "__main__":
    main()
