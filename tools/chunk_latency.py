#!/usr/bin/env python3
"""Event-timed service time of a fused search chunk on the search lane, in the engine's normal mix (C4 shape by default).

  python tools/chunk_latency.py [--rows N] [--steps S] [--tree DIR]

For every chunk of `steps` timed steps an event is recorded on the search lane in front of ``submit_chunk`` and one behind it
(where the chunk's buffer sets record ``ev_done``): the time from the lane taking the chunk up to its four batches being complete,
the encoder forward it may wait for included.  Prints one JSON line (median / mean / max in ms, chunks per step).
--tree DIR measures another checkout of the project (A/B runs against a parent commit)."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    root = os.path.abspath(args.tree)
    sys.path[:0] = [root, os.path.join(root, "compressed-rag-suite_amd")]
    import numpy as np
    import torch
    from oracle import encoder_ref as er
    from rag import _native as nat
    from rag._encoder import HipEncoder, ModelShape
    from rag._engine import RetrievalEngine, ShardView
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = er.MINILM_L6
    enc = HipEncoder(ModelShape(cfg.vocab_size, cfg.hidden, cfg.layers, cfg.heads, cfg.ffn, cfg.max_pos, cfg.ln_eps, cfg.pooling,
                                cfg.max_seq), er.make_weights(cfg, seed=3), device=dev)
    n, d, qb, seq, k = args.rows, 384, 64, 16, 10
    g = torch.Generator(device=dev).manual_seed(1)
    slab = torch.zeros((n, nat.padded_dim(d)), dtype=torch.float16, device=dev)
    shadow = torch.empty((n, d), dtype=torch.float32, device=dev)
    err = torch.zeros(1, dtype=torch.float32, device=dev)
    for lo in range(0, n, 250_000):
        m = min(250_000, n - lo)
        nat.slab_append_f32(torch.randn((m, d), generator=g, device=dev), slab, lo, nat.SLAB_F16, shadow=shadow, row_err=err)
    eng = RetrievalEngine(enc, ShardView(slab, None, shadow, n, d, nat.SLAB_F16, 0, float(err.item())), qb, seq, k)
    rng = np.random.default_rng(2)
    for i in range(eng.n_ctx):
        ids = rng.integers(1000, 30000, size=(qb, seq)).astype(np.int32)
        ids[:, 0] = 101
        eng.set_tokens(i, ids, np.full(qb, seq, dtype=np.int32))
    eng.warm_up()
    for _ in range(3):
        eng.step()
    torch.cuda.synchronize()
    F, evs = eng.search_fuse, []
    for _ in range(args.steps):
        for i0 in range(0, eng.n_ctx, F):
            st = eng.srch_streams[(eng._issued // F) % eng.n_srch]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            eng.submit_chunk(i0)
            e1.record(st)
            evs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    print(json.dumps({"what": "search-lane time of one fused chunk, lane free -> the chunk's ev_done (ms)", "tree": os.path.basename(root),
                      "rows": n, "batches_per_chunk": F, "lanes": eng.describe_lanes(), "chunks": len(ms),
                      "median_ms": round(statistics.median(ms), 4), "mean_ms": round(statistics.fmean(ms), 4), "max_ms": round(max(ms), 4)}))


if __name__ == "__main__":
    main()
