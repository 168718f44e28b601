#!/usr/bin/env python3
"""Timing of the MMR ordering kernel (csrc/mmr.hip) against the host loop it replaces, at two levels.

(a) op:       512 lists of m rows of a ROWS x d fp32 matrix, (m, d) in (10, 384), (20, 384), (40, 768), (64, 384): device events around
              crs::mmr_order_out alone (median of REPS launches after a warm-up) against the wall time of
              ContextRetriever._apply_diversity over the same lists with the same vectors already on the host.
(b) pipeline: RAGPipeline.retrieve_batch, 512 queries, top_k 10, rerank on, diversity_penalty 0.1, on --rows x 384 synthetic rows
              (the row count is part of every line), mmr_vectors 'auto' (the host loop: the baseline) and 'device' alternating in
              one process, REPS repetitions after a warm-up, median [min - max] of the call, and of the time the call spends in
              its MMR step (rows_f32 gather + Python loop / pack + launch + readback + reorder).
One JSON line per case to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

OP_CASES = ((10, 384), (20, 384), (40, 768), (64, 384))
WORDS = ("retrieval augmented generation language model quantization weights perplexity attention embedding cosine similarity "
         "vector index chunk context answer question compression memory latency throughput accuracy benchmark kernel").split()


class _NoStore:
    collection = None


def spread(ts):
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": len(ts)}


def bench_op(args, out):
    import numpy as np
    import torch
    from rag import _native as nat
    from rag.retrieval import ContextRetriever
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    lam, nq = 0.9, 512
    host = ContextRetriever(_NoStore(), None, {"diversity_penalty": 1.0 - lam})
    for m, d in OP_CASES:
        g = torch.Generator(device=dev).manual_seed(m * 1000 + d)
        vecs = torch.nn.functional.normalize(torch.randn((args.op_rows, d), device=dev, generator=g), dim=1).contiguous()
        rows_h = np.stack([rng.choice(args.op_rows, m, replace=False) for _ in range(nq)]).astype(np.int64)
        rel_h = np.sort(rng.random((nq, m)), axis=1)[:, ::-1].copy()
        rows, rel = torch.from_numpy(rows_h).to(dev), torch.from_numpy(rel_h).to(dev)
        counts = torch.full((nq,), m, dtype=torch.int32, device=dev)
        order = torch.empty((nq, m), dtype=torch.int32, device=dev)
        ts = []
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); nat.mmr_order(vecs, args.op_rows, rows, rel, counts, lam, out=order); e1.record()
            torch.cuda.synchronize()
            if rep:
                ts.append(e0.elapsed_time(e1))
        got = order.cpu().numpy()
        vec_h = vecs.cpu().numpy()
        lists = [([{"score": float(s), "pos": j} for j, s in enumerate(rel_h[i])], vec_h[rows_h[i]]) for i in range(nq)]
        th = []
        for rep in range(min(args.reps, 3) + 1):
            t0 = time.perf_counter()
            done = [host._apply_diversity(chunks, vectors=v) for chunks, v in lists]
            if rep:
                th.append((time.perf_counter() - t0) * 1e3)
        same = sum([c["pos"] for c in done[i]] == got[i].tolist() for i in range(nq))
        rec = {"level": "op", "lists": nq, "m": m, "dim": d, "rows": args.op_rows, "lam": lam, "device": spread(ts), "host_loop": spread(th),
               "host_over_device": round(statistics.median(th) / statistics.median(ts), 1), "lists_in_the_host_order": same}
        out.write(json.dumps(rec) + "\n"); out.flush()
        print(json.dumps(rec), flush=True)


def bench_pipeline(args, out):
    import logging
    import numpy as np
    import torch
    logging.disable(logging.WARNING)
    from rag import RAGPipeline
    from rag.chunking import Chunk
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"

    cfg = {"embedding": {"model_name": "synthetic:minilm", "device": "cuda", "batch_size": 64, "normalize": True},
           "retrieval": {"top_k": 10, "similarity_threshold": 0.0, "rerank": True, "diversity_penalty": 0.1, "batch_queries": 64},
           "vector_store": {"collection_name": "bench_mmr"}}
    p = RAGPipeline(cfg)
    p.setup(Stub())
    g = torch.Generator(device=dev); g.manual_seed(1234)
    base_docs = [" ".join(rng.choice(WORDS, size=40)) for _ in range(4096)]
    for lo in range(0, args.rows, 250_000):
        m = min(250_000, args.rows - lo)
        chunks = [Chunk(text=base_docs[(lo + r) & 4095] + f" {lo + r}", chunk_id=f"chunk_{lo + r}", start_char=0, end_char=1) for r in range(m)]
        p.vector_store.create_index(chunks, torch.randn((m, 384), generator=g, device=dev))
    torch.cuda.synchronize()
    queries = [" ".join(rng.choice(WORDS, size=int(rng.integers(5, 12)))) for _ in range(512)]
    r = p.retriever
    in_mmr = [0.0]

    def clocked(name):
        inner = getattr(r, name)

        def wrapped(*a, **kw):
            t0 = time.perf_counter()
            try:
                return inner(*a, **kw)
            finally:
                in_mmr[0] += time.perf_counter() - t0
        setattr(r, name, wrapped)

    clocked("_mmr_on_device")
    clocked("_apply_diversity")
    store = p.vector_store
    gather = store.rows_f32

    def rows_f32(rows):
        t0 = time.perf_counter()
        try:
            return gather(rows)
        finally:
            in_mmr[0] += time.perf_counter() - t0
    store.rows_f32 = rows_f32

    call, step, ran = {"auto": [], "device": []}, {"auto": [], "device": []}, {}
    for rep in range(args.reps + 1):
        for mode in ("auto", "device"):
            r.mmr_vectors = mode
            in_mmr[0] = 0.0
            t0 = time.perf_counter()
            p.retrieve_batch(queries)
            dt = time.perf_counter() - t0
            ran[mode] = dict(r.last_mmr)
            if rep:
                call[mode].append(dt * 1e3); step[mode].append(in_mmr[0] * 1e3)
    for mode in ("auto", "device"):
        med = statistics.median(call[mode])
        rec = {"level": "pipeline", "mmr_vectors": mode, "rows": args.rows, "dim": 384, "queries": len(queries), "top_k": 10, "rerank": True,
               "diversity_penalty": 0.1, "call": spread(call[mode]), "mmr_step": spread(step[mode]), "queries_per_s": round(len(queries) / med * 1e3, 1),
               "last_mmr": ran[mode], "exactness": dict(store.last_exactness)}
        out.write(json.dumps(rec) + "\n"); out.flush()
        print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000, help="pipeline level: corpus rows (C4: 10 M x 384)")
    ap.add_argument("--op-rows", type=int, default=1_000_000, help="op level: rows of the fp32 matrix the lists point into")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--level", default="both", choices=("op", "pipeline", "both"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_mmr.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as out:
        if args.level in ("op", "both"):
            bench_op(args, out)
        if args.level in ("pipeline", "both"):
            bench_pipeline(args, out)


if __name__ == "__main__":
    main()
