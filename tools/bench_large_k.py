#!/usr/bin/env python3
"""Time VectorStore.search_rows at top_k above and at the scan kernels' 64 on a 10 M x 384 fp16 store.

  python tools/bench_large_k.py [--rows N] [--nq 1,64] [--k 64,100,256,1024] [--iters I] [--warmup W] [--pkg DIR]

Rows are seeded Gaussian rows generated on the device and appended in 250 k-row batches, as bench.py builds its stores (the
slab append normalises them).  Queries: half planted near a row (+ 0.1 noise), half random.  Each (nq, top_k) is warmed up,
then timed with a host clock around search_rows, which ends in a device synchronise (its results come back as numpy).
One JSON line per (nq, top_k): mean / median / min milliseconds per search and the last search's certificate tally
(VectorStore.last_exactness).  --pkg points at another checkout's package directory (A/B against an older tree); a run
without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--nq", default="1,64")
    ap.add_argument("--k", default="64,100,256,1024")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pkg", default=os.path.join(ROOT, "compressed-rag-suite_amd"))
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    import torch
    from rag import _native as nat
    from rag.chunking import Chunk
    from rag.indexing import VectorStore

    nat.require_gpu()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    store = VectorStore({"collection_name": "large-k-bench"})
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    t0 = time.perf_counter()
    for lo in range(0, args.rows, 250_000):
        m = min(250_000, args.rows - lo)
        chunks = [Chunk(text="", chunk_id=f"c{lo + r}", start_char=0, end_char=0) for r in range(m)]
        store.create_index(chunks, torch.randn((m, args.dim), generator=g, device=dev), metadata_fields=[])
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t0
    shadow = store.collection.shards[0].shadow
    nq_max = max(int(x) for x in args.nq.split(","))
    q = torch.randn((nq_max, args.dim), generator=g, device=dev)
    j = torch.randint(0, args.rows, (nq_max,), generator=g, device=dev)
    q[0::2] = shadow[j[0::2]] + 0.1 * q[0::2]
    q = torch.nn.functional.normalize(q, dim=1).cpu().numpy()
    print(json.dumps({"label": args.label, "rows": args.rows, "dim": args.dim, "index_s": round(t_index, 1),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    for nq in (int(x) for x in args.nq.split(",")):
        for k in (int(x) for x in args.k.split(",")):
            qs = q[:nq]
            for _ in range(args.warmup):
                store.search_rows(qs, k)
            ms = []
            for _ in range(args.iters):
                torch.cuda.synchronize()
                t = time.perf_counter()
                store.search_rows(qs, k)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
            print(json.dumps({"label": args.label, "nq": nq, "top_k": k, "iters": args.iters, "ms_mean": round(statistics.mean(ms), 3),
                              "ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3),
                              "exactness": dict(store.last_exactness)}), flush=True)


if __name__ == "__main__":
    main()
