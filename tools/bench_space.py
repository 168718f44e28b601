#!/usr/bin/env python3
"""search_batch throughput of an 'ip' and an 'l2' VectorStore against a cosine store over the SAME rows, and how often their
searches certify or escalate (csrc/space.hip).

(a) throughput: --rows x --dim random rows whose norms are log-normal (sigma --sigma), one store per space, 64 and 256 queries,
                top_k 10: wall time of VectorStore.search_batch (the call ends in a readback), the three stores ALTERNATING rep by rep
                in one process, median [min - max] of --reps calls after a warm-up, as q/s; with each line the certified / escalated
                counts of the last call.  The expectation: ip = cosine plus one small launch (same sweep, same padded row), l2 at
                384 about the ratio of the 512-element to the 384-element sweep.
(b) exactness:  (--exactness) for sigma in 0.1, 0.5 an ip and an l2 store over --rows rows, 8192 random queries in batches of 256,
                top_k 10: the certified / escalated / unproven fractions.  Exactness does not depend on them (escalation restores
                it); the second sweep of an escalated batch is what they cost.
One JSON line per case to stdout and to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

SLICE = 250_000


def _rows(rows, dim, sigma, seed):
    """Slices of fp32 rows on the device: random directions times log-normal norms (median 1)."""
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    for lo in range(0, rows, SLICE):
        m = min(SLICE, rows - lo)
        x = torch.nn.functional.normalize(torch.randn((m, dim), generator=g, device=dev), dim=1)
        yield lo, x * torch.exp(sigma * torch.randn((m, 1), generator=g, device=dev))


def _stores(spaces, rows, dim, sigma, seed, chunks):
    from rag.indexing import VectorStore
    import torch
    stores = {space: VectorStore({"collection_name": f"bench_space_{space}", "space": space}) for space in spaces}
    for lo, x in _rows(rows, dim, sigma, seed):
        for store in stores.values():
            store.create_index(chunks[lo:lo + x.shape[0]], x)
    torch.cuda.synchronize()
    return stores


def _queries(n, dim, seed):
    import torch
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn((n, dim), generator=g, device="cuda:0"), dim=1).contiguous()


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def bench_throughput(args, chunks):
    import torch
    spaces = ("cosine", "ip", "l2")
    stores = _stores(spaces, args.rows, args.dim, args.sigma, 1234, chunks)
    for nq in (64, 256):
        q = _queries(nq, args.dim, 99 + nq)
        times = {space: [] for space in spaces}
        for rep in range(args.reps + 2):                  # two warm-up rounds (plans, workspaces, first launches)
            for space in spaces:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                stores[space].search_batch(q, top_k=10)
                dt = time.perf_counter() - t0
                if rep >= 2:
                    times[space].append(dt)
        for space in spaces:
            ts, col = times[space], stores[space].collection
            ex = stores[space].last_exactness
            emit({"case": "throughput", "space": space, "rows": args.rows, "dim": args.dim, "pdim": col.pdim, "sigma": args.sigma,
                  "norm_scale": col.shards[0].norm_scale_host, "queries": nq, "top_k": 10, "reps": len(ts),
                  "qps_median": round(nq / statistics.median(ts), 1), "qps_min": round(nq / max(ts), 1), "qps_max": round(nq / min(ts), 1),
                  "ms_median": round(1e3 * statistics.median(ts), 4), "certified": ex["certified"], "escalated": ex["escalated"],
                  "unproven": ex["unproven"]}, args.out)
    del stores
    torch.cuda.empty_cache()


def bench_exactness(args, chunks):
    import torch
    from rag import _search
    q = _queries(8192, args.dim, 7)
    for sigma in (0.1, 0.5):
        stores = _stores(("ip", "l2"), args.rows, args.dim, sigma, 4321, chunks)
        for space, store in stores.items():
            total = None
            for lo in range(0, q.shape[0], 256):
                store.search_rows(q[lo:lo + 256], 10)
                total = dict(store.last_exactness) if total is None else _search.add_tallies(total, store.last_exactness)
            n = total["queries"]
            emit({"case": "exactness", "space": space, "rows": args.rows, "dim": args.dim, "sigma": sigma,
                  "norm_scale": store.collection.shards[0].norm_scale_host, "queries": n, "top_k": 10,
                  "certified": round(total["certified"] / n, 5), "escalated": round(total["escalated"] / n, 5),
                  "unproven": round(total["unproven"] / n, 5)}, args.out)
        del stores
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--sigma", type=float, default=0.25, help="log-normal sigma of the row norms of the throughput case")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--exactness", action="store_true", help="also run the certified / escalated fractions (8192 queries, sigma 0.1 and 0.5)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from rag.chunking import Chunk
    chunks = [Chunk(text=f"row {r}", chunk_id=f"c_{r}", start_char=0, end_char=1) for r in range(args.rows)]
    bench_throughput(args, chunks)
    if args.exactness:
        bench_exactness(args, chunks)


if __name__ == "__main__":
    main()
