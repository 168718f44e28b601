#!/usr/bin/env python3
"""Recall and call time of the ``ivf`` option beside the flat, certified search of the same store.

Two synthetic sets of unit rows: isotropic, and clustered (a Gaussian mixture with nlist / 4 components).  Per set:
  * Recall@10 of search_rows at nprobe 1, 2, 4 .. 64 against the flat answer of the same store object (ivf switched off);
  * time per search_rows call (host clock around a call that ends in the device-to-host copy of its result) at nq 1, 16 and 64,
    ivf and flat alternated call by call in one process after a warm-up of every shape: median and inter-quartile range;
  * what the build cost.
One JSON document on stdout and, with --out, in a file.

    python tools/bench_ivf.py --rows 1000000 --dim 384 --out profiles/ivf_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "compressed-rag-suite_amd"))

NPROBES = (1, 2, 4, 8, 16, 32, 64)


def unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def make_rows(kind, n, dim, components, rng):
    """(rows, sampler of queries): a query is a fresh draw of the rows' own distribution."""
    if kind == "isotropic":
        draw = lambda m: unit(rng.standard_normal((m, dim), dtype=np.float32))
    else:      # unit centres, noise of norm ~0.7 around them
        centres = unit(rng.standard_normal((components, dim), dtype=np.float32))
        draw = lambda m: unit(centres[rng.integers(0, components, m)] + 0.7 / np.sqrt(dim) * rng.standard_normal((m, dim), dtype=np.float32))
    return draw(n), draw


def timed(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def summary(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": round(float(med), 4), "iqr_ms": round(float(q3 - q1), 4)}


def bench_set(kind, args):
    import torch
    from rag.chunking import Chunk
    from rag.indexing import VectorStore
    from rag import _ivf
    rng = np.random.default_rng(args.seed)
    nlist = _ivf.resolve_nlist(_ivf.parse_config({}), args.rows)
    x, draw = make_rows(kind, args.rows, args.dim, max(1, nlist // 4), rng)
    store = VectorStore({"collection_name": f"bench_{kind}", "ivf": {}})
    for r0 in range(0, args.rows, 1 << 17):
        part = x[r0:r0 + (1 << 17)]
        store.create_index([Chunk(text="", chunk_id=str(r0 + i), start_char=0, end_char=0) for i in range(len(part))], part)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = store.ivf_index()
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    print(f"{kind}: {args.rows} rows indexed, {index.nlist} lists built in {build_s:.1f} s", file=sys.stderr, flush=True)
    cfg = store._ivf_cfg

    def flat(q, k=10):
        store._ivf_cfg = None      # the same store object with ivf off
        try:
            return store.search_rows(q, k)
        finally:
            store._ivf_cfg = cfg

    q = draw(args.queries)
    _, want = flat(q)
    recall = {}
    for nprobe in NPROBES:
        store.nprobe = nprobe
        _, got = store.search_rows(q, 10)
        recall[str(nprobe)] = round(float(np.mean([len(set(g) & set(w)) / 10.0 for g, w in zip(got, want)])), 4)
    print(f"{kind}: recall@10 {recall}", file=sys.stderr, flush=True)
    best = recall[str(NPROBES[-1])]
    chosen = next(p for p in NPROBES if recall[str(p)] >= best - 0.01)
    times = {}
    for nprobe in sorted({chosen, 16}):
        store.nprobe = nprobe
        for nq in (1, 16, 64):
            qs = q[:nq]
            for _ in range(args.warmup):
                store.search_rows(qs, 10)
                flat(qs)
            a, b = [], []
            for _ in range(args.reps):      # alternated call by call
                a += timed(lambda: store.search_rows(qs, 10), 1)
                b += timed(lambda: flat(qs), 1)
            times[f"nprobe{nprobe}_nq{nq}"] = {"ivf": summary(a), "flat": summary(b)}
    return {"rows": args.rows, "dim": args.dim, "nlist": index.nlist, "largest_list": int(index.sizes_host.max()),
            "build_s": round(build_s, 2), "recall_at_10": recall, "smallest_nprobe_within_0.01_of_64": chosen, "call_ms": times}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {"tool": "tools/bench_ivf.py", "args": vars(args), "sets": {kind: bench_set(kind, args) for kind in ("isotropic", "clustered")}}
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
