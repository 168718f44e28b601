#!/usr/bin/env python3
"""Timing of the sorted-list merge kernel (csrc/merge_sorted.hip, crs::merge_sorted) against VectorStore._order, the two stable
argsorts + gathers that joined the shards' lists above top_k 64 before it.

Points (nlists, nq, k): (2, 64, 100), (8, 64, 256), (8, 64, 1024), (8, 1, 1024) -- k_in = k_out = k, as _topk_device calls it.
Input: stacked [nlists, nq, k] lists, each sorted (score desc, id asc) with distinct global ids, built once per point on the
device.  Both sides run on the same stacked tensors in ONE process, alternating: per repetition ITERS back-to-back calls of one
side between two device events, then the other side; one untimed warm-up repetition of each, then --reps (5) repetitions; the
median of the per-call times is reported.  The outputs are compared byte for byte before timing.  One JSON line per point to
--out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

POINTS = [(2, 64, 100), (8, 64, 256), (8, 64, 1024), (8, 1, 1024)]


def main():
    import torch
    from rag import _native as nat
    from rag.indexing import VectorStore
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_merge_sorted.jsonl"))
    args = ap.parse_args()
    nat.require_gpu()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(8)
    lines = []
    for nlists, nq, k in POINTS:
        # distinct global ids per query, dealt to the lists; each list ordered by (score desc, id asc) with the path under test's
        # own reference (_order), so the input is what a shard hands in
        ids = torch.stack([torch.randperm(4 * nlists * k, generator=g, device=dev)[: nlists * k] for _ in range(nq)])
        ids = ids.view(nq, nlists, k).permute(1, 0, 2).contiguous()
        sc = torch.randn((nlists, nq, k), generator=g, device=dev)
        s2, i2 = VectorStore._order(sc.view(nlists * nq, k), ids.view(nlists * nq, k), k)
        gs, gi = s2.view(nlists, nq, k).contiguous(), i2.view(nlists, nq, k).contiguous()
        out_s = torch.empty((nq, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((nq, k), dtype=torch.int64, device=dev)

        def kernel():
            return nat.merge_sorted(gs, gi, k, out_s, out_i)

        def order():
            return VectorStore._order(gs.permute(1, 0, 2).reshape(nq, -1), gi.permute(1, 0, 2).reshape(nq, -1), k)

        ks, ki = kernel()
        os_, oi = order()
        torch.cuda.synchronize()
        same = bool(torch.equal(ki, oi) and torch.equal(ks.view(torch.int32), os_.view(torch.int32)))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / args.iters      # us per call

        t_k, t_o = [], []
        for rep in range(args.reps + 1):
            a, b = timed(kernel), timed(order)
            if rep:                                             # repetition 0 is the warm-up
                t_k.append(a)
                t_o.append(b)
        line = {"nlists": nlists, "nq": nq, "k": k, "identical": same, "merge_sorted_us": round(statistics.median(t_k), 2),
                "order_us": round(statistics.median(t_o), 2), "merge_sorted_us_all": [round(x, 2) for x in t_k],
                "order_us_all": [round(x, 2) for x in t_o], "reps": args.reps, "iters": args.iters,
                "device": torch.cuda.get_device_name(0)}
        line["speedup"] = round(line["order_us"] / line["merge_sorted_us"], 2)
        print(json.dumps(line))
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
    return 0 if all(x["identical"] for x in lines) else 1


if __name__ == "__main__":
    sys.exit(main())
