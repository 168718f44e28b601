#!/usr/bin/env python3
"""Throughput of exact late-interaction retrieval (crs_maxsim_topk, csrc/maxsim_scan.hip).

  python tools/bench_late_scan.py --out profiles/late_scan_bench.json

  kernel      crs_maxsim_topk alone over a synthetic token index of --rows rows of 64..180 random unit tokens at dimp 128, k 10, for
              nq in 8, 64, 256 and every query 16, 32 and 64 tokens long: milliseconds, the token bytes ONE query group streams per
              second (index bytes / time: every group of 8 queries reads the whole index once), the bytes all groups read per
              second, and the MFMA FLOP/s (2 x query tokens padded to 16 x index tokens x dimp), beside the copy bandwidth measured
              on the same buffer (bytes read per second by tensor.copy_ of its first 4 GiB) and the 2.5 PFLOP/s fp16 peak DESIGN uses
  retriever   ContextRetriever.retrieve_batch end to end over a store of --store-rows chunks under ``synthetic:colbert-minilm``,
              first_stage 'dense' against 'scan': queries/s

--token-dtype fp16 | fp8 | both: the index and the queries as fp16 rows, as e4m3 rows (crs_maxsim_topk_f8, csrc/maxsim_scan_f8.hip,
DESIGN 3.23: the same unit vectors times 2^8, rounded by torch's float8_e4m3fn cast), or both ALTERNATELY at every shape in one
job, each fp8 entry then carrying its time as a ratio to the fp16 sweep's.

--token-dtype res2: the fp16, fp8 and 2-bit residual sweeps (crs_maxsim_topk_rc, csrc/maxsim_scan_rc.hip) ALTERNATELY at
every shape in one job.  The res2 index is the same unit rows compressed by crs_token_compress against a codec of --centroids
centroids that rag/_token_codec.py trains on the first 32 x centroids tokens (two k-means iterations: random unit rows have no
clusters to find, the table's size and the spread of the cids over it are what the sweep's gathers see); queries stay fp16.  Its
index bytes are those of the planes and the table as built.  A third section, `overlap`, builds one store per format over
--overlap-rows chunks under ``synthetic:colbert-minilm`` and reports how many of the fp16 top 10 each other format's top 10 holds.

--first-stage centroid (with --token-dtype res2): a fourth section, `centroid`, on the SAME res2 index and in the same job as the res2
sweep: crs_centroid_scores, the crs_centroid_maxsim_topk sweep for 64 candidates and the exact crs_maxsim_rc re-score of those, each
in ms per query beside the exact res2 sweep's, at centroid thresholds 0.5, 0.25 and 0.15; the share of index tokens whose centroid a
query keeps; the cid-plane bytes the sweep reads per second per query group against tensor.copy_ of that plane; and how many of the
exact sweep's top 10 the final top 10 holds.  The queries are document tokens of the index (random unit queries keep nothing at any
of these thresholds).  The `overlap` section then also compares first_stage 'centroid' with 'scan' on the synthetic model.

hipEvent spans after a warm-up, median of --reps spans, clocks as found.  A report, not a pass condition."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

PEAK_FLOPS = 2.5e15
WORDS = ("retrieval augmented generation answers questions from compressed documents with a vector index and an encoder on the device "
         "while late interaction keeps one small vector per token of every chunk and scores a query token by token").split()


def span_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}


def kernel(args, result):
    import numpy as np
    import torch
    from rag import _native as nat
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    dimp, k = 128, 10
    lens = rng.integers(64, 181, args.rows)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev)
    n_tokens = int(lens.sum())
    tok = torch.empty((n_tokens, dimp), dtype=torch.float16, device=dev)
    for lo in range(0, n_tokens, 1 << 22):                                   # random unit rows, a slice at a time
        x = torch.randn((min(1 << 22, n_tokens - lo), dimp), device=dev)
        tok[lo:lo + x.shape[0]] = torch.nn.functional.normalize(x, dim=1).half()
    dtypes = {"both": ("fp16", "fp8"), "res2": ("fp16", "fp8", "res2")}.get(args.token_dtype, (args.token_dtype,))
    f8 = lambda x: (x.float() * 256.0).to(torch.float8_e4m3fn).view(torch.uint8)
    toks = {"fp16": tok, "fp8": f8(tok) if "fp8" in dtypes else None}
    index_bytes = n_tokens * dimp * 2
    rc_index = rc_bytes = None
    if "res2" in dtypes:
        from types import SimpleNamespace
        from rag import _token_codec as tc
        kc = args.centroids
        t0 = time.perf_counter()
        codec = tc.train(tok[: min(n_tokens, 32 * kc)], dimp, kc, {"codec_seed": 0, "kmeans_iters": 2})
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        rc_index = SimpleNamespace(cid=torch.empty(n_tokens, dtype=torch.int32, device=dev),
                                   codes=torch.empty((n_tokens, dimp // 4), dtype=torch.uint8, device=dev),
                                   scale=torch.empty(n_tokens, dtype=torch.float16, device=dev), n_tokens=n_tokens, offsets_dev=offsets,
                                   n_rows=args.rows, codec=codec)
        for lo in range(0, n_tokens, 1 << 22):
            nat.token_compress(tok[lo:lo + (1 << 22)], dimp, codec.centroids, codec.cutoffs, codec.weights, first=lo, cid=rc_index.cid,
                               codes=rc_index.codes, scale=rc_index.scale)
        torch.cuda.synchronize()
        rc_bytes = sum(x.numel() * x.element_size() for x in (rc_index.cid, rc_index.codes, rc_index.scale, codec.centroids))
        assert rc_bytes == tc.index_bytes(n_tokens, dimp, kc)
        used = int(torch.unique(rc_index.cid).numel())
        result["res2_index"] = {"centroids": kc, "bytes": rc_bytes, "bytes_per_token": round(rc_bytes / n_tokens, 2),
                                "ratio_to_fp16_bytes": round(rc_bytes / index_bytes, 4), "centroids_in_use": used,
                                "train_s": round(t1 - t0, 2), "compress_s": round(time.perf_counter() - t1, 2),
                                "cutoffs": [round(float(x), 5) for x in codec.cutoffs], "weights": [round(float(x), 5) for x in codec.weights]}
        print(json.dumps({"res2_index": result["res2_index"]}), flush=True)
    part = tok[: min(n_tokens, (4 << 30) // (dimp * 2))]
    scratch = torch.empty_like(part)
    scratch.copy_(part)
    t = span_ms(lambda: scratch.copy_(part), args.reps)
    del scratch
    copy_gbps = part.numel() * 2 / (t["median"] * 1e-3) / 1e9
    result["index"] = {"rows": args.rows, "tokens": n_tokens, "bytes": index_bytes, "dimp": dimp, "copy_read_gb_per_s": round(copy_gbps, 1)}
    print(json.dumps({"index": result["index"]}), flush=True)
    result["kernel"] = []
    for nq in (8, 64, 256):
        for lq in (16, 32, 64):
            q16 = torch.nn.functional.normalize(torch.randn((nq, lq, dimp), device=dev), dim=2).half().contiguous()
            q_len = torch.full((nq,), lq, dtype=torch.int32, device=dev)
            base = None
            for dt in dtypes:
                is8 = dt == "fp8"
                if dt == "res2":
                    nbytes = rc_bytes
                    ws = torch.empty(nat.maxsim_topk_rc_workspace_bytes(nq, k, args.rows), dtype=torch.uint8, device=dev)
                    fn = lambda: nat.maxsim_topk_rc(q16, q_len, rc_index, k, workspace=ws)
                    plan = nat.maxsim_topk_rc_plan_describe(nq, lq, dimp, k, args.rows)
                else:
                    qx, tx, nbytes = (f8(q16), toks["fp8"], index_bytes // 2) if is8 else (q16, tok, index_bytes)
                    ws = torch.empty(nat.maxsim_topk_workspace_bytes(nq, k, args.rows, f8=is8), dtype=torch.uint8, device=dev)
                    fn = lambda: nat.maxsim_topk(qx, q_len, tx, n_tokens, offsets, args.rows, k, workspace=ws)
                    plan = nat.maxsim_topk_plan_describe(nq, lq, dimp, k, args.rows, f8=is8)
                fn()
                t = span_ms(fn, args.reps)
                sec, groups = t["median"] * 1e-3, (nq + 7) // 8
                flops = 2.0 * nq * lq * n_tokens * dimp
                entry = {"token_dtype": dt, "nq": nq, "q_len": lq, "ms": t, "plan": plan,
                         "ms_per_query": round(t["median"] / nq, 4),
                         "gb_per_s_per_query_group": round(nbytes / sec / 1e9, 1),
                         "gb_per_s_all_groups": round(groups * nbytes / sec / 1e9, 1),
                         "copy_read_gb_per_s": round(copy_gbps, 1), "tflop_per_s": round(flops / sec / 1e12, 1),
                         "share_of_peak": round(flops / sec / PEAK_FLOPS, 4), "queries_per_s": round(nq / sec, 1)}
                if dt != "fp16" and base:
                    entry["time_ratio_to_fp16"] = round(t["median"] / base, 3)
                base = t["median"] if dt == "fp16" else base
                result["kernel"].append(entry)
                print(json.dumps(entry), flush=True)
    return tok, rc_index


def centroid(args, result, tok, index):
    """The pruned centroid-interaction first stage against the exact res2 sweep, on one index in one job."""
    import torch
    from rag import _native as nat
    dev, dimp, k, cand, lq = tok.device, tok.shape[1], 10, 64, 32
    cent = index.codec.centroids
    scratch = torch.empty_like(index.cid)
    scratch.copy_(index.cid)
    t = span_ms(lambda: scratch.copy_(index.cid), args.reps)
    del scratch
    cid_bytes = index.cid.numel() * 4
    copy_gbps = cid_bytes / (t["median"] * 1e-3) / 1e9
    result["centroid"] = {"cid_plane_bytes": cid_bytes, "cid_copy_read_gb_per_s": round(copy_gbps, 1), "candidates": cand, "runs": []}
    gen = torch.Generator(device=dev).manual_seed(5)
    for nq in (8, 64):
        pick = torch.randint(0, index.n_tokens, (nq * lq,), device=dev, generator=gen)
        q16 = tok[pick].reshape(nq, lq, dimp).contiguous()
        q_len = torch.full((nq,), lq, dtype=torch.int32, device=dev)
        ws = torch.empty(nat.maxsim_topk_rc_workspace_bytes(nq, k, args.rows), dtype=torch.uint8, device=dev)
        exact = lambda: nat.maxsim_topk_rc(q16, q_len, index, k, workspace=ws)
        exact_rows = exact()[1]
        t_exact = span_ms(exact, args.reps)
        s16 = torch.empty((nq, cent.shape[0], lq), dtype=torch.float16, device=dev)
        keep = torch.empty((nq, (cent.shape[0] + 31) // 32), dtype=torch.int32, device=dev)
        ws2 = torch.empty(nat.centroid_maxsim_topk_workspace_bytes(nq, cand, args.rows), dtype=torch.uint8, device=dev)
        for thr in (0.5, 0.25, 0.15):
            f1 = lambda: nat.centroid_scores(q16, q_len, cent, thr, s16=s16, keep=keep)
            f2 = lambda: nat.centroid_maxsim_topk(s16, keep, q_len, lq, index, cand, workspace=ws2)
            f1()
            rows = f2()[1]
            out = torch.empty((nq, cand), dtype=torch.float32, device=dev)
            f3 = lambda: nat.maxsim_rc(q16, q_len, index, rows, out=out)
            f3()
            t1, t2, t3 = span_ms(f1, args.reps), span_ms(f2, args.reps), span_ms(f3, args.reps)
            order = torch.argsort(out, dim=1, descending=True, stable=True)[:, :k]
            final = torch.gather(rows, 1, order).cpu().tolist()
            shared = [len(set(a) & set(b)) / float(k) for a, b in zip(final, exact_rows.cpu().tolist())]
            bits = (keep[:8, :, None] >> torch.arange(32, device=dev, dtype=torch.int32)) & 1       # the first 8 queries: [8, words, 32]
            kept = [float(bits[a].reshape(-1)[index.cid.long()].float().mean()) for a in range(min(nq, 8))]
            groups, sec2 = (nq + 7) // 8, t2["median"] * 1e-3
            total = t1["median"] + t2["median"] + t3["median"]
            entry = {"nq": nq, "q_len": lq, "threshold": thr, "plan": nat.centroid_maxsim_topk_plan_describe(nq, lq, cent.shape[0], cand, args.rows),
                     "ms": {"centroid_scores": t1, "sweep": t2, "rescore": t3, "exact_res2_sweep": t_exact},
                     "ms_per_query": {"centroid_scores": round(t1["median"] / nq, 4), "sweep": round(t2["median"] / nq, 4),
                                      "rescore": round(t3["median"] / nq, 4), "total": round(total / nq, 4),
                                      "exact_res2_sweep": round(t_exact["median"] / nq, 4)},
                     "time_ratio_to_exact_res2_sweep": round(total / t_exact["median"], 3),
                     "share_of_tokens_kept": round(sum(kept) / len(kept), 5),
                     "share_of_centroids_kept": round(float(bits.float().mean()), 5),
                     "cid_gb_per_s_per_query_group": round(cid_bytes / sec2 / 1e9, 1),
                     "cid_gb_per_s_all_groups": round(groups * cid_bytes / sec2 / 1e9, 1),
                     "mean_overlap_at_10_with_exact": round(sum(shared) / len(shared), 3), "least_overlap": min(shared)}
            result["centroid"]["runs"].append(entry)
            print(json.dumps(entry), flush=True)


def overlap(args, result):
    """Top-10 agreement of search_late_batch between token formats on seeded random weights: a report, no retrieval-quality claim."""
    import numpy as np
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"
    rng = np.random.default_rng(1)
    texts = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(60, 181)))) + f" chunk{r}" for r in range(args.overlap_rows)]
    queries = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(4, 13)))) for _ in range(args.queries)]
    lists = {}
    for dt in ("fp16", "fp8", "res2"):
        p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny", "device": "cuda", "batch_size": 256, "normalize": True},
                         "vector_store": {"collection_name": "late-overlap-" + dt},
                         "retrieval": {"top_k": 10, "rerank": True,
                                       "late_interaction": {"model_name": "synthetic:colbert-minilm", "first_stage": "scan", "token_dtype": dt}}})
        p.setup(Stub())
        chunks = [Chunk(text=t, chunk_id=f"c_{r}", start_char=0, end_char=1) for r, t in enumerate(texts)]
        p.vector_store.create_index(chunks, p.embedding_model.embed_chunks_device(chunks))
        lists[dt] = p.vector_store.search_late_batch(queries, top_k=10)["rows"]
        if dt == "res2":
            index = p.vector_store.token_index()
            result["overlap_res2_index"] = {"tokens": index.n_tokens, "centroids": index.codec.n_centroids}
            if args.first_stage == "centroid":      # the same store through the pruned first stage, at the retriever's defaults
                lists["centroid"] = p.vector_store.search_late_batch(queries, top_k=10, candidates=64, threshold=0.5)["rows"]
    result["overlap"] = {"rows": args.overlap_rows, "queries": args.queries, "top_k": 10}
    for dt in ("fp8", "res2"):
        shared = [len(set(a) & set(b)) / 10.0 for a, b in zip(lists["fp16"], lists[dt])]
        result["overlap"][dt] = {"mean_overlap_at_10": round(float(np.mean(shared)), 3), "least": round(min(shared), 2),
                                 "same_first_hit": round(float(np.mean([a[0] == b[0] for a, b in zip(lists["fp16"], lists[dt])])), 3)}
    if "centroid" in lists:
        shared = [len(set(a) & set(b)) / 10.0 for a, b in zip(lists["res2"], lists["centroid"])]
        result["overlap"]["centroid_vs_res2_scan"] = {"mean_overlap_at_10": round(float(np.mean(shared)), 3), "least": round(min(shared), 2),
                                                      "candidates": 64, "threshold": 0.5}
    print(json.dumps({"overlap": result["overlap"]}), flush=True)


def retriever(args, result):
    import numpy as np
    import torch
    from rag import RAGPipeline
    from rag.chunking import Chunk

    class Stub:
        def generate(self, prompt, **kw):
            return "n/a"
    rng = np.random.default_rng(1)
    texts = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(60, 181)))) + f" chunk{r}" for r in range(args.store_rows)]
    queries = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(4, 13)))) for _ in range(args.queries)]
    result["retriever"] = {"rows": args.store_rows, "queries": args.queries, "top_k": 10}
    for stage in ("dense", "scan"):
        p = RAGPipeline({"embedding": {"model_name": "synthetic:tiny", "device": "cuda", "batch_size": 256, "normalize": True},
                         "vector_store": {"collection_name": "late-scan-bench-" + stage},
                         "retrieval": {"top_k": 10, "rerank": True, "similarity_threshold": -1.0, "diversity_penalty": 0.0,
                                       "late_interaction": {"model_name": "synthetic:colbert-minilm", "first_stage": stage,
                                                            "token_dtype": "fp16" if args.token_dtype == "both" else args.token_dtype}}})      # 'res2': the res2 store
        p.setup(Stub())
        chunks = [Chunk(text=t, chunk_id=f"c_{r}", start_char=0, end_char=1) for r, t in enumerate(texts)]
        p.vector_store.create_index(chunks, p.embedding_model.embed_chunks_device(chunks))
        p.vector_store.token_index()
        p.retriever.retrieve_batch(queries)
        spans = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.retriever.retrieve_batch(queries)
            torch.cuda.synchronize()
            spans.append(time.perf_counter() - t0)
        sec = statistics.median(spans)
        result["retriever"][stage] = {"ms": round(sec * 1e3, 3), "queries_per_s": round(args.queries / sec, 1)}
        print(json.dumps({stage: result["retriever"][stage]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--store-rows", type=int, default=16384)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-retriever", action="store_true")
    ap.add_argument("--token-dtype", choices=("fp16", "fp8", "both", "res2"), default="fp16")
    ap.add_argument("--centroids", type=int, default=1 << 17, help="res2: the codec's table (2^17 is the store's default at 1 M chunks)")
    ap.add_argument("--first-stage", choices=("scan", "centroid"), default="scan", help="centroid (with --token-dtype res2): also measure the pruned first stage")
    ap.add_argument("--overlap-rows", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from rag import _native as nat
    nat.require_gpu()
    result = {"device": torch.cuda.get_device_name(torch.cuda.current_device())}
    if args.first_stage == "centroid" and args.token_dtype != "res2":
        ap.error("--first-stage centroid needs --token-dtype res2")
    tok, rc_index = kernel(args, result)
    if args.first_stage == "centroid":
        centroid(args, result, tok, rc_index)
    del tok, rc_index
    if args.token_dtype == "res2":
        overlap(args, result)
    if not args.skip_retriever:
        retriever(args, result)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
