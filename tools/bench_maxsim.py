#!/usr/bin/env python3
"""Throughput of late-interaction re-ranking (rag/late_interaction.py, crs_maxsim) on a synthetic store, against the cross-encoder
of the same encoder shape on the same lists.

  python tools/bench_maxsim.py --out profiles/maxsim_bench.json

A store of --rows chunks of 150-200 words (doc_maxlen 180: about 180 index tokens each) under ``synthetic:colbert-minilm`` (the
MiniLM shape, dim 128); --queries queries of 4-12 words with --cands random candidate rows each.  hipEvent spans after a warm-up,
median of --reps spans of --iters back-to-back calls each, clocks as found:

  index        one pass of VectorStore.token_index() over the whole store: documents/s and tokens/s (host tokenisation + encoder
               + crs_token_project), and beside it the seconds the host tokeniser alone takes for the same texts
  late         LateInteractionReranker.score_rows: the queries' encoder forward + projection + ONE crs_maxsim launch; pairs/s
  cross        CrossEncoderReranker.predict_device (``synthetic:minilm-ce``) over the same (query, chunk text) pairs; pairs/s
  kernel       crs_maxsim alone on pre-encoded queries, for 1, --queries and 4 x --queries lists of --cands candidates: milliseconds,
               pairs/s and the token bytes it reads per second (sum of the candidates' tokens x dimp x 2), beside the 6.29 TB/s
               plain-copy figure of DESIGN 6 -- the SAME lists launch after launch, so these are cache-resident rates
  kernel_rotating   the largest of those shapes over 8 different candidate sets in turn, which together read the index (about 0.7 GB at
               the default --rows, beyond the 256 MB last-level cache) more than twice over: the rate from HBM
  kernel_rotating_by_q_len   the same with every query 16, 32, 48 and 64 tokens long (one to four query row blocks per pair)

A report, not a pass condition."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

COPY_TBPS = 6.29        # plain device copy on this part
WORDS = ("retrieval augmented generation answers questions from compressed documents with a vector index and an encoder on the device "
         "while late interaction keeps one small vector per token of every chunk and scores a query token by token").split()


def span_ms(fn, iters, reps):
    import torch
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return {"median": round(statistics.median(out), 4), "min": round(min(out), 4), "max": round(max(out), 4)}


def run(args):
    import time
    import numpy as np
    import torch
    from rag import _native as nat
    from rag.chunking import Chunk
    from rag.indexing import VectorStore
    from rag.late_interaction import LateInteractionReranker
    from rag.reranking import CrossEncoderReranker
    nat.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device())
    rng = np.random.default_rng(0)
    texts = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(150, 201)))) + f" chunk{r}" for r in range(args.rows)]
    queries = [" ".join(str(w) for w in rng.choice(WORDS, int(rng.integers(4, 13)))) for _ in range(4 * args.queries)]
    store = VectorStore({"collection_name": "maxsim-bench"})
    chunks = [Chunk(text=t, chunk_id=f"c_{r}", start_char=0, end_char=1) for r, t in enumerate(texts)]
    emb = torch.nn.functional.normalize(torch.randn((args.rows, 384), device=dev), dim=1)     # the dense stage is not what is measured
    store.create_index(chunks, emb)
    li = LateInteractionReranker({"model_name": "synthetic:colbert-minilm", "batch_size": 64})
    store.attach_token_encoder(li)
    li.model                                                            # upload
    t0 = time.perf_counter()
    li.tokenize_docs(texts)                                             # what the timed pass spends on the host tokeniser
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = store.token_index()
    torch.cuda.synchronize()
    t_index = time.perf_counter() - t0
    result = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "dimp": li.dimp, "doc_maxlen": li.doc_maxlen,
              "index": {"seconds": round(t_index, 4), "host_tokenise_seconds": round(t_host, 4), "tokens": index.n_tokens, "bytes": index.n_tokens * li.dimp * 2,
                        "docs_per_s": round(args.rows / t_index, 1), "tokens_per_s": round(index.n_tokens / t_index, 1),
                        "mean_tokens_per_doc": round(index.n_tokens / args.rows, 2)}}
    print(json.dumps({"index": result["index"]}), flush=True)

    rows_all = rng.integers(0, args.rows, (4 * args.queries, args.cands)).astype(np.int64)
    nq, m = args.queries, args.cands
    q_main, rows_main = queries[:nq], rows_all[:nq]
    pairs = nq * m
    # late interaction, whole step
    li.score_rows(q_main, rows_main, store)
    t_late = span_ms(lambda: li.score_rows(q_main, rows_main, store), args.iters, args.reps)
    result["late"] = {"queries": nq, "candidates": m, "ms": t_late, "pairs_per_s": round(pairs / (t_late["median"] * 1e-3), 1)}
    print(json.dumps({"late": result["late"]}), flush=True)
    # the cross-encoder on the same lists
    ce = CrossEncoderReranker({"model_name": "synthetic:minilm-ce", "batch_size": 128, "max_seq_length": 256})
    ce_pairs = [(q, texts[r]) for q, rr in zip(q_main, rows_main) for r in rr.tolist()]
    ce.predict_device(ce_pairs)
    t_ce = span_ms(lambda: ce.predict_device(ce_pairs), 1, max(3, args.reps // 2))
    result["cross"] = {"pairs": pairs, "ms": t_ce, "pairs_per_s": round(pairs / (t_ce["median"] * 1e-3), 1)}
    result["late_over_cross"] = round(result["late"]["pairs_per_s"] / result["cross"]["pairs_per_s"], 2)
    print(json.dumps({"cross": result["cross"], "late_over_cross": result["late_over_cross"]}), flush=True)
    # the kernel alone
    result["kernel"] = []
    counts = np.diff(index.offsets)
    for n in (1, nq, 4 * nq):
        q16, q_len = li.encode_queries_device(queries[:n])
        rows_d = torch.from_numpy(rows_all[:n]).to(dev)
        out = torch.empty((n, m), dtype=torch.float32, device=dev)
        fn = lambda: nat.maxsim(q16, q_len, index.tok16, index.n_tokens, index.offsets_dev, index.n_rows, rows_d, out=out)
        fn()
        t = span_ms(fn, max(args.iters, 20), args.reps)
        tok_bytes = int(counts[rows_all[:n]].sum()) * li.dimp * 2
        gbps = tok_bytes / (t["median"] * 1e-3) / 1e9
        result["kernel"].append({"queries": n, "candidates": m, "mean_q_len": round(float(q_len.float().mean().item()), 2), "ms": t,
                                 "pairs_per_s": round(n * m / (t["median"] * 1e-3), 1), "token_bytes": tok_bytes,
                                 "token_gb_per_s": round(gbps, 2), "share_of_plain_copy": round(gbps / (COPY_TBPS * 1e3), 4),
                                 "plain_copy_tb_per_s": COPY_TBPS})
        print(json.dumps(result["kernel"][-1]), flush=True)
    # the same launch shape over ROTATING candidate sets: the sets together cover the index several times over, so a launch finds
    # little of what it reads in the caches (the repeated launch above re-reads one set, which the 256 MB last-level cache can hold)
    n, sets = 4 * nq, 8
    q16, q_len = li.encode_queries_device(queries[:n])
    rot = [torch.from_numpy(rng.integers(0, args.rows, (n, m)).astype(np.int64)).to(dev) for _ in range(sets)]
    out = torch.empty((n, m), dtype=torch.float32, device=dev)
    tok_bytes = sum(int(counts[r.cpu().numpy()].sum()) for r in rot) * li.dimp * 2

    def measure(q16, q_len):
        def cycle():
            for r in rot:
                nat.maxsim(q16, q_len, index.tok16, index.n_tokens, index.offsets_dev, index.n_rows, r, out=out)
        cycle()
        t = span_ms(cycle, 2, args.reps)
        gbps = tok_bytes / (t["median"] * 1e-3) / 1e9
        return {"queries": n, "candidates": m, "sets": sets, "mean_q_len": round(float(q_len.float().mean().item()), 2),
                "ms_per_cycle": t, "ms_per_launch": round(t["median"] / sets, 4), "token_bytes_per_cycle": tok_bytes,
                "index_bytes": index.n_tokens * li.dimp * 2, "pairs_per_s": round(sets * n * m / (t["median"] * 1e-3), 1),
                "token_gb_per_s": round(gbps, 2), "share_of_plain_copy": round(gbps / (COPY_TBPS * 1e3), 4),
                "plain_copy_tb_per_s": COPY_TBPS}

    result["kernel_rotating"] = measure(q16, q_len)
    print(json.dumps({"kernel_rotating": result["kernel_rotating"]}), flush=True)
    # longer queries: the encoded ones above run ONE of the kernel's four query row blocks (4-12 words + [CLS] [SEP]); query_maxlen
    # 32 (ColBERT's default with query_augment) runs two and 64 all four, at the same token bytes.  Random unit vectors: the time
    # does not depend on the values
    result["kernel_rotating_by_q_len"] = []
    for lq in (16, 32, 48, 64):
        qr = torch.nn.functional.normalize(torch.randn((n, lq, li.dimp), device=dev), dim=2).half().contiguous()
        result["kernel_rotating_by_q_len"].append(measure(qr, torch.full((n,), lq, dtype=torch.int32, device=dev)))
        print(json.dumps({"kernel_rotating_by_q_len": result["kernel_rotating_by_q_len"][-1]}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--queries", type=int, default=64)
    ap.add_argument("--cands", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out")
    args = ap.parse_args()
    result = run(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
