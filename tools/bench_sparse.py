#!/usr/bin/env python3
"""Timing of learned sparse retrieval: the MLM head with the max-pool epilogue (csrc/mlm_pool.hip), what it adds to an
encoder forward, and the impact scan (csrc/sparse_scan.hip).

(a) head:    crs_mlm_sparse_pool (zeroing + transform + projection/max-pool + log1p: four launches) against the UNFUSED chain built
             from what the library already had -- crs_gemm_f16 mode 1 (GELU) + torch layer_norm for the transform, crs_gemm_f16
             mode 0 writing the fp16 logits [tokens, V], torch amax over the sequence, torch log1p(relu) -- at the splade-base shape
             (H 768, V 30522), 64 x 256 and 64 x 32 tokens, every text at full length (the chain then needs no mask: its best case).
             Same process, alternating, --rounds rounds of --reps launches each, device events around each form.  Reported: median
             [min - max] per form, the bytes each form must move (computed from the shapes below, not measured) and the achieved
             FLOP/s of the whole head (2 tokens H (H + V) over the median).
(b) encode:  SparseEncoder('synthetic:splade-base').encode_docs_device against EmbeddingModel('synthetic:bge-base-en-v1.5')
             .embed_device over the same --docs seeded texts (the same layer stack: the difference is the head and the compaction).
(c) scan:    crs::sparse_topk, 64 queries x 64 terms, top_k 10, over --scan-rows rows x 128 terms (ids stratified over V 30522),
             next to crs::bm25_topk on the SAME offsets and ids (tf 1, length 128): the BM25 kernel's work minus a division a term.
A JSON array, one record per line, to --out."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

H, V = 768, 30522


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


def bench_head(args, emit):
    import torch
    from rag import _native as nat
    from rag._encoder import gemm_f16
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(1)
    w_t = (torch.randn((H, H), generator=g, device=dev) / H ** 0.5).half()
    w_d = (torch.randn((V, H), generator=g, device=dev) * 0.05).half()
    b_t, gamma, beta = torch.zeros(H, device=dev), torch.ones(H, device=dev), torch.zeros(H, device=dev)
    bias = torch.full((V,), -4.0, device=dev)
    Vc = (V + 255) // 256 * 256                        # the library GEMM's tiles are 256 columns wide: the chain gets zero rows up to there
    w_dc = torch.zeros((Vc, H), dtype=torch.float16, device=dev)
    w_dc[:V] = w_d
    bias_c = torch.full((Vc,), -4.0, device=dev)
    for batch, seq in ((64, 256), (64, 32)):
        tokens = batch * seq
        hidden = torch.randn((batch, seq, H), generator=g, device=dev)
        lens = torch.full((batch,), seq, dtype=torch.int32, device=dev)
        ws = torch.empty(nat.mlm_workspace_bytes(batch, seq, H, V), dtype=torch.uint8, device=dev)
        out = torch.empty((batch, V), dtype=torch.float32, device=dev)

        def fused():
            nat.mlm_sparse_pool(hidden, lens, w_t, b_t, gamma, beta, 1e-12, w_d, bias, 512, ws, out)

        def chain():
            x = gemm_f16(hidden.view(tokens, H).half(), w_t, b_t, None, 1)
            t = torch.nn.functional.layer_norm(x.float(), (H,), gamma, beta, 1e-12).half()
            logits = gemm_f16(t, w_dc, bias_c, None, 0)                    # fp16 [tokens, Vc]: the matrix the fused form never writes
            return torch.log1p(torch.relu(logits.view(batch, seq, Vc).amax(1).float()))[:, :V]

        fused(); ref = chain(); torch.cuda.synchronize()
        diff = float((out - ref).abs().max())                              # the chain rounds its logits to fp16: agreement to ~1e-3
        t_f, t_c = [], []
        for _ in range(args.rounds):
            t_f += timed(fused, args.reps)
            t_c += timed(chain, args.reps)
        flop = 2.0 * tokens * H * (H + V)
        by_fused = tokens * H * 4 + tokens * H * 2 * 2 + V * H * 2 + batch * V * 4 * 3
        by_chain = tokens * H * (4 + 2) + tokens * H * (2 + 4 + 4 + 2) + tokens * H * 2 + V * H * 2 + tokens * V * 2 * 2 + batch * V * (2 + 4 + 4)
        mf, mc = statistics.median(t_f), statistics.median(t_c)
        emit({"level": "head", "batch": batch, "seq": seq, "hidden": H, "vocab": V, "fused": spread(t_f), "chain": spread(t_c),
              "fused_range_below_chain": max(t_f) < min(t_c), "chain_over_fused": round(mc / mf, 3), "flop": flop,
              "fused_tflops": round(flop / mf / 1e9, 1), "chain_tflops": round(flop / mc / 1e9, 1), "fused_min_bytes": by_fused,
              "chain_min_bytes": by_chain, "fused_workspace_bytes": int(ws.numel()), "chain_logits_bytes": tokens * Vc * 2, "chain_vocab_padded": Vc,
              "max_abs_diff": round(diff, 5)})
        del hidden, ws, out, ref
        torch.cuda.empty_cache()


def bench_encode(args, emit):
    import logging
    import numpy as np
    import torch
    logging.disable(logging.WARNING)
    from rag.embedding import EmbeddingModel
    from rag.sparse import SparseEncoder
    rng = np.random.default_rng(2)
    words = [f"w{t}" for t in range(5000)]
    texts = [" ".join(rng.choice(words, int(rng.integers(40, 200)))) for _ in range(args.docs)]
    sp = SparseEncoder({"model_name": "synthetic:splade-base", "batch_size": 64})
    em = EmbeddingModel({"model_name": "synthetic:bge-base-en-v1.5", "device": "cuda", "batch_size": 64, "normalize": True})

    def run(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    t_s, t_e, counts = [], [], None
    for rep in range(args.rounds + 1):
        a = run(lambda: sp.encode_docs_device(texts))
        b = run(lambda: em.embed_device(texts))
        if rep:
            t_s.append(a); t_e.append(b)
    counts = sp.encode_docs_device(texts[:256])[2].cpu().numpy()
    emit({"level": "encode", "docs": len(texts), "tokens_mean": round(float(np.mean([len(t.split()) for t in texts])) + 2, 1),
          "sparse": spread(t_s), "dense": spread(t_e), "sparse_docs_per_s": round(len(texts) / statistics.median(t_s) * 1e3, 1),
          "dense_docs_per_s": round(len(texts) / statistics.median(t_e) * 1e3, 1), "sparse_over_dense": round(statistics.median(t_s) / statistics.median(t_e), 3),
          "terms_per_doc_median": int(np.median(counts)), "terms_per_doc_max": int(counts.max())})


def bench_scan(args, emit):
    import torch
    from rag import _native as nat
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(3)
    terms, nq, qt, k = 128, 64, 64, 10
    for rows in args.scan_rows:
        step = V // terms
        tok = (torch.arange(terms, device=dev, dtype=torch.int32) * step)[None, :] + \
            torch.randint(0, step, (rows, terms), generator=g, device=dev, dtype=torch.int32)
        tok = tok.reshape(-1).contiguous()
        w = torch.rand(rows * terms, generator=g, device=dev) + 0.01
        off = torch.arange(rows + 1, device=dev, dtype=torch.int64) * terms
        tf = torch.ones(rows * terms, dtype=torch.int32, device=dev)
        dl = torch.full((rows,), terms, dtype=torch.int32, device=dev)
        qstep = V // qt
        q_tok = ((torch.arange(qt, device=dev, dtype=torch.int32) * qstep)[None, :] +
                 torch.randint(0, qstep, (nq, qt), generator=g, device=dev, dtype=torch.int32)).reshape(-1).contiguous()
        q_w = torch.rand(nq * qt, generator=g, device=dev) + 0.01
        q_off = torch.arange(nq + 1, device=dev, dtype=torch.int64) * qt
        ws = torch.empty(nat.sparse_workspace_bytes(nq, k, rows), dtype=torch.uint8, device=dev)
        o_s, o_r = torch.empty((nq, k), device=dev), torch.empty((nq, k), dtype=torch.int64, device=dev)

        def sparse():
            nat.sparse_topk(off, tok, w, rows, q_off, q_tok, q_w, k, ws, o_s, o_r)

        def bm25():
            nat.bm25_topk(off, tok, tf, dl, rows, q_off, q_tok, q_w, 0.375, 0.0087, 2.5, k, ws, o_s, o_r)

        t_s, t_b = [], []
        for _ in range(args.rounds):
            t_s += timed(sparse, args.reps)
            t_b += timed(bm25, args.reps)
        sparse(); torch.cuda.synchronize()
        ms, mb = statistics.median(t_s), statistics.median(t_b)
        csr_bytes = rows * terms * 8 + (rows + 1) * 8
        emit({"level": "scan", "rows": rows, "terms_per_row": terms, "queries": nq, "terms_per_query": qt, "top_k": k, "sparse": spread(t_s),
              "bm25_same_csr": spread(t_b), "sparse_over_bm25": round(ms / mb, 3), "sparse_queries_per_s": round(nq / ms * 1e3, 1),
              "bm25_queries_per_s": round(nq / mb * 1e3, 1), "csr_bytes": csr_bytes, "csr_read_gb_per_s": round(csr_bytes / ms / 1e6, 1),
              "hits_in_first_list": int((o_r[0] >= 0).sum())})
        del tok, w, off, tf, dl
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--level", default="all", choices=("head", "encode", "scan", "all"))
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two forms (at least three)")
    ap.add_argument("--reps", type=int, default=5, help="timed launches per form and round (after 2 warm-up launches)")
    ap.add_argument("--docs", type=int, default=1024)
    ap.add_argument("--scan-rows", type=int, nargs="*", default=[1_000_000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_bench.json"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)
        with open(args.out, "w") as out:                    # rewritten after every record: a run cut short keeps what it measured
            out.write("[\n" + ",\n".join(json.dumps(r) for r in records) + "\n]\n")

    if args.level in ("head", "all"):
        bench_head(args, emit)
    if args.level in ("encode", "all"):
        bench_encode(args, emit)
    if args.level in ("scan", "all"):
        bench_scan(args, emit)


if __name__ == "__main__":
    main()
