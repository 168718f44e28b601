"""Worker of tests/test_large_k_sharded_gpu.py: one rank of a 2-rank SPMD VectorStore(sharded=True) on the one card (gloo
carries the all-gather).  Every rank runs the searches of `searches()` at top_k above 64 and writes its lists (scores, sidecar
rows) and the message of the error a search at top_k 2000 raises to lists_<rank>.npz; the test compares the ranks with each other and with a single-shard store it builds itself."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

D = 128
N = 2300
ADDS = ((0, 1100), (1100, 1101), (1101, 2300))       # every add is split over the ranks
NQ = 5
# (name, VectorStore config): the certified path (fp16 and int8, escalating) and a store without the fp32 shadow (rag._search.topk_gemm)
CONFIGS = (("fp16", {"index_dtype": "fp16", "refine_fp32": True, "refine_exact": True}),
           ("int8", {"index_dtype": "int8", "refine_fp32": True, "refine_exact": True}),
           ("fp16-slab", {"index_dtype": "fp16", "refine_fp32": False}))


def make_data():
    """2300 x 128 unit rows, 5 queries; 40 rows planted within 1e-5 of query 0 and 60 exact duplicates of other rows, both spread
    over the whole row range (so over both ranks' shards)."""
    import numpy as np
    rng = np.random.default_rng(29551)
    emb = rng.standard_normal((N, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    q = rng.standard_normal((NQ, D)).astype(np.float32)
    q[1] = emb[17] + 0.1 * q[1]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    planted = rng.choice(N, size=40, replace=False)
    emb[planted] = q[0] + 1e-5 * rng.standard_normal((40, D)).astype(np.float32)
    rest = np.setdiff1d(np.arange(N), planted)
    dup = rng.choice(rest, size=120, replace=False)
    emb[dup[:60]] = emb[dup[60:]]
    return emb, q


def chunks(lo, hi):
    from rag.chunking import Chunk
    return [Chunk(text=f"t{r}", chunk_id=f"c_{r}", start_char=0, end_char=1) for r in range(lo, hi)]


def searches(store, q, stage):
    """The lists of one store at one stage (rows added so far), keyed for the comparison: search_batch at top_k 100 and 1024
    (clamped to the count by the store) and search for a single query."""
    import numpy as np
    out = {}
    for k in (100, 1024):
        res = store.search_batch(q, top_k=k)
        out[f"{stage}/batch{k}/rows"] = np.array([[int(x[2:]) for x in ids] for ids in res["ids"]], dtype=np.int64)
        out[f"{stage}/batch{k}/dist"] = np.array(res["distances"], dtype=np.float64)
    one = store.search(q[2], top_k=1024)
    out[f"{stage}/one/rows"] = np.array([int(x[2:]) for x in one["ids"][0]], dtype=np.int64)
    out[f"{stage}/one/dist"] = np.array(one["distances"][0], dtype=np.float64)
    return out


def too_large(store, q):
    """The message of the ValueError a search at top_k 2000 raises ('' = it answered)."""
    try:
        store.search_batch(q, top_k=2000)
    except ValueError as e:
        return str(e)
    return ""


def run_config(cfg, emb, q, shard_rows=None, errors=None):
    """Build the store in the three adds; search after the second (1101 rows: on two ranks each shard is smaller than top_k 1024)
    and after the third."""
    from rag.indexing import VectorStore
    store = VectorStore(dict(cfg))
    out = {}
    for a, (lo, hi) in enumerate(ADDS):
        store.create_index(chunks(lo, hi), emb[lo:hi])
        if a >= 1:
            out.update(searches(store, q, f"add{a}"))
            if shard_rows is not None:
                shard_rows.append(int(store.get_stats()["rows_on_this_gpu"]))
    if errors is not None:
        errors.append(too_large(store, q))
    return out


def main(out_dir):
    import numpy as np
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank = dist.get_rank()
    emb, q = make_data()
    out = {}
    for name, cfg in CONFIGS:
        rows, errors = [], []
        for key, val in run_config(dict(cfg, sharded=True), emb, q, rows, errors).items():
            out[f"{name}/{key}"] = val
        out[f"{name}/shard_rows"] = np.array(rows, dtype=np.int64)
        out[f"{name}/too_large"] = np.array(errors[0])
    np.savez(os.path.join(out_dir, f"lists_{rank}.npz"), **out)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])
