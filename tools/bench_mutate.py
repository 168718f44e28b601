#!/usr/bin/env python3
"""Timing of the in-place mutation kernels (csrc/mutate.hip, csrc/row_build.hip) against what a user of the write-once store could do.

Store: ROWS x DIM fp16 + fp32 shadow on one device.  Cases: delete of 10 random rows, 1 % random, 50 % random, the first row only;
update of 1 000 and 100 000 rows.  Per case, REPS repetitions after one warm-up, each on a freshly re-filled store, alternating
in the same process with the baselines:
  in_place     VectorStore.delete / update: device time of the call from events around it (kernels + index tensors)
  index_select the out-of-place way: slab / shadow index_select of the survivors (time and peak memory); deletes only
  rebuild      delete_collection + create_index of the survivors from already-computed embeddings; deletes only
Derived: moved bytes (rows at or above the first dead row x row bytes), moved bytes / time, and the model
4 x moved bytes / 6.29 TB/s (every moved byte is read twice and written twice through the bounce buffer; 6.29 TB/s is the
measured float4 copy rate of the part).  One JSON line per case and variant to --out."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "compressed-rag-suite_amd")):
    sys.path.insert(0, p)

COPY_RATE = 6.29e12


class _C:
    __slots__ = ("chunk_id", "text", "page_number", "section", "tokens")

    def __init__(self, i):
        self.chunk_id, self.text, self.page_number, self.section, self.tokens = f"c{i}", "t", 1, None, 1


def main():
    import numpy as np
    import torch
    from rag.indexing import VectorStore
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06_mutate.jsonl"))
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, dim = args.rows, args.dim
    g = torch.Generator(device=dev).manual_seed(1)
    block = 1_000_000
    chunks = [_C(i) for i in range(n)]
    ids = [c.chunk_id for c in chunks]
    emb_blocks = [torch.randn((min(block, n - lo), dim), device=dev, generator=g) for lo in range(0, n, block)]
    store = VectorStore({"collection_name": "bench_mutate"})

    def fill():
        """(re)build the store's device rows in place: same arrays, n rows"""
        if store.collection is None:
            for b, lo in zip(emb_blocks, range(0, n, block)):
                store.create_index(chunks[lo: lo + b.shape[0]], b)
            return
        col, sh = store.collection, store.collection.shards[0]
        sh.n = 0
        sh.row_err.zero_()
        for b in emb_blocks:
            sh.append(b, sh.n)
        col.ids, col.documents, col.metadatas = list(ids), ["t"] * n, [{"page_number": 1, "tokens": 1} for _ in range(n)]
        col._drop_derived(True)
        col._id_rows()

    from rag import _native as nat
    kernel_ms = []

    def bracket(name):
        """events around the native op alone: the store's call also spends host time on the sidecars, during which the
        device idles; `kernel_ms` is the compaction / scatter itself, `median_ms` the whole call as the stream saw it"""
        inner = getattr(nat, name)

        def wrapped(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); inner(*a, **kw); e1.record()
            kernel_ms.append((e0, e1))
        setattr(nat, name, wrapped)

    bracket("slab_compact")
    bracket("slab_write_rows_f32")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        del kernel_ms[:]
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        timed.kernel = sum(e0.elapsed_time(e1) for e0, e1 in kernel_ms)
        return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base

    rng = np.random.default_rng(0)
    cases = [("delete 10 random", "delete", np.sort(rng.choice(n, 10, replace=False))),
             ("delete 1 % random", "delete", np.sort(rng.choice(n, n // 100, replace=False))),
             ("delete 50 % random", "delete", np.sort(rng.choice(n, n // 2, replace=False))),
             ("delete first row", "delete", np.array([0])),
             ("update 1 000", "update", rng.choice(n, min(n, 1000), replace=False)),
             ("update 100 000", "update", rng.choice(n, min(n, 100_000), replace=False))]
    row_bytes = 2 * store_pdim(dim) + 4 * dim
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as out:
        for name, kind, rows in cases:
            sel = [ids[r] for r in rows]
            new = torch.randn((len(rows), dim), device=dev, generator=g) if kind == "update" else None
            moved = (n - len(rows) - int(rows[0])) * row_bytes if kind == "delete" else len(rows) * row_bytes
            t_in, t_k, t_sel, t_reb, m_in, m_sel = [], [], [], [], 0, 0
            for rep in range(args.reps + 1):
                fill()
                if kind == "delete":
                    ms, mem = timed(lambda: store.delete(ids=sel))
                else:
                    ms, mem = timed(lambda: store.update(sel, embeddings=new))
                if rep:
                    t_in.append(ms); t_k.append(timed.kernel); m_in = max(m_in, mem)
                if kind != "delete" or args.no_baselines:
                    continue
                fill()
                sh = store.collection.shards[0]
                keep = torch.ones(n, dtype=torch.bool, device=dev); keep[torch.from_numpy(rows).to(dev)] = False
                keep = keep.nonzero().flatten()
                res = []
                ms, mem = timed(lambda: res.extend((sh.slab[:n].index_select(0, keep), sh.shadow[:n].index_select(0, keep))))
                del res
                if rep:
                    t_sel.append(ms); m_sel = max(m_sel, mem)
                if rep in (1, 2):      # the rebuild re-allocates the arrays: twice is enough to see its scale
                    keep_h = keep.cpu().numpy()
                    sub = [chunks[r] for r in keep_h.tolist()]
                    survivors = torch.cat(emb_blocks)[keep]

                    def rebuild():
                        store.delete_collection()
                        store.create_index(sub, survivors)
                    ms, _ = timed(rebuild)
                    t_reb.append(ms)
                    del survivors, sub
                    store.delete_collection()
                del keep
                torch.cuda.empty_cache()

            def line(variant, ts, mem=None, kernel=None):
                if not ts:
                    return
                med = statistics.median(ts)
                rec = {"case": name, "variant": variant, "rows": n, "dim": dim, "affected_rows": int(len(rows)), "median_ms": round(med, 4),
                       "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "reps": len(ts), "moved_bytes": int(moved),
                       "moved_GBps": round(moved / med / 1e6, 1), "model_ms": round(4 * moved / COPY_RATE * 1e3, 4) if kind == "delete" else None}
                if kernel:
                    km = statistics.median(kernel)
                    rec.update(kernel_median_ms=round(km, 4), kernel_min_ms=round(min(kernel), 4), kernel_max_ms=round(max(kernel), 4),
                               kernel_moved_GBps=round(moved / km / 1e6, 1))
                if mem is not None:
                    rec["peak_extra_MiB"] = round(mem / 2**20, 1)
                out.write(json.dumps(rec) + "\n"); out.flush()
                print(json.dumps(rec), flush=True)

            line("in_place", t_in, m_in, t_k)
            line("index_select", t_sel, m_sel)
            line("rebuild", t_reb)


def store_pdim(dim):
    from rag import _native as nat
    return nat.padded_dim(dim)


if __name__ == "__main__":
    main()
