"""GPU: top_k 65 .. 1024 on the two multi-GPU drivers of VectorStore (crs::merge_sorted / crs::merge_sorted_wire).

Each shard's list is that shard's exact fp32 top-k (certified or escalated), so the merged list is the exact fp32 top-k of the
whole store and the merge does no arithmetic: a sharded store must return the single-shard store's ids and distance BITS.
  * one process, two shards (devices ["cuda:0", "cuda:0"]) against one shard, fp16 and int8;
  * SPMD, two ranks over gloo on the one card (tests/_large_k_sharded_worker.py), where top_k > 64 raised before;
  * top_k above 1024: a ValueError naming the limit on SPMD, the two stable sorts on the one-process store."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _large_k_sharded_worker as worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128


def _chunks(n):
    from rag.chunking import Chunk
    return [Chunk(text=f"t{r}", chunk_id=f"c_{r}", start_char=0, end_char=1) for r in range(n)]


@pytest.fixture(scope="module")
def data():
    """6000 x 128 unit rows, 5 queries: 40 rows planted within 1e-5 of query 0, 200 exact duplicates of other rows."""
    rng = np.random.default_rng(6000)
    n = 6000
    emb = rng.standard_normal((n, D)).astype(np.float32)
    emb /= np.linalg.norm(emb, axis=1, keepdims=True)
    q = rng.standard_normal((5, D)).astype(np.float32)
    q[1] = emb[11] + 0.1 * q[1]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    planted = rng.choice(n, size=40, replace=False)
    emb[planted] = q[0] + 1e-5 * rng.standard_normal((40, D)).astype(np.float32)
    dup = rng.choice(np.setdiff1d(np.arange(n), planted), size=400, replace=False)
    emb[dup[:200]] = emb[dup[200:]]
    return emb, q


def _same(got, want, what):
    assert got["ids"] == want["ids"], f"{what}: ids differ"
    g, w = np.array(got["distances"], dtype=np.float64), np.array(want["distances"], dtype=np.float64)
    assert g.shape == w.shape and np.array_equal(g.view(np.int64), w.view(np.int64)), f"{what}: distance bits differ"


@pytest.mark.parametrize("dtype", ["fp16", "int8"])
def test_two_shards_in_one_process_equal_one_shard_bit_for_bit(cuda, data, dtype):
    from rag.indexing import VectorStore
    emb, q = data
    cfg = {"index_dtype": dtype, "refine_fp32": True, "refine_exact": True}
    one, two = VectorStore(dict(cfg)), VectorStore(dict(cfg, devices=["cuda:0", "cuda:0"]))
    for st in (one, two):
        st.create_index(_chunks(len(emb)), emb)
    assert len(two.collection.shards) == 2 and len(one.collection.shards) == 1
    for k in (65, 100, 300, 1024):
        got = two.search_batch(q, top_k=k)
        ex = dict(two.last_exactness)
        want = one.search_batch(q, top_k=k)
        assert all(len(ids) == k for ids in got["ids"])
        _same(got, want, f"{dtype} top_k {k}")
        assert ex["mode"] == "certificate" and ex["queries"] == 5, ex
        if dtype == "fp16":
            assert ex["unproven"] == 0, ex


def test_top_k_above_1024_on_two_shards_in_one_process(cuda, data, monkeypatch):
    """Still answered, through VectorStore._order and not through the kernel (its limit is 1024).  The SPMD store's ValueError
    is checked with the two ranks below."""
    from rag import _native as nat
    from rag.indexing import VectorStore
    emb, q = data
    two = VectorStore({"devices": ["cuda:0", "cuda:0"], "refine_fp32": True})
    two.create_index(_chunks(len(emb)), emb)
    calls = []
    merge_sorted = nat.merge_sorted
    monkeypatch.setattr(nat, "merge_sorted", lambda *a, **kw: calls.append(1) or merge_sorted(*a, **kw))
    res = two.search_batch(q, top_k=2000)
    assert not calls
    assert all(len(ids) == 2000 == len(set(ids)) for ids in res["ids"])
    assert all(np.all(np.diff(d) >= 0) for d in res["distances"])
    two.search_batch(q, top_k=1024)
    assert calls == [1]


def test_spmd_two_ranks_equal_one_shard_bit_for_bit(cuda, tmp_path):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29551", os.path.join(ROOT, "tests", "_large_k_sharded_worker.py"), str(tmp_path)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [dict(np.load(tmp_path / f"lists_{rank}.npz")) for rank in range(2)]
    emb, q = worker.make_data()
    small = False
    for name, cfg in worker.CONFIGS:
        want = worker.run_config(cfg, emb, q)
        assert len(want) == 12
        # rank 1's rows after the second and the third add: below top_k 1024 at first
        small |= bool(ranks[1][f"{name}/shard_rows"][0] < 1024)
        for rank in range(2):      # top_k 2000 on the SPMD store: refused, naming the limit
            msg = str(ranks[rank][f"{name}/too_large"])
            assert "top_k 2000" in msg and "1024" in msg, f"{name} rank {rank}: {msg!r}"
        for key, w in want.items():
            for rank in range(2):
                g = ranks[rank][f"{name}/{key}"]
                assert g.shape == w.shape and g.dtype == w.dtype, f"{name}/{key} rank {rank}: {g.shape} vs {w.shape}"
                same = np.array_equal(g.view(np.int64), w.view(np.int64))
                assert same, f"{name}/{key} rank {rank}: differs from the single-shard store at {np.argwhere(g != w)[:5].tolist()}"
        assert want["add2/batch1024/rows"].shape == (worker.NQ, 1024) and want["add1/batch100/rows"].shape == (worker.NQ, 100)
    assert small, "no configuration had a shard smaller than top_k"
